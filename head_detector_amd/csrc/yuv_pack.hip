// libvghvideo.so (include/vgh_video.h): vghy_pack_rgb -- a u8 [H, W, 3] RGB image packed into the three planes of an 8-bit YUV 4:2:0 frame (NV12, NV21 or
// I420: the destination's pointers, pitches and steps say which), by the integer rule of the header with the coefficients the caller hands over.
// One launch; one lane per 2 x 2 block of pixels: up to four luma samples and one (U, V) pair, stored with one 16-bit access where the destination chroma is
// the interleaved pair of one plane.  Nothing is staged or allocated.
#include "../../include/vgh_video.h"
#include "companion_host.h"
#include "plane_views.h"

namespace {

using namespace companion;

struct PackArgs {
    const uint8_t* src;
    int64_t src_pitch;
    planes::Chan y, c[2];  // the destination planes Y and (U, V); their source side is unused
    int32_t pair;          // 0 = U and V are stored apart; 1 / 2 = U / V is the even, lower byte of interleaved pairs
    int32_t W, H, CW, CH;
    int32_t coef[9];
    int32_t y_offset;
};

__device__ __forceinline__ uint32_t clamp8(int32_t v) { return (uint32_t)min(max(v, 0), 255); }

__global__ __launch_bounds__(256) void pack_kernel(PackArgs a) {
    const int cx = (int)(blockIdx.x * 64u + (threadIdx.x & 63)), cy = (int)(blockIdx.y * 4u + (threadIdx.x >> 6));
    if (cx >= a.CW || cy >= a.CH) return;
    int32_t sum[3] = {0, 0, 0}, m = 0;
    for (int dy = 0; dy < 2; ++dy) {
        const int y = 2 * cy + dy;
        if (y >= a.H) break;
        for (int dx = 0; dx < 2; ++dx) {
            const int x = 2 * cx + dx;
            if (x >= a.W) break;
            const uint8_t* p = a.src + (int64_t)y * a.src_pitch + (int64_t)x * 3;
            const int32_t r = p[0], g = p[1], b = p[2];
            sum[0] += r, sum[1] += g, sum[2] += b, ++m;
            a.y.dst[(int64_t)y * a.y.dpitch + (int64_t)x * a.y.dstep] = (uint8_t)clamp8(a.y_offset + ((a.coef[0] * r + a.coef[1] * g + a.coef[2] * b + 32768) >> 16));
        }
    }
    const int32_t rm = (2 * sum[0] + m) / (2 * m), gm = (2 * sum[1] + m) / (2 * m), bm = (2 * sum[2] + m) / (2 * m);
    const uint32_t u = clamp8(128 + ((a.coef[3] * rm + a.coef[4] * gm + a.coef[5] * bm + 32768) >> 16));
    const uint32_t v = clamp8(128 + ((a.coef[6] * rm + a.coef[7] * gm + a.coef[8] * bm + 32768) >> 16));
    const uint32_t uv[2] = {u, v};
    planes::store(a.c, 2, cx, cy, a.pair, uv);
}

const char* const PACK_PLANES[3] = {"Y", "U", "V"};

// every check, and the kernel's arguments: no HIP call
int pack_plan(const vghy_pack_job* job, PackArgs& a) {
    CH_REQUIRE(job, "pack_rgb: null job");
    const vghy_pack_job& j = *job;
    CH_REQUIRE(j.src_dev, "pack_rgb: null image");
    CH_REQUIRE(j.height >= 1 && j.width >= 1 && j.height <= VGHY_MAX_SIDE && j.width <= VGHY_MAX_SIDE, "pack_rgb: image %d x %d outside 1 .. %d", j.height, j.width, VGHY_MAX_SIDE);
    const int64_t H = j.height, W = j.width, CH = (H + 1) / 2, CW = (W + 1) / 2;
    CH_REQUIRE(j.src_pitch_bytes >= W * 3, "pack_rgb: src_pitch_bytes %lld < width * 3 = %lld", (long long)j.src_pitch_bytes, (long long)W * 3);
    CH_REQUIRE(j.src_pitch_bytes <= ((int64_t)1 << 40), "pack_rgb: src_pitch_bytes %lld is too large", (long long)j.src_pitch_bytes);
    CH_REQUIRE(j.y_offset >= 0 && j.y_offset <= 255, "pack_rgb: y_offset %d outside 0 .. 255", j.y_offset);
    for (int k = 0; k < 9; ++k) CH_REQUIRE(j.coef[k] >= -(1 << 20) && j.coef[k] <= (1 << 20), "pack_rgb: coefficient %d is %d, beyond +-2^20", k, j.coef[k]);
    const uintptr_t s0 = (uintptr_t)j.src_dev, s1 = s0 + (uintptr_t)((H - 1) * j.src_pitch_bytes + W * 3);
    char why[400];
    for (int k = 0; k < 3; ++k) {
        const vghy_plane& q = j.planes[k];
        const int64_t pw = k ? CW : W, ph = k ? CH : H;
        CH_REQUIRE(q.dst_dev, "pack_rgb: plane %s: null plane", PACK_PLANES[k]);
        CH_REQUIRE(q.src_dev == nullptr && q.src_pitch == 0 && q.src_step == 0, "pack_rgb: plane %s: the src_ fields of a destination plane are not 0", PACK_PLANES[k]);
        CH_REQUIRE(q.dst_step == 1 || q.dst_step == 2, "pack_rgb: plane %s: step %d is not 1 or 2", PACK_PLANES[k], q.dst_step);
        CH_REQUIRE(!planes::check_pitch(q.dst_pitch, q.dst_step, pw, "pack_rgb", PACK_PLANES[k], "dst", why, sizeof(why)), "%s", why);
        uintptr_t d0, d1;
        planes::plane_range(q.dst_dev, q.dst_pitch, q.dst_step, pw, ph, d0, d1);
        CH_REQUIRE(d1 <= s0 || s1 <= d0, "pack_rgb: plane %s overlaps the source image (the source is never modified)", PACK_PLANES[k]);
        (k ? a.c[k - 1] : a.y) = planes::chan_of(q);
    }
    a.src = j.src_dev, a.src_pitch = j.src_pitch_bytes;
    a.W = (int32_t)W, a.H = (int32_t)H, a.CW = (int32_t)CW, a.CH = (int32_t)CH;
    for (int k = 0; k < 9; ++k) a.coef[k] = j.coef[k];
    a.y_offset = j.y_offset;
    a.pair = planes::pair_of(a.c[0].dst, a.c[1].dst, a.c[0].dpitch, a.c[1].dpitch, a.c[0].dstep, a.c[1].dstep);
    return OK;
}

}  // namespace

extern "C" VGHY_API int vghy_pack_rgb(const vghy_pack_job* job, void* stream) {
    PackArgs a;
    if (int rc = pack_plan(job, a)) return rc;  // everything is checked before anything is queued
    hipLaunchKernelGGL(pack_kernel, dim3((a.CW + 63) / 64, (a.CH + 3) / 4), dim3(256), 0, (hipStream_t)stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("pack_rgb: launch -> %s", hipGetErrorString(e));
        return ERR_HIP;
    }
    return OK;
}
