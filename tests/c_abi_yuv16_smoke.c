/* C-only client of libvgh.so on a 10-bit video frame as a hardware decoder delivers it (no Python, no torch, no colour conversion of its own): vgh_create from a
 * .vghpack, ONE P010 surface uploaded as it is, one vgh_ctx_detect(..., VGH_IMG_YUV420P16_RAW, ...); every result written as raw little-endian arrays.
 * tests/test_gpu_yuv16.py::test_c_only_client_on_a_p010_frame compiles this with plain gcc, runs it and compares the bytes with the Python path.
 *   c_abi_yuv16_smoke <pack> <frame.bin> <conf> <out_prefix>
 * frame.bin: {int32 h, w; int64 pitch, uv_offset, bytes; int32 bit_depth, shift, y_offset, cy, crv, cgu, cgv, cbu; `bytes` surface bytes}. */
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vgh.h"

#define CHECK_HIP(e)                                                                            \
    do {                                                                                        \
        hipError_t _e = (e);                                                                    \
        if (_e != hipSuccess) {                                                                 \
            fprintf(stderr, "%s:%d hip error %s\n", __FILE__, __LINE__, hipGetErrorString(_e)); \
            return 2;                                                                           \
        }                                                                                       \
    } while (0)

static int dump(const char* prefix, const char* name, const void* dev, size_t bytes) {
    char path[1024];
    void* host = malloc(bytes ? bytes : 1);
    FILE* f;
    if (hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    snprintf(path, sizeof(path), "%s.%s", prefix, name);
    f = fopen(path, "wb");
    if (!f) return 1;
    fwrite(host, 1, bytes, f);
    fclose(f);
    free(host);
    return 0;
}

int main(int argc, char** argv) {
    vgh_config cfg;
    vgh_ctx* ctx = NULL;
    vgh_ctx_info info;
    vgh_detect_out out;
    vgh_yuv420p16_image frame;
    int32_t hw[2], coef[8];
    int64_t geo[3];
    int rc, cap;
    float conf;
    FILE* f;
    void *host, *dev;
    const float* unpad;
    if (argc != 5) {
        fprintf(stderr, "usage: %s pack frame.bin conf out_prefix\n", argv[0]);
        return 1;
    }
    if (vgh_abi_version() != VGH_ABI_VERSION) {
        fprintf(stderr, "libvgh.so has ABI revision %d, vgh.h %d\n", vgh_abi_version(), VGH_ABI_VERSION);
        return 1;
    }
    conf = (float)atof(argv[3]);
    memset(&cfg, 0, sizeof(cfg));
    cfg.device = 0;
    cfg.pack_path = argv[1];
    cfg.max_batch = 1;
    rc = vgh_create(&cfg, &ctx);
    if (rc != VGH_OK) {
        fprintf(stderr, "vgh_create failed (%d): %s\n", rc, vgh_last_error());
        return 3;
    }
    if (vgh_ctx_get_info(ctx, &info) != VGH_OK) return 3;
    /* the surface as it is: one device allocation, luma rows `pitch` apart, the interleaved chroma plane at uv_offset with the same pitch */
    f = fopen(argv[2], "rb");
    if (!f) return 1;
    if (fread(hw, 4, 2, f) != 2 || fread(geo, 8, 3, f) != 3 || fread(coef, 4, 8, f) != 8) return 1;
    host = malloc((size_t)geo[2]);
    if (fread(host, 1, (size_t)geo[2], f) != (size_t)geo[2]) return 1;
    fclose(f);
    CHECK_HIP(hipMalloc(&dev, (size_t)geo[2]));
    CHECK_HIP(hipMemcpy(dev, host, (size_t)geo[2], hipMemcpyHostToDevice));
    free(host);
    memset(&frame, 0, sizeof(frame));
    frame.y_dev = (const uint16_t*)dev;
    frame.u_dev = (const uint16_t*)((const char*)dev + geo[1]); /* P010: (U, V) pairs of words */
    frame.v_dev = frame.u_dev + 1;
    frame.h = hw[0];
    frame.w = hw[1];
    frame.y_pitch_bytes = geo[0];
    frame.uv_pitch_bytes = geo[0];
    frame.chroma_step = 4; /* bytes */
    frame.bit_depth = coef[0];
    frame.shift = coef[1];
    frame.y_offset = coef[2];
    frame.cy = coef[3];
    frame.crv = coef[4];
    frame.cgu = coef[5];
    frame.cgv = coef[6];
    frame.cbu = coef[7];
    printf("frame: %d x %d, %d bits >> %d, pitch %lld, chroma at %lld\n", hw[0], hw[1], coef[0], coef[1], (long long)geo[0], (long long)geo[1]);
    cap = info.keep_top_k;
    memset(&out, 0, sizeof(out));
    CHECK_HIP(hipMalloc((void**)&out.boxes_dev, (size_t)cap * 4 * 4));
    CHECK_HIP(hipMalloc((void**)&out.scores_dev, (size_t)cap * 4));
    CHECK_HIP(hipMalloc((void**)&out.flame_dev, (size_t)cap * VGH_NUM_FLAME_PARAMS * 4));
    CHECK_HIP(hipMalloc((void**)&out.counts_dev, 4));
    CHECK_HIP(hipMalloc((void**)&out.n_heads_dev, 4));
    CHECK_HIP(hipMalloc((void**)&out.head_image_dev, (size_t)cap * 4));
    CHECK_HIP(hipMalloc((void**)&out.rpy_dev, (size_t)cap * 3 * 4));
    CHECK_HIP(hipMalloc((void**)&out.proj_dev, (size_t)cap * info.num_vertices * 3 * 4));
    CHECK_HIP(hipMemset(out.proj_dev, 0, (size_t)cap * info.num_vertices * 3 * 4));
    CHECK_HIP(hipMemset(out.rpy_dev, 0, (size_t)cap * 3 * 4));
    CHECK_HIP(hipMemset(out.head_image_dev, 0, (size_t)cap * 4));
    out.head_capacity = cap;
    out.unpad_dev = NULL; /* the FLAME outputs are un-padded with the detector's own table */
    /* an invalid descriptor fails before anything is queued, naming the image */
    frame.chroma_step = 3;
    if (vgh_ctx_detect(ctx, &frame, VGH_IMG_YUV420P16_RAW, 1, conf, 0.5f, &out, NULL) != VGH_ERR_INVALID || !strstr(vgh_ctx_last_error(ctx), "image 0") ||
        !strstr(vgh_ctx_last_error(ctx), "chroma_step")) {
        fprintf(stderr, "expected chroma_step 3 to fail naming image 0, got: %s\n", vgh_ctx_last_error(ctx));
        return 4;
    }
    frame.chroma_step = 4;
    if (vgh_detector_scratch(vgh_ctx_detector(ctx), VGH_SCRATCH_UNPAD) != NULL) {
        fprintf(stderr, "the un-pad table exists before the first raw call\n");
        return 4;
    }
    rc = vgh_ctx_detect(ctx, &frame, VGH_IMG_YUV420P16_RAW, 1, conf, 0.5f, &out, NULL);
    if (rc != VGH_OK) {
        fprintf(stderr, "vgh_ctx_detect failed (%d): %s\n", rc, vgh_ctx_last_error(ctx));
        return 4;
    }
    CHECK_HIP(hipDeviceSynchronize());
    unpad = (const float*)vgh_detector_scratch(vgh_ctx_detector(ctx), VGH_SCRATCH_UNPAD);
    if (!unpad) {
        fprintf(stderr, "VGH_SCRATCH_UNPAD is NULL after a raw call\n");
        return 4;
    }
    if (dump(argv[4], "counts", out.counts_dev, 4) || dump(argv[4], "boxes", out.boxes_dev, (size_t)cap * 16) || dump(argv[4], "scores", out.scores_dev, (size_t)cap * 4) ||
        dump(argv[4], "flame", out.flame_dev, (size_t)cap * VGH_NUM_FLAME_PARAMS * 4) || dump(argv[4], "n_heads", out.n_heads_dev, 4) ||
        dump(argv[4], "head_image", out.head_image_dev, (size_t)cap * 4) || dump(argv[4], "rpy", out.rpy_dev, (size_t)cap * 12) ||
        dump(argv[4], "proj", out.proj_dev, (size_t)cap * info.num_vertices * 12) || dump(argv[4], "unpad", unpad, 12) ||
        dump(argv[4], "canvas", vgh_detector_scratch(vgh_ctx_detector(ctx), VGH_SCRATCH_CANVAS), (size_t)info.image_size * info.image_size * 3))
        return 5;
    vgh_destroy(ctx);
    hipFree(dev);
    printf("ok\n");
    return 0;
}
