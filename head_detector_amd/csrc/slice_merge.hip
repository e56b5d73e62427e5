// libvghmerge.so (include/vgh_merge.h): the cross-tile merge of sliced detection.  The per-tile slabs of vgh_detect (up to 16 384 candidates, live counts on the
// device) become one list of heads in image coordinates; the rule is stated once, in the header, and restated in NumPy by tests/slice_merge_ref.py.
//
//   map     one lane per candidate: clip, the truncation test against the interior edges of its tile, image coordinates, and a 64-bit sort key
//           (~ordered score bits, index); a candidate that is absent or truncated gets a key behind every live one.  Keys are unique.
//   rank    rank by counting: the keys stream through LDS 4096 at a time (32 KB) and every lane counts the keys below its own.  Unique keys make the
//           ranks a permutation, so the scatter into sorted order is deterministic and in bounds by construction.
//   mask    bit (i, j) of the matrix [N, N / 64], j behind i in the order: the tiles differ and the match rule holds.  One 64 x 64 block per workgroup
//           of one wave: the 64 row boxes in LDS, one column box per lane, one ballot per row = one word.
//   scan    ONE wave walks the sorted candidates 64 at a time: the diagonal words of the block in registers (one per lane, passed around with shuffles),
//           the "removed" words of all blocks in LDS.  Only the rows of candidates that are still alive are applied -- A > B > C, A matches B and B
//           matches C: B is removed, its row is never applied, C stays.
//   emit    compaction from the kept bits and the per-block prefix: outputs, the two counters, the statuses, and the fill of the rows behind n_heads.
// Five launches, one memset and one upload whatever the counts are.  Values are written with ordinary vector stores; integer atomics only (the live
// count); every float operation in the stated order with contraction off.
#include <math.h>

#include <map>
#include <mutex>

#include "../../include/vgh_merge.h"
#include "companion_host.h"

#pragma clang fp contract(off)

namespace {

using namespace companion;
static_assert(VGHM_OK == OK && VGHM_ERR_INVALID == ERR_INVALID && VGHM_ERR_HIP == ERR_HIP && VGHM_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

constexpr int WAVE = 64;
constexpr int MAX_WORDS = VGHM_MAX_CANDIDATES / WAVE;  // mask words of a row at the capacity
constexpr int RANK_LANES = 256;
constexpr int RANK_TILE = 4096;  // keys held in LDS at a time: 32 KB
constexpr uint32_t DEAD = 0x80000000u;  // bit 31 of a key's low word: absent or truncated
static_assert(MAX_WORDS == 256 && VGHM_MAX_CANDIDATES % WAVE == 0, "scan_kernel keeps 256 removed words in LDS");
static_assert(RANK_TILE * sizeof(uint64_t) <= 64 * 1024, "static LDS");

struct Tile {  // one row of the plan as the kernels read it: 48 bytes
    int32_t off_x, off_y, w, h, pad_x, pad_y, new_w, new_h;
    float scale;
    uint32_t interior;
    uint32_t unused[2];
};

// the workspace, every part from a 16-byte boundary; n_pad = N rounded up to 64, words = n_pad / 64
struct Layout {
    size_t keys, fbox, st0, sidx, sbox, stile, mask, keptw, prefix, counters, total;
    Layout(size_t n_pad) {
        const size_t words = n_pad / WAVE;
        size_t at = 0;
        auto take = [&](size_t bytes) {
            const size_t here = at;
            at += align16(bytes);
            return here;
        };
        keys = take(n_pad * 8);
        fbox = take(n_pad * 16);
        st0 = take(n_pad);
        sidx = take(n_pad * 4);
        sbox = take(n_pad * 16);
        stile = take(n_pad * 4);
        mask = take(n_pad * words * 8);
        keptw = take(words * 8);
        prefix = take(words * 4);
        counters = take(16);  // [0] live candidates, [1] kept candidates
        total = at;
    }
};

__device__ __forceinline__ float clip(float v, float S) { return fminf(fmaxf(v, 0.0f), S); }

// ---- map ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void map_kernel(const float4* __restrict__ boxes, const float* __restrict__ scores, const int32_t* __restrict__ counts,
                                                  const Tile* __restrict__ tiles, int N, int n_pad, int keep_k, float S, float border,
                                                  uint64_t* __restrict__ keys, float4* __restrict__ fbox, uint8_t* __restrict__ st0, int32_t* __restrict__ n_live) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_pad) return;  // n_pad is a multiple of 64: whole waves leave together
    uint8_t st = VGHM_STATUS_ABSENT;
    float4 f = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    uint32_t hi = 0xffffffffu;
    if (i < N) {
        const int t = i / keep_k, r = i - t * keep_k;
        if (r < counts[t]) {
            const Tile g = tiles[t];
            const float4 b = boxes[i];
            const float x1 = clip(b.x, S), y1 = clip(b.y, S), x2 = clip(b.z, S), y2 = clip(b.w, S);
            const float bs = border * g.scale;
            const float px = (float)g.pad_x, py = (float)g.pad_y;
            const bool cut = ((g.interior & 1u) && x1 < px + bs) || ((g.interior & 2u) && y1 < py + bs) ||
                             ((g.interior & 4u) && x2 > (float)(g.pad_x + g.new_w) - bs) || ((g.interior & 8u) && y2 > (float)(g.pad_y + g.new_h) - bs);
            const float ox = (float)g.off_x, oy = (float)g.off_y;
            f = make_float4(((x1 - px) / g.scale) + ox, ((y1 - py) / g.scale) + oy, ((x2 - px) / g.scale) + ox, ((y2 - py) / g.scale) + oy);
            st = cut ? VGHM_STATUS_TRUNCATED : VGHM_STATUS_KEPT;  // KEPT = live so far
            const uint32_t bits = __float_as_uint(scores[i]);
            hi = ~(bits ^ ((bits & 0x80000000u) ? 0xffffffffu : 0x80000000u));  // ascending key = descending score
        }
    }
    const bool live = st == VGHM_STATUS_KEPT;
    keys[i] = live ? ((uint64_t)hi << 32) | (uint32_t)i : ((uint64_t)0xffffffffu << 32) | DEAD | (uint32_t)i;
    fbox[i] = f;
    st0[i] = st;
    const unsigned long long m = __ballot(live);
    if ((threadIdx.x & (WAVE - 1)) == 0 && m) atomicAdd(n_live, __popcll(m));
}

// ---- rank -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(RANK_LANES) void rank_kernel(const uint64_t* __restrict__ keys, const float4* __restrict__ fbox, int n_pad, int keep_k,
                                                          int32_t* __restrict__ sidx, float4* __restrict__ sbox, int32_t* __restrict__ stile) {
    __shared__ uint64_t s_keys[RANK_TILE];
    const int i = blockIdx.x * RANK_LANES + threadIdx.x;
    const uint64_t mine = i < n_pad ? keys[i] : ~(uint64_t)0;
    int rank = 0;
    for (int base = 0; base < n_pad; base += RANK_TILE) {
        const int n = min(RANK_TILE, n_pad - base);
        for (int k = threadIdx.x; k < n; k += RANK_LANES) s_keys[k] = keys[base + k];
        __syncthreads();
        for (int k = 0; k < n; ++k) rank += s_keys[k] < mine ? 1 : 0;  // every lane reads the same word: a broadcast
        __syncthreads();
    }
    if (i >= n_pad) return;
    // the n_pad keys are distinct, so rank is a permutation of 0 .. n_pad - 1
    sidx[rank] = i;
    sbox[rank] = fbox[i];
    stile[rank] = ((uint32_t)mine & DEAD) ? -1 : i / keep_k;
}

// ---- mask -----------------------------------------------------------------------------------------------------------------------------------------
template <int METRIC>
__device__ __forceinline__ bool matches(const float4 a, const float4 b, const float thr) {
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y);
    const float xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    const float ovr = METRIC == VGHM_METRIC_IOU ? inter / (area_a + area_b - inter) : inter / fminf(area_a, area_b);
    return ovr > thr;  // false for NaN
}

// blockIdx.y = row block, blockIdx.x = column block; only blocks on or above the diagonal with live candidates in both write their 64 words
template <int METRIC>
__global__ __launch_bounds__(WAVE) void mask_kernel(const float4* __restrict__ sbox, const int32_t* __restrict__ stile, const int32_t* __restrict__ n_live_p, int words,
                                                    float thr, uint64_t* __restrict__ mask) {
    const int bi = blockIdx.y, bj = blockIdx.x, lane = threadIdx.x;
    if (bj < bi) return;
    const int n_live = *n_live_p;
    if (bi * WAVE >= n_live || bj * WAVE >= n_live) return;
    __shared__ float4 s_box[WAVE];
    __shared__ int32_t s_tile[WAVE];
    s_box[lane] = sbox[bi * WAVE + lane];  // sorted arrays have n_pad = words * 64 rows
    s_tile[lane] = stile[bi * WAVE + lane];
    const int j = bj * WAVE + lane;
    const float4 cb = sbox[j];
    const int ct = stile[j];
    __syncthreads();
    uint64_t mine = 0;
    for (int r = 0; r < WAVE; ++r) {
        const int gi = bi * WAVE + r;
        const bool match = j > gi && j < n_live && gi < n_live && s_tile[r] != ct && matches<METRIC>(s_box[r], cb, thr);
        const unsigned long long m = __ballot(match);
        if (lane == r) mine = m;
    }
    mask[(size_t)(bi * WAVE + lane) * words + bj] = mine;
}

// ---- scan -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(WAVE) void scan_kernel(const uint64_t* __restrict__ mask, const int32_t* __restrict__ n_live_p, int words, uint64_t* __restrict__ keptw,
                                                    int32_t* __restrict__ prefix, int32_t* __restrict__ n_kept) {
    __shared__ uint64_t s_removed[MAX_WORDS];
    const int lane = threadIdx.x;
    const int n_live = min(*n_live_p, words * WAVE);
    const int blocks = (n_live + WAVE - 1) / WAVE;  // <= words <= MAX_WORDS
    for (int w = lane; w < MAX_WORDS; w += WAVE) s_removed[w] = 0;
    __syncthreads();
    int count = 0;
    for (int b = 0; b < blocks; ++b) {
        const int rows = min(WAVE, n_live - b * WAVE);
        const uint64_t diag = lane < rows ? mask[(size_t)(b * WAVE + lane) * words + b] : 0;
        uint64_t cur = s_removed[b];
        uint64_t kept = 0;
        for (int r = 0; r < rows; ++r) {  // uniform: every lane walks the same 64 candidates
            const uint64_t row = __shfl(diag, r);
            if (!((cur >> r) & 1)) {
                kept |= (uint64_t)1 << r;
                cur |= row;
            }
        }
        if (lane == 0) {
            keptw[b] = kept;
            prefix[b] = count;
        }
        count += __popcll(kept);
        for (int w = b + 1 + lane; w < blocks; w += WAVE) {  // the rows of the block's KEPT candidates, one later word per lane
            uint64_t acc = 0;
            for (uint64_t k = kept; k; k &= k - 1) acc |= mask[(size_t)(b * WAVE + __ffsll((unsigned long long)k) - 1) * words + w];
            s_removed[w] |= acc;
        }
        __syncthreads();
    }
    if (lane == 0) *n_kept = count;
}

// ---- emit -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void emit_kernel(const int32_t* __restrict__ sidx, const float4* __restrict__ sbox, const uint8_t* __restrict__ st0,
                                                   const uint64_t* __restrict__ keptw, const int32_t* __restrict__ prefix, const int32_t* __restrict__ counters,
                                                   const float* __restrict__ scores, int N, int n_pad, int keep_k, int max_heads, int32_t* __restrict__ head_row,
                                                   int32_t* __restrict__ head_tile, float4* __restrict__ boxes_full, float* __restrict__ scores_out,
                                                   int32_t* __restrict__ n_heads_out, int32_t* __restrict__ n_kept_out, uint8_t* __restrict__ status) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const int n_live = min(counters[0], n_pad), n_kept = counters[1];
    const int n_heads = min(n_kept, max_heads);
    if (p == 0) {
        *n_heads_out = n_heads;
        *n_kept_out = n_kept;
    }
    if (p < n_pad) {
        const int i = sidx[p];  // a permutation of 0 .. n_pad - 1
        uint8_t st;
        if (p < n_live) {
            const uint64_t word = keptw[p >> 6];
            const int bit = p & 63;
            if ((word >> bit) & 1) {
                const int pos = prefix[p >> 6] + __popcll(word & (((uint64_t)1 << bit) - 1));
                if (pos < max_heads) {
                    head_row[pos] = i;
                    head_tile[pos] = i / keep_k;
                    boxes_full[pos] = sbox[p];
                    scores_out[pos] = scores[i];  // live, hence i < N
                    st = VGHM_STATUS_KEPT;
                } else {
                    st = VGHM_STATUS_OVER_CAP;
                }
            } else {
                st = VGHM_STATUS_SUPPRESSED;
            }
        } else {
            st = st0[i];  // absent or truncated
        }
        if (status && i < N) status[i] = st;
    }
    if (p < max_heads && p >= n_heads) {
        head_row[p] = -1;
        head_tile[p] = -1;
        boxes_full[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        scores_out[p] = 0.0f;
    }
}

std::mutex g_mutex;
std::map<int, Staging> g_staging;

}  // namespace

extern "C" VGHM_API const char* vghm_version(void) { return "vghmerge 1 (gfx950)"; }

extern "C" VGHM_API const char* vghm_last_error(void) { return last_error(); }

extern "C" VGHM_API int64_t vghm_merge_workspace_bytes(int32_t n_tiles, int32_t keep_k) {
    if (n_tiles < 1 || keep_k < 1 || (int64_t)n_tiles * keep_k > VGHM_MAX_CANDIDATES) return 0;
    const size_t n = (size_t)n_tiles * keep_k;
    return (int64_t)Layout((n + WAVE - 1) / WAVE * WAVE).total;
}

extern "C" VGHM_API int vghm_merge_tiles(const vghm_merge_job* job, void* workspace_dev, void* stream) {
    CH_REQUIRE(job, "merge_tiles: null job");
    const vghm_merge_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(j.n_tiles >= 1, "merge_tiles: n_tiles %d < 1", j.n_tiles);
    CH_REQUIRE(j.keep_k >= 1, "merge_tiles: keep_k %d < 1", j.keep_k);
    CH_REQUIRE((int64_t)j.n_tiles * j.keep_k <= VGHM_MAX_CANDIDATES, "merge_tiles: n_tiles * keep_k = %lld exceeds the %d candidates of one call",
               (long long)j.n_tiles * j.keep_k, VGHM_MAX_CANDIDATES);
    CH_REQUIRE(j.image_size >= 1, "merge_tiles: image_size %d < 1", j.image_size);
    CH_REQUIRE(j.max_heads >= 1 && j.max_heads <= VGHM_MAX_HEADS, "merge_tiles: max_heads %d outside 1 .. %d", j.max_heads, VGHM_MAX_HEADS);
    CH_REQUIRE(j.metric == VGHM_METRIC_IOU || j.metric == VGHM_METRIC_IOS, "merge_tiles: metric %d is neither 0 (iou) nor 1 (ios)", j.metric);
    CH_REQUIRE(isfinite(j.border) && j.border >= 0.0f, "merge_tiles: border %g is not a finite non-negative number", (double)j.border);
    CH_REQUIRE(!isnan(j.match_thr), "merge_tiles: match_thr is NaN");
    CH_REQUIRE(j.boxes_dev, "merge_tiles: null boxes_dev");
    CH_REQUIRE(j.scores_dev, "merge_tiles: null scores_dev");
    CH_REQUIRE(j.counts_dev, "merge_tiles: null counts_dev");
    CH_REQUIRE(j.tiles, "merge_tiles: null tiles");
    CH_REQUIRE(j.scale, "merge_tiles: null scale");
    CH_REQUIRE(j.interior, "merge_tiles: null interior");
    CH_REQUIRE(j.head_row_dev, "merge_tiles: null head_row_dev");
    CH_REQUIRE(j.head_tile_dev, "merge_tiles: null head_tile_dev");
    CH_REQUIRE(j.boxes_full_dev, "merge_tiles: null boxes_full_dev");
    CH_REQUIRE(j.scores_out_dev, "merge_tiles: null scores_out_dev");
    CH_REQUIRE(j.n_heads_dev, "merge_tiles: null n_heads_dev");
    CH_REQUIRE(j.n_kept_uncapped_dev, "merge_tiles: null n_kept_uncapped_dev");
    CH_REQUIRE(workspace_dev, "merge_tiles: null workspace");
    CH_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "merge_tiles: the workspace is not 16-byte aligned");
    CH_REQUIRE(((uintptr_t)j.boxes_dev & 15) == 0 && ((uintptr_t)j.boxes_full_dev & 15) == 0, "merge_tiles: boxes_dev / boxes_full_dev are not 16-byte aligned");
    const int T = j.n_tiles, N = T * j.keep_k;
    for (int t = 0; t < T; ++t)
        CH_REQUIRE(isfinite(j.scale[t]) && j.scale[t] > 0.0f, "merge_tiles: tile %d: scale %g is not a finite positive number", t, (double)j.scale[t]);
    const int n_pad = (N + WAVE - 1) / WAVE * WAVE, words = n_pad / WAVE;
    const Layout at((size_t)n_pad);
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& s = g_staging[device];
    const size_t total = (size_t)T * sizeof(Tile);
    if (int rc = reserve(s, total, "merge_tiles")) return rc;  // also waits for this device's previous call
    Tile* rows = (Tile*)s.host;
    for (int t = 0; t < T; ++t) {
        const int32_t* g = j.tiles + 8 * t;
        rows[t] = Tile{g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], j.scale[t], j.interior[t], {0, 0}};
    }
    // from here on work is queued (companion_host.h, queue-then-record)
    uint8_t* ws = (uint8_t*)workspace_dev;
    uint64_t* keys = (uint64_t*)(ws + at.keys);
    float4* fbox = (float4*)(ws + at.fbox);
    uint8_t* st0 = ws + at.st0;
    int32_t* sidx = (int32_t*)(ws + at.sidx);
    float4* sbox = (float4*)(ws + at.sbox);
    int32_t* stile = (int32_t*)(ws + at.stile);
    uint64_t* mask = (uint64_t*)(ws + at.mask);
    uint64_t* keptw = (uint64_t*)(ws + at.keptw);
    int32_t* prefix = (int32_t*)(ws + at.prefix);
    int32_t* counters = (int32_t*)(ws + at.counters);
    Queue q;
    CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));  // first: whatever follows, the event covers the staging block
    CH_QUEUE(q, hipMemsetAsync(counters, 0, 16, st));
    if (q.ok())
        hipLaunchKernelGGL(map_kernel, dim3((unsigned)(n_pad + 255) / 256), dim3(256), 0, st, (const float4*)j.boxes_dev, j.scores_dev, j.counts_dev, (const Tile*)s.dev, N, n_pad,
                           j.keep_k, (float)j.image_size, j.border, keys, fbox, st0, counters);
    if (q.ok())
        hipLaunchKernelGGL(rank_kernel, dim3((unsigned)(n_pad + RANK_LANES - 1) / RANK_LANES), dim3(RANK_LANES), 0, st, (const uint64_t*)keys, (const float4*)fbox, n_pad, j.keep_k,
                           sidx, sbox, stile);
    if (q.ok()) {
        auto kernel = j.metric == VGHM_METRIC_IOU ? mask_kernel<VGHM_METRIC_IOU> : mask_kernel<VGHM_METRIC_IOS>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)words, (unsigned)words), dim3(WAVE), 0, st, (const float4*)sbox, (const int32_t*)stile, (const int32_t*)counters, words,
                           j.match_thr, mask);
    }
    if (q.ok())
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(WAVE), 0, st, (const uint64_t*)mask, (const int32_t*)counters, words, keptw, prefix, counters + 1);
    if (q.ok()) {
        const int lanes = n_pad > j.max_heads ? n_pad : j.max_heads;
        hipLaunchKernelGGL(emit_kernel, dim3((unsigned)(lanes + 255) / 256), dim3(256), 0, st, (const int32_t*)sidx, (const float4*)sbox, (const uint8_t*)st0,
                           (const uint64_t*)keptw, (const int32_t*)prefix, (const int32_t*)counters, j.scores_dev, N, n_pad, j.keep_k, j.max_heads, j.head_row_dev,
                           j.head_tile_dev, (float4*)j.boxes_full_dev, j.scores_out_dev, j.n_heads_dev, j.n_kept_uncapped_dev, j.status_dev);
    }
    return finish(q, s, true, st, "merge_tiles");
}
