// Post-network stages for gfx950: DFL/box/score decode, per-image top-k, candidate gather with FLAME
// parameter fix-up, greedy NMS, slab compaction.  All fp32; IoU arithmetic is IEEE (no contraction,
// true division) so keep/suppress decisions are bit-identical to the reference CPU path.
//
// Reference: yolo_head_training/yolo_head/yolo_head_ndfl_heads.py:143-172 (decode + fix-up),
// yolo_head_dfl_head.py:162-184 (activations, zero pad, channel order), yolo_heads.py:63-86 (top-k),
// head_detector/utils.py:159-194 + torchvision.ops.nms (conf filter, NMS, keep-100).
#include "per_device.h"
#include "vgh_internal.h"

namespace {

constexpr int MAX_LEVELS = 4;
struct Levels {
    const float* pred[MAX_LEVELS];
    int h[MAX_LEVELS], w[MAX_LEVELS], pitch[MAX_LEVELS], stride[MAX_LEVELS], start[MAX_LEVELS + 1];
    int n;
};

__device__ __forceinline__ int find_level(const Levels& L, int a) {
    int l = 0;
#pragma unroll
    for (int i = 1; i < MAX_LEVELS; ++i)
        if (i < L.n && a >= L.start[i]) l = i;
    return l;
}

// ---- K6: boxes + scores for every anchor --------------------------------------------------------
__global__ __launch_bounds__(256) void head_decode_kernel(Levels L, int B, int A, float* __restrict__ boxes, float* __restrict__ scores) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (int64_t)B * A) return;
    const int b = (int)(gid / A), a = (int)(gid - (int64_t)b * A);
    const int l = find_level(L, a);
    const int p = a - L.start[l];
    const int hw = L.h[l] * L.w[l];
    const float* pr = L.pred[l] + ((int64_t)b * hw + p) * L.pitch[l];
    const int ay = p / L.w[l], ax = p - ay * L.w[l];
    float d[4];
#pragma unroll
    for (int side = 0; side < 4; ++side) {
        float x[17];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < 17; ++k) {
            x[k] = pr[side * 17 + k];
            m = fmaxf(m, x[k]);
        }
        float s = 0.0f;
#pragma unroll
        for (int k = 0; k < 17; ++k) {
            x[k] = expf(x[k] - m);
            s += x[k];
        }
        float e = 0.0f;
#pragma unroll
        for (int k = 0; k < 17; ++k) e += (x[k] / s) * (float)k;  // softmax(dim=bins) * linspace(0..16), summed
        d[side] = e;
    }
    const float cx = (float)ax + 0.5f, cy = (float)ay + 0.5f, st = (float)L.stride[l];
    float4 o;
    o.x = (cx - d[0]) * st;  // batch_distance2bbox: x1y1 = p - lt, x2y2 = p + rb ; then * stride
    o.y = (cy - d[1]) * st;
    o.z = (cx + d[2]) * st;
    o.w = (cy + d[3]) * st;
    *(float4*)(boxes + gid * 4) = o;
    scores[gid] = 1.0f / (1.0f + expf(-pr[VGH_PRED_CLS_OFF]));
}

// ---- K7: per-image top-k via radix select on a 64-bit composite (score key, ~index) -------------
// The order of torch.sort(descending=True, stable=True), which is what the reference's top-k is held to: every NaN (either sign, any payload) ranks above +inf,
// -0.0 == +0.0, equal keys by ascending index.  Key 0 is taken by no score (-inf has 0x007fffff): topk_kernel<.., FILTER> gives it to the rows that fail the filter.
__device__ __forceinline__ uint32_t float_key(float f) {
    uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;  // NaN
    if (u == 0x80000000u) u = 0u;                             // -0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);        // order-preserving
}
template <bool FILTER>
__device__ __forceinline__ uint64_t composite(float f, int idx, float conf) {
    const uint32_t key = (FILTER && !(f >= conf)) ? 0u : float_key(f);
    return ((uint64_t)key << 32) | (uint32_t)(~(uint32_t)idx);
}

// r06 (profiles/r06_latency_trace_l1.txt: 47 us of a 2.0-ms single-image call): (i) RC composites per thread live in registers when the row fits (A <= RC * 1024: the
// 8 400 anchors of a 640 image; the 33 600 of a 1280 image re-read the scores as before), so the scores are read once instead of once per pass; (ii) the radix
// select STOPS at the first pass whose selected bin holds exactly the remaining count -- every element of that bin is then selected, the threshold is the bin's lower
// edge, and with distinct scores that is the 3rd or 4th of the 8 passes (the index bits only matter when the k-th score is tied).  Same selected set, same order.
// FILTER (vgh_topk_nms): a row that fails score >= conf ranks below every row that passes (key 0, ascending index among themselves), so it takes a candidate slot
// only when fewer than k rows pass -- and the NMS never visits it.  The selected set of passing rows is that of "filter, then top-k".
template <bool CACHED, bool FILTER>
__global__ __launch_bounds__(1024) void topk_kernel(const float* __restrict__ scores, int A, int k, int32_t* __restrict__ out_idx,
                                                    float* __restrict__ out_scores, float conf) {
    constexpr int RC = 9;
    __shared__ uint32_t hist[256];
    __shared__ uint64_t s_prefix;
    __shared__ int s_kk;
    __shared__ int s_count;
    __shared__ int s_done;
    __shared__ uint64_t sel[1024];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* sc = scores + (int64_t)b * A;
    if (tid == 0) {
        s_prefix = 0;
        s_kk = k;
        s_count = 0;
        s_done = 0;
    }
    sel[tid] = 0;
    uint64_t cache[RC];
    if constexpr (CACHED) {
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const int i = tid + r * 1024;
            cache[r] = i < A ? composite<FILTER>(sc[i], i, conf) : 0ull;  // 0 is below every real composite (its low word would be the index 0xffffffff)
        }
    }
    __syncthreads();
    // up to 8 passes x 8 bits, MSB first: after the last pass s_prefix == the k-th largest composite (or the lower edge of a bin that is selected as a whole)
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        const uint64_t prefix = s_prefix;
        if constexpr (CACHED) {
#pragma unroll
            for (int r = 0; r < RC; ++r) {
                const uint64_t c = cache[r];
                const bool match = c != 0ull && ((pass == 0) || ((c >> (shift + 8)) == (prefix >> (shift + 8))));
                if (match) atomicAdd(&hist[(c >> shift) & 255], 1u);
            }
        } else {
            for (int i = tid; i < A; i += 1024) {
                const uint64_t c = composite<FILTER>(sc[i], i, conf);
                const bool match = (pass == 0) || ((c >> (shift + 8)) == (prefix >> (shift + 8)));
                if (match) atomicAdd(&hist[(c >> shift) & 255], 1u);
            }
        }
        __syncthreads();
        const int kk = s_kk;
        __syncthreads();
        if (tid < 256) {
            uint32_t above = 0;
            for (int j = tid + 1; j < 256; ++j) above += hist[j];
            const uint32_t mine = hist[tid];
            if ((int)above < kk && kk <= (int)(above + mine)) {
                s_prefix = prefix | ((uint64_t)tid << shift);
                s_kk = kk - (int)above;
                if (kk == (int)(above + mine)) s_done = 1;  // the whole bin is selected: its lower edge is a valid threshold
            }
        }
        __syncthreads();
        if (s_done) break;  // (block-uniform: read after the barrier)
    }
    const uint64_t T = s_prefix;
    if constexpr (CACHED) {
#pragma unroll
        for (int r = 0; r < RC; ++r) {
            const uint64_t c = cache[r];
            if (c != 0ull && c >= T) {
                const int slot = atomicAdd(&s_count, 1);
                if (slot < 1024) sel[slot] = c;
            }
        }
    } else {
        for (int i = tid; i < A; i += 1024) {
            const uint64_t c = composite<FILTER>(sc[i], i, conf);
            if (c >= T) {
                const int slot = atomicAdd(&s_count, 1);
                if (slot < 1024) sel[slot] = c;
            }
        }
    }
    __syncthreads();
    // bitonic sort, descending, 1024 entries (zeros = padding sink to the end).  r06: every thread keeps ITS entry in registers; the 45 compare-exchange steps whose
    // partner sits in the same wave (stride < 64) are cross-lane shuffles with no barrier, only the 10 steps with stride >= 64 go through LDS (20 barriers instead
    // of 55: the sort was ~15 us of a 34-us launch whose single block per image has nothing else to hide behind).  Same network, same comparisons, same result.
    uint64_t v = sel[tid];
    for (int size = 2; size <= 1024; size <<= 1) {
        const bool desc = (tid & size) == 0;
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            uint64_t pv;
            if (stride >= 64) {
                __syncthreads();  // (everybody has read its partner of the previous LDS step)
                sel[tid] = v;
                __syncthreads();
                pv = sel[tid ^ stride];
            } else {
                pv = __shfl_xor(v, stride, 64);
            }
            const bool take_max = ((tid & stride) == 0) == desc;  // the lower index of a pair keeps the larger entry in a descending run
            v = take_max ? (v > pv ? v : pv) : (v < pv ? v : pv);
        }
    }
    if (tid < k) {
        const int idx = (int)(~(uint32_t)(v & 0xffffffffu));
        out_idx[(int64_t)b * k + tid] = idx;
        if (out_scores) out_scores[(int64_t)b * k + tid] = sc[idx];
    }
}

// ---- K6b: gather boxes + FLAME 413-vector for selected anchors ----------------------------------
// channel c of the reference's 413-vector for the anchor whose prediction row has the FLAME segment `pf` (channel VGH_PRED_FLAME_OFF and up of the row) (yolo_head_dfl_head.py:162-184, yolo_head_ndfl_heads.py:143-172): tanh * 3 on the
// live shape / expression channels (zeros behind them), the rotation / jaw permutation, translation += anchor centre * stride, exp(scale) / 0.05 * stride
__device__ __forceinline__ float flame_channel(const float* __restrict__ pr, int c, int S, int E, int ax, int ay, float st) {
    const int o_shape = 0, o_expr = o_shape + S, o_rot = o_expr + E, o_jaw = o_rot + 6, o_tr = o_jaw + 3, o_sc = o_tr + 3;
    float v = 0.0f;
    if (c < 300) {
        if (c < S) v = tanhf(pr[o_shape + c]) * 3.0f;
    } else if (c < 400) {
        if (c - 300 < E) v = tanhf(pr[o_expr + c - 300]) * 3.0f;
    } else if (c < 403) {
        v = pr[o_rot + 3 + (c - 400)];  // T[400:403] = O[403:406] = rot branch [3:6]
    } else if (c < 406) {
        v = pr[o_jaw + (c - 403)];  // T[403:406] = O[406:409] = jaw branch
    } else if (c < 409) {
        v = pr[o_rot + (c - 406)];  // T[406:409] = O[400:403] = rot branch [0:3]
    } else if (c == 409) {
        v = pr[o_tr + 0] + ((float)ax + 0.5f) * st;  // translation[:, 0:2] += anchor * stride
    } else if (c == 410) {
        v = pr[o_tr + 1] + ((float)ay + 0.5f) * st;
    } else if (c == 411) {
        v = pr[o_tr + 2];
    } else {
        v = (expf(pr[o_sc]) / 0.05f) * st;  // exp(x)/0.05, then scale *= stride
    }
    return v;
}

// (r06: four candidate rows per 256-thread block, one wave each -- 16 000 blocks per 64 images instead of 64 000 one-wave blocks)
__global__ __launch_bounds__(256) void gather_kernel(Levels L, int A, int S, int E, const float* __restrict__ boxes, const int32_t* __restrict__ idx,
                                                     int k, float* __restrict__ out_boxes, float* __restrict__ out_flame) {
    const int j = blockIdx.x * 4 + (threadIdx.x >> 6), b = blockIdx.y, lane = threadIdx.x & 63;
    if (j >= k) return;
    const int a = idx[(int64_t)b * k + j];
    const int l = find_level(L, a);
    const int p = a - L.start[l];
    const int hw = L.h[l] * L.w[l];
    const float* pr = L.pred[l] + ((int64_t)b * hw + p) * L.pitch[l];
    const int ay = p / L.w[l], ax = p - ay * L.w[l];
    const float st = (float)L.stride[l];
    if (lane < 4) out_boxes[((int64_t)b * k + j) * 4 + lane] = boxes[((int64_t)b * A + a) * 4 + lane];
    if (!out_flame) return;  // lazy mode (vgh_detector_set_lazy_flame): the 413-vector is built for the SURVIVORS only, inside nms_select_kernel
    float* of = out_flame + ((int64_t)b * k + j) * VGH_NUM_FLAME_PARAMS;
    for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) of[c] = flame_channel(pr + VGH_PRED_FLAME_OFF, c, S, E, ax, ay, st);
}

// ---- K8: conf filter + greedy NMS + keep-k -------------------------------------------------------
__device__ __forceinline__ bool iou_gt(const float4 a, const float area_a, const float4 b, const float thr) {
#pragma clang fp contract(off)
    const float area_b = (b.z - b.x) * (b.w - b.y);
    const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y);
    const float xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
    const float w = fmaxf(0.0f, xx2 - xx1), h = fmaxf(0.0f, yy2 - yy1);
    const float inter = w * h;
    const float ovr = inter / (area_a + area_b - inter);
    return ovr > thr;
}

// The greedy loop of nms_kernel and nms_select_kernel: one 1024-thread block per image, thread t owns candidate row t; `boxes` / `scores` / `keep_row` are the image's.
// Every row that fails score >= conf (utils.py:174), and every position behind n_in, is marked in `removed` BEFORE the first round: such a row is never visited,
// never kept and never suppresses anything, wherever it stands.  With scores sorted descending the rows that pass are a prefix -- except for NaN scores, which head
// vgh_topk's order and fail every filter.  The remaining rows are visited in position order, torchvision's loop.  Writes keep_row[0 .. keep_k) (positions, -1 behind
// the count) and, where s_keep is given, the kept positions to LDS as well; returns the count (block-uniform).
__device__ __forceinline__ int greedy_nms(const float* __restrict__ boxes, const float* __restrict__ scores, int n_in, float conf, float thr, int keep_k,
                                          int32_t* __restrict__ keep_row, float4* sb, unsigned long long* removed, int* s_keep) {
    const int tid = threadIdx.x;
    bool valid = false;
    if (tid < n_in) {
        sb[tid] = *(const float4*)(boxes + (int64_t)tid * 4);
        valid = scores[tid] >= conf;
    }
    const unsigned long long bal = __ballot(valid);
    if ((tid & 63) == 0) removed[tid >> 6] = ~bal;
    for (int j = tid; j < keep_k; j += 1024) keep_row[j] = -1;
    __syncthreads();
    int kept = 0;
    int i = 0;
    while (kept < keep_k) {
        // next candidate not yet suppressed (uniform: every thread scans the same LDS words)
        int nxt = -1;
        for (int wd = i >> 6; wd < 16 && nxt < 0; ++wd) {
            unsigned long long free_bits = ~removed[wd];
            if (wd == (i >> 6)) free_bits &= ~0ull << (i & 63);
            if (free_bits) nxt = wd * 64 + __ffsll((long long)free_bits) - 1;
        }
        if (nxt < 0) break;
        i = nxt;
        if (tid == 0) {
            keep_row[kept] = i;
            if (s_keep) s_keep[kept] = i;
        }
        ++kept;
        const float4 bi = sb[i];
        float area_i;
        {
#pragma clang fp contract(off)
            area_i = (bi.z - bi.x) * (bi.w - bi.y);
        }
        const bool sup = (tid > i) && valid && iou_gt(bi, area_i, sb[valid ? tid : 0], thr);
        const unsigned long long m = __ballot(sup);
        __syncthreads();  // everyone has finished scanning `removed` for this round
        if ((tid & 63) == 0 && m) removed[tid >> 6] |= m;
        __syncthreads();
        ++i;
    }
    return kept;
}

__global__ __launch_bounds__(1024) void nms_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, int n_in, float conf, float thr,
                                                   int keep_k, int32_t* __restrict__ keep_idx, int32_t* __restrict__ counts) {
    __shared__ float4 sb[1024];
    __shared__ unsigned long long removed[16];
    const int b = blockIdx.x;
    const int kept = greedy_nms(boxes + (int64_t)b * n_in * 4, scores + (int64_t)b * n_in, n_in, conf, thr, keep_k, keep_idx + (int64_t)b * keep_k, sb, removed, nullptr);
    if (threadIdx.x == 0) counts[b] = kept;
}

// r06 (single-image latency: profiles/r06_latency_trace_l1.txt shows nms -> compact -> head_list as three 5.7-us launches, each waiting for the one before): the three
// as ONE launch.  Block b = image b: nms_kernel's greedy loop (greedy_nms; kept positions also kept in LDS), then its 16 waves copy the image's keep_k survivor rows
// (compact_kernel's copy, zeros behind the count); the block that finishes LAST (a ticket in device memory, reset for the next launch) builds the image-major head list
// from counts[B] (head_list_kernel's scan).  Same decisions, same bytes: tests compare it with the staged entry points.
__global__ __launch_bounds__(1024) void nms_select_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const float* __restrict__ flame, int n_in,
                                                          float conf, float thr, int keep_k, int32_t* __restrict__ keep_idx, int32_t* __restrict__ counts,
                                                          float* __restrict__ ob, float* __restrict__ os, float* __restrict__ of, int B, int capacity,
                                                          int32_t* __restrict__ head_row, int32_t* __restrict__ head_image, int32_t* __restrict__ n_heads,
                                                          int32_t* __restrict__ ticket, Levels L, const int32_t* __restrict__ lazy_idx, int S, int E, int rows_later) {
    __shared__ float4 sb[1024];
    __shared__ unsigned long long removed[16];
    __shared__ int s_keep[1024];
    __shared__ int s_off[1025];
    __shared__ int s_last;
    const int b = blockIdx.x, tid = threadIdx.x;
    const int kept = greedy_nms(boxes + (int64_t)b * n_in * 4, scores + (int64_t)b * n_in, n_in, conf, thr, keep_k, keep_idx + (int64_t)b * keep_k, sb, removed, s_keep);
    if (tid == 0) counts[b] = kept;
    __syncthreads();  // s_keep is complete
    // ---- the image's survivor rows ----
    const int w = tid >> 6, lane = tid & 63;
    for (int j = w; j < keep_k; j += 16) {
        const int64_t o = (int64_t)b * keep_k + j;
        if (j >= kept) {
            if (lane < 4) ob[o * 4 + lane] = 0.0f;
            if (lane == 0) os[o] = 0.0f;
            if (of)
                for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) of[o * VGH_NUM_FLAME_PARAMS + c] = 0.0f;
            continue;
        }
        const int64_t sr = (int64_t)b * n_in + s_keep[j];
        if (lane < 4) ob[o * 4 + lane] = boxes[sr * 4 + lane];
        if (lane == 0) os[o] = scores[sr];
        if (of && !rows_later) {  // (rows_later: survivor_rows_kernel, queued behind this launch, writes the survivors' vectors)
            if (lazy_idx) {  // lazy mode: the candidate tensor was never filled; the survivor's vector straight from its prediction row (gather_kernel's arithmetic)
                const int a = lazy_idx[sr];
                const int l = find_level(L, a);
                const int p = a - L.start[l];
                const float* pr = L.pred[l] + ((int64_t)b * (L.h[l] * L.w[l]) + p) * L.pitch[l];
                const int ay = p / L.w[l], ax = p - ay * L.w[l];
                const float st = (float)L.stride[l];
                for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) of[o * VGH_NUM_FLAME_PARAMS + c] = flame_channel(pr + VGH_PRED_FLAME_OFF, c, S, E, ax, ay, st);
            } else {
                for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) of[o * VGH_NUM_FLAME_PARAMS + c] = flame[sr * VGH_NUM_FLAME_PARAMS + c];
            }
        }
    }
    if (!head_row) return;
    // ---- the head list, by the block that finishes last ----
    __threadfence();  // this block's counts[b] is visible before its ticket
    __syncthreads();
    if (tid == 0) s_last = (atomicAdd(ticket, 1) == B - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    if (tid == 0) *ticket = 0;  // (every other block has taken its ticket: nobody touches it again in this launch)
    __threadfence();
    const int per = (B + 1023) / 1024;
    const int b0 = tid * per, b1 = min(B, b0 + per);
    int mine = 0;
    for (int q = b0; q < b1; ++q) mine += min(max(__hip_atomic_load(counts + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0), keep_k);
    s_off[tid] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = (tid >= d) ? s_off[tid - d] : 0;
        __syncthreads();
        s_off[tid] += v;
        __syncthreads();
    }
    int at = s_off[tid] - mine;
    if (tid == 1023) *n_heads = min(s_off[1023], capacity);
    for (int q = b0; q < b1; ++q) {
        const int c = min(max(__hip_atomic_load(counts + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), 0), keep_k);
        for (int e = 0; e < c; ++e) {
            if (at + e < capacity) {
                head_row[at + e] = q * keep_k + e;
                head_image[at + e] = q;
            }
        }
        at += c;
    }
}

__global__ __launch_bounds__(64) void compact_kernel(const float* __restrict__ boxes, const float* __restrict__ scores, const float* __restrict__ flame,
                                                     int n_in, const int32_t* __restrict__ keep_idx, int keep_k, float* __restrict__ ob,
                                                     float* __restrict__ os, float* __restrict__ of) {
    const int j = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int src = keep_idx[(int64_t)b * keep_k + j];
    const int64_t o = (int64_t)b * keep_k + j;
    if (src < 0) {
        if (lane < 4) ob[o * 4 + lane] = 0.0f;
        if (lane == 0) os[o] = 0.0f;
        if (of)
            for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) of[o * VGH_NUM_FLAME_PARAMS + c] = 0.0f;
        return;
    }
    const int64_t s = (int64_t)b * n_in + src;
    if (lane < 4) ob[o * 4 + lane] = boxes[s * 4 + lane];
    if (lane == 0) os[o] = scores[s];
    if (of)
        for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) of[o * VGH_NUM_FLAME_PARAMS + c] = flame[s * VGH_NUM_FLAME_PARAMS + c];
}

// rows of boxes [B,n,4] picked by idx [B,k] -> sorted boxes [B,k,4]
__global__ __launch_bounds__(256) void gather_boxes_kernel(const float* __restrict__ boxes, const int32_t* __restrict__ idx, int n, int k, float* __restrict__ out) {
    const int j = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (j >= k) return;
    const int src = idx[(int64_t)b * k + j];
    const f32x4_t v = *(const f32x4_t*)(boxes + ((int64_t)b * n + src) * 4);
    *(f32x4_t*)(out + ((int64_t)b * k + j) * 4) = v;
}

// survivors of the NMS (positions into the top-k order) -> rows of the ORIGINAL tensors: src = idx[b][keep[b][j]]
__global__ __launch_bounds__(64) void compact_indirect_kernel(const float* __restrict__ boxes, const float* __restrict__ flame, int flame_w, int n,
                                                              const int32_t* __restrict__ idx, const float* __restrict__ sorted_scores, int k,
                                                              const int32_t* __restrict__ keep_idx, int keep_k, float* __restrict__ ob, float* __restrict__ os,
                                                              float* __restrict__ of) {
    const int j = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    const int pos = keep_idx[(int64_t)b * keep_k + j];
    const int64_t o = (int64_t)b * keep_k + j;
    if (pos < 0) {
        if (lane < 4) ob[o * 4 + lane] = 0.0f;
        if (lane == 0) os[o] = 0.0f;
        if (of)
            for (int c = lane; c < flame_w; c += 64) of[o * flame_w + c] = 0.0f;
        return;
    }
    const int64_t s = (int64_t)b * n + idx[(int64_t)b * k + pos];
    if (lane < 4) ob[o * 4 + lane] = boxes[s * 4 + lane];
    if (lane == 0) os[o] = sorted_scores[(int64_t)b * k + pos];
    if (of)
        for (int c = lane; c < flame_w; c += 64) of[o * flame_w + c] = flame[s * flame_w + c];
}

// ---- the FLAME prediction rows of the NMS survivors, computed on demand ----------------------------
// The last layer of the FLAME towers is a set of 1x1 convs with fp32 output (heads.head*.flame_*_pred.3): pointwise, so the rows the select needs -- a handful per
// image out of 8 400 -- can be computed alone from the survivors' rows of the towers' last bf16 tensors, and a forward that defers those convs (vgh_net_set_defer)
// never writes or reads the dense rows.  Bit for bit what the implicit-GEMM tiles (conv_kernels.inc, conv_igemm_kernel) write: the same 32x32x16 bf16 MFMA with the
// weights as A (32 couts) and the pixels as B (here: 32 survivors, missing ones as zero columns that are thrown away), accumulators from zero, the 32-channel
// k-blocks in ascending order and the two 16-channel halves of each in order, the bias added in fp32 afterwards, the activation as one max against act_bound.  An
// output element of the MFMA depends on its own weight row and pixel column only, so where the pixel stands in the tile does not matter; nor does the tile of the
// table (they differ in how many k-blocks a stage holds and in who stores what, not in this chain).
struct RowOps {
    Levels L;
    vgh_row_op op[MAX_LEVELS][kMaxRowOps];
    int n[MAX_LEVELS];
};
constexpr int ROW_W = 416;  // floats per staged row: 300 + 100 + 13 FLAME channels at most, rounded up to 16 bytes

// grid (ceil(keep_k / 32), B), 256 threads: block (g, b) takes survivors [32 g, 32 g + 32) of image b and leaves at once when the image has fewer.  Lane & 31 = the
// survivor (in every wave), the four waves share the (op, 32-cout tile) units of a level; the rows meet in LDS, then wave w writes survivors w, w + 4, ...
__global__ __launch_bounds__(256) void survivor_rows_kernel(const RowOps R, int n_in, int keep_k, const int32_t* __restrict__ idx, const int32_t* __restrict__ keep_idx,
                                                            const int32_t* __restrict__ counts, int S, int E, float* __restrict__ out) {
    __shared__ float rows[32][ROW_W];
    const int b = blockIdx.y, j0 = blockIdx.x * 32, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int kept = min(max(counts[b], 0), keep_k);
    if (j0 >= kept) return;  // (block-uniform)
    for (int i = tid; i < 32 * ROW_W; i += 256) (&rows[0][0])[i] = 0.0f;
    const Levels& L = R.L;
    const int A = L.start[L.n];
    const int px = lane & 31, hi = lane >> 5;
    const bool valid = j0 + px < kept;
    int lvl = -1, p = 0;
    if (valid) {
        const int pos = min(max(keep_idx[(int64_t)b * keep_k + j0 + px], 0), n_in - 1);
        const int a = min(max(idx[(int64_t)b * n_in + pos], 0), A - 1);
        lvl = find_level(L, a);
        p = a - L.start[lvl];
    }
    __syncthreads();
    for (int l = 0; l < L.n; ++l) {
        const bool mine = lvl == l;
        if (!__any(mine)) continue;  // (the same in every wave: each holds all 32 survivors)
        const int hw = L.h[l] * L.w[l];
        int units = 0;
        for (int k = 0; k < R.n[l]; ++k) units += R.op[l][k].cout_pad >> 5;
        for (int u = w; u < units; u += 4) {  // (wave-uniform)
            int k = 0, t = u;
            while (t >= (R.op[l][k].cout_pad >> 5)) t -= R.op[l][k++].cout_pad >> 5;
            const vgh_row_op& o = R.op[l][k];
            const int co = t * 32 + px;  // this lane's weight row of the A fragments
            const uint16_t* const xr = o.in + ((int64_t)b * hw + p) * o.in_pitch + o.in_coff + hi * 8;
            const uint16_t* const wr = o.wpack + (int64_t)co * 32;
            const int sw = (co >> 2) & 3;  // the packed image stores logical 16-byte chunk c of a row in slot c ^ ((row >> 2) & 3)
            f32x16_t acc;
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
            for (int kb = 0; kb < o.cblocks; ++kb) {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bf16x8_t af = *(const bf16x8_t*)(wr + (int64_t)kb * o.cout_pad * 32 + ((2 * h + hi) ^ sw) * 8);
                    bf16x8_t bf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) bf[e] = (__bf16)0.0f;
                    if (mine) bf = *(const bf16x8_t*)(xr + kb * 32 + h * 16);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
                }
            }
            const float act_lo = o.act == VGH_ACT_RELU ? 0.0f : __builtin_nanf("");  // (conv_kernels.inc, act_bound)
            const int oc = o.out_coff - VGH_PRED_FLAME_OFF;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = t * 32 + q * 8 + hi * 4 + e;  // accumulator register 4 q + e of lane (pixel px, half hi)
                    if (mine && c < o.cout_store) rows[px][oc + c] = fmaxf(acc[q * 4 + e] + o.bias[c], act_lo);
                }
        }
    }
    __syncthreads();
    for (int r = w; r < 32 && j0 + r < kept; r += 4) {
        const int pos = min(max(keep_idx[(int64_t)b * keep_k + j0 + r], 0), n_in - 1);
        const int a = min(max(idx[(int64_t)b * n_in + pos], 0), A - 1);
        const int l = find_level(L, a);
        const int pp = a - L.start[l];
        const int ay = pp / L.w[l], ax = pp - ay * L.w[l];
        const float st = (float)L.stride[l];
        const int64_t o = (int64_t)b * keep_k + j0 + r;
        for (int c = lane; c < VGH_NUM_FLAME_PARAMS; c += 64) out[o * VGH_NUM_FLAME_PARAMS + c] = flame_channel(rows[r], c, S, E, ax, ay, st);
    }
}

// ---- ... and from the ROOT of the FLAME towers, where the forward skipped the 3x3 towers in front of those convs as well (tower_plan.h) -------------------------
// A survivor's prediction row depends on the (2 depth + 1)^2 window of the towers' root tensor around its anchor only.  One workgroup per survivor stages that
// window in LDS (positions outside the map as zeros) and walks the level's tree: layer t turns tensor t - 1 into tensor t, one ring smaller, as bf16 in LDS -- and a
// position of tensor t that lies outside the map is stored as ZERO, not as the value computed from padding: it is the next layer's zero padding.  The prediction
// 1x1 convs then read the single pixel left, as survivor_rows_kernel does.
// Bit for bit what the dense ops write.  Every 3x3 tile of the table issues the same v_mfma_f32_32x32x16_bf16 per (tap, 32-channel block, 16-channel half) with the
// same eight channels per lane half; an output element depends on its weight row and pixel column only, so which pixels share an MFMA does not matter.  What does
// differ between families is the ORDER of the (tap, channel block) pairs and where the bias enters (conv_tiles.h, kChainTrait): the op carries the code of the tile
// the dense launch would have run on (vgh_tree_op::chain), resolved by the launcher's own rule for the pending forward.  Padding taps contribute exact zeros in both.
// Cost: ~37 M MACs and ~4 MB of weights out of L2 per survivor on the L net; sized for a few hundred survivors per forward (one workgroup each, all resident at
// once).  At capacity (B x keep_k survivors) the workgroups run in rounds of one per CU: the dense towers are cheaper there (vgh_detector_set_lazy_flame(d, 2)).
struct TowerArgs {
    Levels L;
    vgh_tower_tree t[MAX_LEVELS];
    int off[MAX_LEVELS][5];  // vgh_tower_lds
};
static_assert(sizeof(TowerArgs) <= 4000, "kernel arguments: 4 KB");

// grid (keep_k, B), 512 threads: block (j, b) takes survivor j of image b and leaves at once when the image has fewer.  Lane & 31 = the pixel of the layer's output
// window (in every wave), the eight waves share the (op, 32-cout tile, 32-pixel group) units of a layer.  Every barrier is reached by the whole block: the loop
// bounds depend on the survivor's level alone.
__global__ __launch_bounds__(512) void survivor_towers_kernel(const TowerArgs T, int n_in, int keep_k, const int32_t* __restrict__ idx, const int32_t* __restrict__ keep_idx,
                                                              const int32_t* __restrict__ counts, int S, int E, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char tw_smem[];
    const int b = blockIdx.y, j = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kept = min(max(counts[b], 0), keep_k);
    if (j >= kept) return;  // (block-uniform)
    const Levels& L = T.L;
    const int A = L.start[L.n];
    const int pos = min(max(keep_idx[(int64_t)b * keep_k + j], 0), n_in - 1);
    const int a = min(max(idx[(int64_t)b * n_in + pos], 0), A - 1);
    const int l = __builtin_amdgcn_readfirstlane(find_level(L, a));
    const int p = a - L.start[l];
    const int H = L.h[l], W = L.w[l];
    const int ay = p / W, ax = p - ay * W;
    const vgh_tower_tree& t = T.t[l];
    const int D = t.depth;
    float* const row = (float*)(tw_smem + T.off[l][D + 1]);
    {  // the root window, [2 D + 1]^2 pixels x root_c channels, 16 bytes at a time; the prediction row starts as zeros
        const int side = 2 * D + 1, cpp = t.root_c >> 3, pitch = t.chan[0] + 8;
        const uint16_t* const src = t.root + (int64_t)b * H * W * t.root_pitch + t.root_c0;
        for (int i = tid; i < side * side * cpp; i += 512) {
            const int px = i / cpp, ch = i - px * cpp;
            const int wy = px / side, wx = px - wy * side;
            const int iy = ay - D + wy, ix = ax - D + wx;
            bf16x8_t v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (__bf16)0.0f;
            if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = *(const bf16x8_t*)(src + ((int64_t)iy * W + ix) * t.root_pitch + ch * 8);
            *(bf16x8_t*)(tw_smem + T.off[l][0] + ((int64_t)px * pitch + ch * 8) * 2) = v;
        }
        for (int i = tid; i < ROW_W; i += 512) row[i] = 0.0f;
    }
    __syncthreads();
    const int n32 = lane & 31, hi = lane >> 5;
    for (int lay = 1; lay <= D + 1; ++lay) {
        const bool conv3 = lay <= D;
        const int so = conv3 ? 2 * (D - lay) + 1 : 1, si = conv3 ? so + 2 : 1, npix = so * so, ngrp = (npix + 31) >> 5, taps = conv3 ? 9 : 1;
        const int pin = t.chan[lay - 1] + 8;
        const char* const xin = tw_smem + T.off[l][lay - 1];
        int units = 0;
        for (int k = 0; k < t.n_ops; ++k)
            if (t.op[k].layer == lay) units += (t.op[k].cout_pad >> 5) * ngrp;
        for (int u = w; u < units; u += 8) {  // (wave-uniform)
            int k = 0, r = u;
            while (true) {
                const int n = t.op[k].layer == lay ? (t.op[k].cout_pad >> 5) * ngrp : 0;
                if (r < n) break;
                r -= n;
                ++k;
            }
            const vgh_tree_op& o = t.op[k];
            const int ct = r / ngrp, g = r - ct * ngrp;
            const int px = g * 32 + n32;
            const bool valid = px < npix;
            const int oy = valid ? px / so : 0, ox = valid ? px - oy * so : 0;
            const int co = ct * 32 + n32;  // this lane's weight row of the A fragments
            const int in_coff = o.in_coff + (o.grp_cout ? (ct * 32 / o.grp_cout) * o.grp_in_stride : 0);
            const uint16_t* const wr = o.wpack + (int64_t)co * 32;
            const int sw = (co >> 2) & 3;  // the packed image stores logical 16-byte chunk c of a row in slot c ^ ((row >> 2) & 3)
            const bool tap_major = (o.chain & 1) || !conv3, bias_first = (o.chain & 2) && conv3;
            f32x16_t acc;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[q * 4 + e] = bias_first ? o.bias[ct * 32 + q * 8 + hi * 4 + e] : 0.0f;  // accumulator register 4 q + e of lane (pixel, half hi)
            const int nk = taps * o.cblocks;
            for (int s = 0; s < nk; ++s) {
                int tap, cb;
                if (tap_major) {
                    tap = s / o.cblocks;
                    cb = s - tap * o.cblocks;
                } else {
                    cb = s / 9;
                    tap = s - cb * 9;
                }
                const int ky = tap / 3, kx = tap - ky * 3;
                const char* const xr = xin + ((int64_t)((oy + ky) * si + ox + kx) * pin + in_coff + cb * 32 + hi * 8) * 2;
                const uint16_t* const wk = wr + (int64_t)(tap * o.cblocks + cb) * o.cout_pad * 32;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bf16x8_t af = *(const bf16x8_t*)(wk + ((2 * h + hi) ^ sw) * 8);
                    bf16x8_t bf;
#pragma unroll
                    for (int e = 0; e < 8; ++e) bf[e] = (__bf16)0.0f;
                    if (valid) bf = *(const bf16x8_t*)(xr + h * 32);
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf, acc, 0, 0, 0);
                }
            }
            const float act_lo = o.act == VGH_ACT_RELU ? 0.0f : __builtin_nanf("");  // (conv_kernels.inc, act_bound)
            if (conv3) {
                const int my = ay - (D - lay) + oy, mx = ax - (D - lay) + ox;
                const bool inside = (unsigned)my < (unsigned)H && (unsigned)mx < (unsigned)W;
                char* const xo = tw_smem + T.off[l][lay] + ((int64_t)px * (t.chan[lay] + 8) + o.out_coff) * 2;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = ct * 32 + q * 8 + hi * 4;
                    bf16x4_t v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (__bf16)(inside ? fmaxf(bias_first ? acc[q * 4 + e] : acc[q * 4 + e] + o.bias[c + e], act_lo) : 0.0f);
                    if (valid && c < o.cout_store) *(bf16x4_t*)(xo + c * 2) = v;  // (cout_store is a multiple of 4: vgh_conv_prepare)
                }
            } else {
                const int oc = o.out_coff - VGH_PRED_FLAME_OFF;
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int c = ct * 32 + q * 8 + hi * 4 + e;
                        if (n32 == 0 && c < o.cout_store) row[oc + c] = fmaxf(acc[q * 4 + e] + o.bias[c], act_lo);
                    }
            }
        }
        __syncthreads();
    }
    const float st = (float)L.stride[l];
    const int64_t orow = (int64_t)b * keep_k + j;
    for (int c = tid; c < VGH_NUM_FLAME_PARAMS; c += 512) out[orow * VGH_NUM_FLAME_PARAMS + c] = flame_channel(row, c, S, E, ax, ay, st);
}

int make_levels(const vgh_head_level* levels, int n_levels, Levels* L) {
    VGH_REQUIRE(n_levels >= 1 && n_levels <= MAX_LEVELS, "head: n_levels=%d out of range", n_levels);
    L->n = n_levels;
    L->start[0] = 0;
    for (int i = 0; i < MAX_LEVELS; ++i) {
        if (i < n_levels) {
            L->pred[i] = levels[i].pred_dev;
            L->h[i] = levels[i].h;
            L->w[i] = levels[i].w;
            L->pitch[i] = levels[i].pitch;
            L->stride[i] = levels[i].stride;
            L->start[i + 1] = L->start[i] + levels[i].h * levels[i].w;
        } else {
            L->pred[i] = nullptr;
            L->h[i] = L->w[i] = L->pitch[i] = L->stride[i] = 0;
            L->start[i + 1] = L->start[i];
        }
    }
    return VGH_OK;
}

// vgh_topk (FILTER = false) and the candidate stage of vgh_topk_nms (FILTER = true: rows that fail score >= conf rank behind all others)
template <bool FILTER>
int topk_launch(const float* scores_dev, int B, int A, int k, int32_t* idx_dev, float* topk_scores_dev, float conf, void* stream) {
    VGH_REQUIRE(k >= 1 && k <= 1024, "topk: k=%d must be in [1,1024]", k);
    VGH_REQUIRE(k <= A, "topk: k=%d exceeds the number of anchors %d (torch.topk raises too)", k, A);
    if (B == 0) return VGH_OK;
    if (A <= 9 * 1024)
        hipLaunchKernelGGL((topk_kernel<true, FILTER>), dim3(B), dim3(1024), 0, (hipStream_t)stream, scores_dev, A, k, idx_dev, topk_scores_dev, conf);
    else
        hipLaunchKernelGGL((topk_kernel<false, FILTER>), dim3(B), dim3(1024), 0, (hipStream_t)stream, scores_dev, A, k, idx_dev, topk_scores_dev, conf);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

}  // namespace

extern "C" {

int vgh_head_decode(const vgh_head_level* levels, int n_levels, int B, float* boxes_dev, float* scores_dev, void* stream) {
    Levels L;
    if (int rc = make_levels(levels, n_levels, &L)) return rc;
    const int A = L.start[n_levels];
    if (B * (int64_t)A == 0) return VGH_OK;
    for (int i = 0; i < n_levels; ++i) VGH_REQUIRE(levels[i].pitch >= 69, "head_decode: pitch too small");
    const int64_t total = (int64_t)B * A;
    hipLaunchKernelGGL(head_decode_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, L, B, A, boxes_dev, scores_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

int vgh_topk(const float* scores_dev, int B, int A, int k, int32_t* idx_dev, float* topk_scores_dev, void* stream) {
    return topk_launch<false>(scores_dev, B, A, k, idx_dev, topk_scores_dev, 0.0f, stream);
}

int vgh_gather_candidates(const vgh_head_level* levels, int n_levels, int B, int A, int shape_c, int expr_c, const float* boxes_dev,
                          const int32_t* idx_dev, int k, float* out_boxes_dev, float* out_flame_dev, void* stream) {
    Levels L;
    if (int rc = make_levels(levels, n_levels, &L)) return rc;
    VGH_REQUIRE(A == L.start[n_levels], "gather: A=%d does not match the levels (%d)", A, L.start[n_levels]);
    VGH_REQUIRE(shape_c >= 0 && shape_c <= 300 && expr_c >= 0 && expr_c <= 100, "gather: bad live channel counts");
    for (int i = 0; i < n_levels; ++i) VGH_REQUIRE(levels[i].pitch >= VGH_PRED_FLAME_OFF + shape_c + expr_c + 13, "gather: pitch too small");
    if (B == 0 || k == 0) return VGH_OK;
    hipLaunchKernelGGL(gather_kernel, dim3((k + 3) / 4, B), dim3(256), 0, (hipStream_t)stream, L, A, shape_c, expr_c, boxes_dev, idx_dev, k, out_boxes_dev,
                       out_flame_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

int vgh_nms(const float* boxes_dev, const float* scores_dev, int B, int n_in, float conf_thr, float iou_thr, int keep_k, int32_t* keep_idx_dev,
            int32_t* counts_dev, void* stream) {
    VGH_REQUIRE(n_in >= 0 && n_in <= 1024, "nms: n_in=%d must be <= 1024", n_in);
    VGH_REQUIRE(keep_k >= 1, "nms: keep_k must be positive");
    if (B == 0) return VGH_OK;
    hipLaunchKernelGGL(nms_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, boxes_dev, scores_dev, n_in, conf_thr, iou_thr, keep_k, keep_idx_dev,
                       counts_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

}  // extern "C"
// (internal, C++ linkage: declared in vgh_internal.h)
int vgh_nms_select(const float* boxes_dev, const float* scores_dev, const float* flame_dev, int B, int n_in, float conf_thr, float iou_thr, int keep_k,
                   int32_t* keep_idx_dev, int32_t* counts_dev, float* out_boxes_dev, float* out_scores_dev, float* out_flame_dev, int capacity, int32_t* head_row_dev,
                   int32_t* head_image_dev, int32_t* n_heads_dev, int32_t* ticket_dev, const vgh_head_level* lazy_levels, int n_levels, const int32_t* lazy_idx_dev,
                   int shape_c, int expr_c, void* stream, int rows_later) {
    VGH_REQUIRE(n_in >= 0 && n_in <= 1024 && keep_k >= 1 && keep_k <= 1024, "nms_select: n_in=%d / keep_k=%d must be <= 1024", n_in, keep_k);
    VGH_REQUIRE(!head_row_dev || (head_image_dev && n_heads_dev && ticket_dev), "nms_select: the head list needs head_image, n_heads and the ticket");
    if (B == 0) return VGH_OK;
    Levels L;
    memset(&L, 0, sizeof(L));
    if (lazy_idx_dev) {
        VGH_REQUIRE(lazy_levels, "nms_select: the lazy FLAME gather needs the head levels");
        if (int rc = make_levels(lazy_levels, n_levels, &L)) return rc;
    }
    hipLaunchKernelGGL(nms_select_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, boxes_dev, scores_dev, flame_dev, n_in, conf_thr, iou_thr, keep_k, keep_idx_dev,
                       counts_dev, out_boxes_dev, out_scores_dev, out_flame_dev, B, capacity, head_row_dev, head_image_dev, n_heads_dev, ticket_dev, L, lazy_idx_dev, shape_c,
                       expr_c, rows_later);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

int vgh_survivor_rows(const vgh_head_level* levels, int n_levels, const vgh_row_op* ops, const int* n_ops, int B, int n_in, int keep_k, const int32_t* idx_dev,
                      const int32_t* keep_idx_dev, const int32_t* counts_dev, int shape_c, int expr_c, float* out_dev, void* stream) {
    VGH_REQUIRE(levels && ops && n_ops && idx_dev && keep_idx_dev && counts_dev && out_dev, "survivor_rows: null argument");
    VGH_REQUIRE(n_in >= 1 && keep_k >= 1 && keep_k <= n_in, "survivor_rows: n_in=%d / keep_k=%d", n_in, keep_k);
    VGH_REQUIRE(shape_c >= 0 && shape_c <= 300 && expr_c >= 0 && expr_c <= 100, "survivor_rows: bad live channel counts");
    RowOps R;
    memset(&R, 0, sizeof(R));
    if (int rc = make_levels(levels, n_levels, &R.L)) return rc;
    const int width = shape_c + expr_c + 13;
    for (int l = 0; l < n_levels; ++l) {
        VGH_REQUIRE(n_ops[l] >= 1 && n_ops[l] <= kMaxRowOps, "survivor_rows: level %d has %d ops", l, n_ops[l]);
        R.n[l] = n_ops[l];
        for (int k = 0; k < n_ops[l]; ++k) {
            const vgh_row_op& o = ops[l * kMaxRowOps + k];
            VGH_REQUIRE(vgh_row_op_ok(o, width), "survivor_rows: level %d op %d does not write FLAME channels of the prediction row from 16-byte aligned bf16 rows", l, k);
            R.op[l][k] = o;
        }
    }
    if (B == 0) return VGH_OK;
    hipLaunchKernelGGL(survivor_rows_kernel, dim3((keep_k + 31) / 32, B), dim3(256), 0, (hipStream_t)stream, R, n_in, keep_k, idx_dev, keep_idx_dev, counts_dev, shape_c, expr_c,
                       out_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

int vgh_survivor_towers(const vgh_head_level* levels, int n_levels, const vgh_tower_tree* trees, int B, int n_in, int keep_k, const int32_t* idx_dev,
                        const int32_t* keep_idx_dev, const int32_t* counts_dev, int shape_c, int expr_c, float* out_dev, void* stream) {
    VGH_REQUIRE(levels && trees && idx_dev && keep_idx_dev && counts_dev && out_dev, "survivor_towers: null argument");
    VGH_REQUIRE(n_in >= 1 && keep_k >= 1 && keep_k <= n_in && keep_k <= 65535 && B <= 65535, "survivor_towers: n_in=%d / keep_k=%d / B=%d", n_in, keep_k, B);
    VGH_REQUIRE(shape_c >= 0 && shape_c <= 300 && expr_c >= 0 && expr_c <= 100, "survivor_towers: bad live channel counts");
    TowerArgs T;
    memset(&T, 0, sizeof(T));
    if (int rc = make_levels(levels, n_levels, &T.L)) return rc;
    int lds = 0;
    for (int l = 0; l < n_levels; ++l) {
        VGH_REQUIRE(vgh_tower_tree_ok(trees[l], shape_c + expr_c + 13), "survivor_towers: the tree of level %d cannot be walked per survivor", l);
        T.t[l] = trees[l];
        const int bytes = vgh_tower_lds(trees[l], T.off[l]);
        lds = bytes > lds ? bytes : lds;
    }
    if (B == 0) return VGH_OK;
    static PerDevice opted_in;  // (the largest walk vgh_tower_tree_ok admits: one opt-in per device serves every tree)
    if (lds > 64 * 1024) VGH_HIP(opt_in_dynamic_lds(opted_in, 144 * 1024, survivor_towers_kernel));
    hipLaunchKernelGGL(survivor_towers_kernel, dim3(keep_k, B), dim3(512), lds, (hipStream_t)stream, T, n_in, keep_k, idx_dev, keep_idx_dev, counts_dev, shape_c, expr_c, out_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

extern "C" {
int vgh_compact(const float* boxes_dev, const float* scores_dev, const float* flame_dev, int B, int n_in, const int32_t* keep_idx_dev, int keep_k,
                float* out_boxes_dev, float* out_scores_dev, float* out_flame_dev, void* stream) {
    if (B == 0) return VGH_OK;
    hipLaunchKernelGGL(compact_kernel, dim3(keep_k, B), dim3(64), 0, (hipStream_t)stream, boxes_dev, scores_dev, flame_dev, n_in, keep_idx_dev, keep_k,
                       out_boxes_dev, out_scores_dev, out_flame_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

int64_t vgh_topk_nms_workspace_bytes(int B, int n, int pre_k, int keep_k) {
    const int64_t k = pre_k < n ? pre_k : n;
    return (int64_t)B * (k * 4 /*idx*/ + k * 4 /*sorted scores*/ + k * 16 /*sorted boxes*/ + (int64_t)keep_k * 4 /*keep*/) + 256;
}

int vgh_topk_nms(const float* boxes_dev, const float* scores_dev, const float* flame_dev, int flame_width, int B, int n, float conf_thr, float iou_thr, int pre_k,
                 int keep_k, void* workspace_dev, float* out_boxes_dev, float* out_scores_dev, float* out_flame_dev, int32_t* counts_dev, void* stream) {
    VGH_REQUIRE(boxes_dev && scores_dev && workspace_dev && out_boxes_dev && out_scores_dev && counts_dev, "topk_nms: null argument");
    VGH_REQUIRE((flame_dev == nullptr) == (out_flame_dev == nullptr) && (!flame_dev || flame_width > 0), "topk_nms: flame input / output must both be given or both be NULL");
    VGH_REQUIRE(B >= 0 && n >= 1 && pre_k >= 1 && keep_k >= 1, "topk_nms: bad sizes");
    const int k = pre_k < n ? pre_k : n;
    VGH_REQUIRE(k <= 1024, "topk_nms: min(pre_k, n) = %d exceeds the 1024 candidates the NMS kernel holds", k);
    if (B == 0) return VGH_OK;
    VGH_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "topk_nms: workspace must be 16-byte aligned");
    auto al16 = [](size_t x) { return (x + 15) & ~(size_t)15; };
    char* ws = (char*)workspace_dev;
    const size_t o_ssc = al16((size_t)B * k * 4), o_sbx = al16(o_ssc + (size_t)B * k * 4), o_keep = o_sbx + (size_t)B * k * 16;
    int32_t* idx = (int32_t*)ws;
    float* ssc = (float*)(ws + o_ssc);
    float* sbx = (float*)(ws + o_sbx);
    int32_t* keep = (int32_t*)(ws + o_keep);
    int rc;
    // utils.py:174-185: the score >= conf filter comes BEFORE the top-k.  One stable descending sort in which the rows that fail the filter rank behind every row that
    // passes: they fill candidate slots only where fewer than k rows pass, and vgh_nms never visits them
    if ((rc = topk_launch<true>(scores_dev, B, n, k, idx, ssc, conf_thr, stream))) return rc;
    hipLaunchKernelGGL(gather_boxes_kernel, dim3((k + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, boxes_dev, (const int32_t*)idx, n, k, sbx);
    VGH_HIP(hipGetLastError());
    if ((rc = vgh_nms(sbx, ssc, B, k, conf_thr, iou_thr, keep_k, keep, counts_dev, stream))) return rc;
    hipLaunchKernelGGL(compact_indirect_kernel, dim3(keep_k, B), dim3(64), 0, (hipStream_t)stream, boxes_dev, flame_dev, flame_width, n, (const int32_t*)idx,
                       (const float*)ssc, k, (const int32_t*)keep, keep_k, out_boxes_dev, out_scores_dev, out_flame_dev);
    VGH_HIP(hipGetLastError());
    return VGH_OK;
}

}  // extern "C"
