// libvgheval.so (include/vgh_eval.h), second source: COCO-style box evaluation, what the reference's head-detection benchmarks
// (yolo_head_training/evaluation/evaluate_wider.py, evaluate_fddb.py) ask of pycocotools' COCOeval(..., 'bbox'), for all images of a test set per call.
//
//   iou      the dense IoU block of every image: blockIdx.x = image, the workgroups of blockIdx.y (1 .. 64, by the set's pair count) stride over its nd x ng pairs.
//   match    one workgroup per image, one wave per IoU threshold.  The detections' ranks are found by counting (score, index) pairs as rank_kernel of
//            mesh_metrics.hip does, 4 x CAP scores in LDS at a time.  Then, area range after area range, the image's ground truths are staged into LDS
//            as float64 in the order the matching walks them (non-ignored first), and every wave runs its threshold's greedy matching over the
//            detections in rank order: the lanes stride over the ground truths, IoUs are recomputed, never stored, and the lanes reduce to (highest
//            IoU, then highest position), which is what the sequential walk with its ">=" update ends on.  A lane owns positions lane, lane + 64, ...,
//            at most 64 of them, so "already matched" is one 64-bit register per lane.  CAP = 512 (17 KB of LDS) serves the common case, CAP = 4096
//            (136 KB of gfx950's 160 KB) the ceiling.
//   sort     the global order (-score, image, rank) of the kept detections: a bitonic sort of (64-bit key, position) in the caller's scratch.  The kept
//            arrays are already in (image, rank) order, so the position breaks ties and the order is total: any correct sort gives one answer.
//            Steps whose partners lie within 2 048 keys run in LDS, one launch per merge; only partners further apart take a global pass each.
//   curve    one workgroup per (threshold, area range, max_dets[k]) walks the sorted detections 1024 at a time: an exact integer scan gives tp, fp and
//            the number of detections of rank < max_dets[k]; a recall threshold "opens" at the one position whose recall first reaches it, takes the
//            maximum of pr from there to the end of its chunk and, from then on, every later chunk's maximum.  A maximum is exact in any order.
// Counts are integers, n_pos is one integer atomic per (image, area range), there is no float atomic, and every float is one float64 operation in the
// order include/vgh_eval.h states with contraction off: every output is bitwise reproducible and equal to tests/detection_ap_ref.py.
#include <math.h>

#include <algorithm>

#include "../../include/vgh_eval.h"
#include "companion_host.h"

#pragma clang fp contract(off)

namespace {

using namespace companion;
static_assert(VGHEV_OK == OK && VGHEV_ERR_INVALID == ERR_INVALID && VGHEV_ERR_HIP == ERR_HIP, "companion_host.h returns these codes");  // this library allocates nothing: its header has no NOMEM

constexpr int WAVE = 64;
constexpr int IOU_LANES = 256;
constexpr int IOU_CHUNKS = 64;      // at most this many workgroups stride over one image's pairs
constexpr int CAP_SMALL = 512;      // ground truths of one image held in LDS: the common case
constexpr int CAP_LARGE = VGHEV_MAX_GT_PER_IMAGE;
constexpr int CURVE_LANES = 1024;   // one chunk of the sorted detections
constexpr int SORT_LANES = 256;
constexpr int SORT_LOCAL = 2048;    // keys one workgroup sorts in LDS: 24 KB
static_assert(CAP_LARGE <= WAVE * 64, "a lane's matched flags are one 64-bit register");
static_assert(CAP_LARGE <= 0x8000, "s_idx keeps the crowd flag in bit 15");

// one image's ranges, checked against the array sizes; false = inconsistent, the image is left out
struct Range {
    int dlo, nd, glo, ng;
};
__device__ __forceinline__ bool image_range(const vghev_box_set& s, int img, Range& r) {
    r.dlo = s.dt_offset_dev[img];
    r.nd = s.dt_offset_dev[img + 1] - r.dlo;
    r.glo = s.gt_offset_dev[img];
    r.ng = s.gt_offset_dev[img + 1] - r.glo;
    return r.dlo >= 0 && r.nd >= 0 && r.nd <= s.n_dt - r.dlo && r.glo >= 0 && r.ng >= 0 && r.ng <= s.n_gt - r.glo && r.ng <= s.max_gt;
}

// bbIou: every operation rounded on its own
__device__ __forceinline__ double box_iou(double dx, double dy, double dx2, double dy2, double da, double gx, double gy, double gw, double gh, bool crowd) {
    const double w = __dsub_rn(fmin(dx2, __dadd_rn(gx, gw)), fmax(dx, gx));
    if (!(w > 0.0)) return 0.0;
    const double h = __dsub_rn(fmin(dy2, __dadd_rn(gy, gh)), fmax(dy, gy));
    if (!(h > 0.0)) return 0.0;
    const double i = __dmul_rn(w, h);
    const double u = crowd ? da : __dsub_rn(__dadd_rn(da, __dmul_rn(gw, gh)), i);
    return __ddiv_rn(i, u);
}

// ---- vghev_box_iou ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(IOU_LANES) void iou_kernel(vghev_box_set s, const int64_t* __restrict__ iou_offset, int64_t n_iou, double* __restrict__ iou,
                                                         int32_t* __restrict__ status) {
    const int img = (int)blockIdx.x;
    Range r;
    const int64_t lo = iou_offset[img];
    const int64_t pairs = iou_offset[img + 1] - lo;
    if (!image_range(s, img, r) || lo < 0 || pairs != (int64_t)r.nd * r.ng || pairs > n_iou - lo) {
        if (threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, 1);
        return;
    }
    for (int64_t e = (int64_t)blockIdx.y * IOU_LANES + threadIdx.x; e < pairs; e += (int64_t)gridDim.y * IOU_LANES) {
        const int d = (int)(e / r.ng), g = (int)(e % r.ng);
        const double* D = s.dt_box_dev + (size_t)(r.dlo + d) * 4;
        const double* G = s.gt_box_dev + (size_t)(r.glo + g) * 4;
        const bool crowd = s.gt_crowd_dev && s.gt_crowd_dev[r.glo + g];
        iou[lo + e] = box_iou(D[0], D[1], __dadd_rn(D[0], D[2]), __dadd_rn(D[1], D[3]), __dmul_rn(D[2], D[3]), G[0], G[1], G[2], G[3], crowd);
    }
}

// ---- vghev_box_match -------------------------------------------------------------------------------------------------------------------------------
// the wave's best (IoU, position): the highest IoU, of equal ones the highest position; pos < 0 = none
__device__ __forceinline__ void wave_best(double& best, int& pos) {
#pragma unroll
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, WAVE);
        const int op = __shfl_xor(pos, off, WAVE);
        if (op >= 0 && (pos < 0 || ob > best || (ob == best && op > pos))) {
            best = ob;
            pos = op;
        }
    }
}

struct MatchArgs {
    vghev_box_set s;
    int T, A, max_det;
    int64_t n_kept;
    const double* iou_thr;
    const double* area_rng;
    const int32_t* kept_offset;
    int32_t* match;
    uint8_t* ignore;
    int32_t* det_image;
    int32_t* det_rank;
    int32_t* det_index;
    double* det_score;
    int32_t* n_pos;
    int32_t* status;
};

// blockIdx.x = image, blockDim.x = T * 64: wave t runs threshold t
template <int CAP>
__global__ __launch_bounds__(VGHEV_MAX_IOU_THR* WAVE) void match_kernel(MatchArgs a) {
    __shared__ double s_box[CAP * 4];  // the scores' tile while ranking, then the ground truths in matching order
    __shared__ uint16_t s_idx[CAP];    // a staged ground truth's input index; bit 15 = crowd
    __shared__ int s_wave[2][VGHEV_MAX_IOU_THR];
    __shared__ int s_valid;
    const int img = (int)blockIdx.x, tid = (int)threadIdx.x, lanes = (int)blockDim.x, wave = tid / WAVE, lane = tid % WAVE, waves = lanes / WAVE;
    Range r;
    const int klo = a.kept_offset[img];
    const int kept = a.kept_offset[img + 1] - klo;
    if (!image_range(a.s, img, r) || r.ng > CAP || klo < 0 || kept != min(r.nd, a.max_det) || (int64_t)kept > a.n_kept - klo) {  // the same for every lane
        if (tid == 0) atomicOr(a.status, 1);
        return;
    }
    const double* score = a.s.dt_score_dev + r.dlo;
    // ---- ranks: the number of detections that order before (score, index) ----
    constexpr int SCORE_TILE = CAP * 4;
    for (int d0 = 0; d0 < r.nd; d0 += lanes) {
        const int d = d0 + tid;
        const bool live = d < r.nd;
        const double sd = live ? score[d] : 0.0;
        int rank = 0;
        for (int base = 0; base < r.nd; base += SCORE_TILE) {
            const int m = min(SCORE_TILE, r.nd - base);
            __syncthreads();
            for (int k = tid; k < m; k += lanes) s_box[k] = score[base + k];
            __syncthreads();
            for (int k = 0; k < m; ++k) {
                const double se = s_box[k];
                rank += (se > sd || (se == sd && base + k < d)) ? 1 : 0;
            }
        }
        if (live && rank < kept) {  // rank <= nd - 1 whatever the data: the detection itself never counts
            const size_t q = (size_t)klo + rank;
            a.det_image[q] = img;
            a.det_rank[q] = rank;
            a.det_index[q] = d;
            a.det_score[q] = sd;
        }
    }
    __syncthreads();  // det_index is read back below, by other waves
    const double* gt_box = a.s.gt_box_dev + (size_t)r.glo * 4;
    const double* gt_area = a.s.gt_area_dev ? a.s.gt_area_dev + r.glo : nullptr;
    const uint8_t* gt_crowd = a.s.gt_crowd_dev ? a.s.gt_crowd_dev + r.glo : nullptr;
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (WAVE - lane));  // the lanes before this one
    for (int ar = 0; ar < a.A; ++ar) {
        const double lo = a.area_rng[2 * ar], hi = a.area_rng[2 * ar + 1];
        // ---- stage the ground truths: non-ignored first, then ignored, each group in input order ----
        __syncthreads();  // the previous range's matchings are done with s_box
        if (tid == 0) s_valid = 0;
        __syncthreads();
        int mine = 0;
        for (int g = tid; g < r.ng; g += lanes) {
            const double area = gt_area ? gt_area[g] : __dmul_rn(gt_box[4 * g + 2], gt_box[4 * g + 3]);
            mine += ((gt_crowd && gt_crowd[g]) || area < lo || area > hi) ? 0 : 1;
        }
        if (mine) atomicAdd(&s_valid, mine);
        __syncthreads();
        const int valid = s_valid;
        int before_v = 0, before_i = 0;
        for (int g0 = 0; g0 < r.ng; g0 += lanes) {
            const int g = g0 + tid;
            const bool live = g < r.ng;
            bool crowd = false, ign = false;
            double bx = 0.0, by = 0.0, bw = 0.0, bh = 0.0;
            if (live) {
                bx = gt_box[4 * g], by = gt_box[4 * g + 1], bw = gt_box[4 * g + 2], bh = gt_box[4 * g + 3];
                crowd = gt_crowd && gt_crowd[g];
                const double area = gt_area ? gt_area[g] : __dmul_rn(bw, bh);
                ign = crowd || area < lo || area > hi;
            }
            const uint64_t mv = __ballot(live && !ign), mi = __ballot(live && ign);
            if (lane == 0) {
                s_wave[0][wave] = __popcll(mv);
                s_wave[1][wave] = __popcll(mi);
            }
            __syncthreads();
            int pv = before_v, pi = before_i;
            for (int w = 0; w < waves; ++w) {
                if (w < wave) {
                    pv += s_wave[0][w];
                    pi += s_wave[1][w];
                }
                before_v += s_wave[0][w];
                before_i += s_wave[1][w];
            }
            if (live) {
                const int pos = ign ? valid + pi + __popcll(mi & below) : pv + __popcll(mv & below);  // < ng: the counts are this image's
                s_box[4 * pos] = bx;
                s_box[4 * pos + 1] = by;
                s_box[4 * pos + 2] = bw;
                s_box[4 * pos + 3] = bh;
                s_idx[pos] = (uint16_t)(g | (crowd ? 0x8000 : 0));
            }
            __syncthreads();  // s_wave is rewritten by the next group
        }
        if (tid == 0 && valid) atomicAdd(a.n_pos + ar, valid);
        // ---- wave t: the greedy matching at threshold t ----
        const int t = wave;
        const double thr = fmin(a.iou_thr[t], 1.0 - 1e-10);
        const size_t out = ((size_t)ar * a.T + t) * (size_t)a.n_kept + klo;
        uint64_t matched = 0;  // bit k: position lane + 64 * k is matched at this threshold
        for (int p = 0; p < kept; ++p) {
            const int d = min(max(a.det_index[klo + p], 0), r.nd - 1);  // kept > 0 means nd > 0; a slot no rank filled (NaN scores) holds anything
            const double* D = a.s.dt_box_dev + (size_t)(r.dlo + d) * 4;
            const double dx = D[0], dy = D[1];
            const double dx2 = __dadd_rn(dx, D[2]), dy2 = __dadd_rn(dy, D[3]), da = __dmul_rn(D[2], D[3]);
            double best = thr;
            int pos = -1;
            for (int k = 0, j = lane; j < valid; ++k, j += WAVE) {  // the non-ignored: none of them is crowd
                if ((matched >> k) & 1) continue;
                const double o = box_iou(dx, dy, dx2, dy2, da, s_box[4 * j], s_box[4 * j + 1], s_box[4 * j + 2], s_box[4 * j + 3], false);
                if (o >= best) {
                    best = o;
                    pos = j;
                }
            }
            wave_best(best, pos);
            if (pos < 0) {  // no non-ignored match: the walk goes on into the ignored ones with best unchanged
                best = thr;
                for (int k = valid / WAVE, j = k * WAVE + lane; j < r.ng; ++k, j += WAVE) {
                    if (j < valid) continue;
                    const bool crowd = (s_idx[j] & 0x8000) != 0;
                    if (((matched >> k) & 1) && !crowd) continue;
                    const double o = box_iou(dx, dy, dx2, dy2, da, s_box[4 * j], s_box[4 * j + 1], s_box[4 * j + 2], s_box[4 * j + 3], crowd);
                    if (o >= best) {
                        best = o;
                        pos = j;
                    }
                }
                wave_best(best, pos);
            }
            if (pos >= 0 && lane == pos % WAVE) matched |= 1ull << (pos / WAVE);
            if (lane == 0) {
                a.match[out + p] = pos >= 0 ? (int32_t)(s_idx[pos] & 0x7fff) : -1;
                a.ignore[out + p] = pos >= 0 ? (pos >= valid ? 1 : 0) : ((da < lo || da > hi) ? 1 : 0);
            }
        }
    }
}

// ---- the global order ------------------------------------------------------------------------------------------------------------------------------
// ascending key = descending score; -0.0 and 0.0 are one score; the padding (position >= n) orders last
__global__ __launch_bounds__(SORT_LANES) void sort_keys_kernel(const double* __restrict__ score, int64_t n, int64_t n2, uint64_t* __restrict__ key,
                                                                uint32_t* __restrict__ at) {
    const int64_t q = (int64_t)blockIdx.x * SORT_LANES + threadIdx.x;
    if (q >= n2) return;
    uint64_t k = ~0ull;
    if (q < n) {
        const uint64_t b = (uint64_t)__double_as_longlong(__dadd_rn(score[q], 0.0));
        k = ~((b >> 63) ? ~b : (b | 0x8000000000000000ull));
    }
    key[q] = k;
    at[q] = (uint32_t)q;
}

__global__ __launch_bounds__(SORT_LANES) void bitonic_kernel(uint64_t* __restrict__ key, uint32_t* __restrict__ at, int64_t n2, int64_t j, int64_t k) {
    const int64_t i = (int64_t)blockIdx.x * SORT_LANES + threadIdx.x;
    const int64_t l = i ^ j;
    if (i >= n2 || l <= i) return;
    const uint64_t ki = key[i], kl = key[l];
    const uint32_t ai = at[i], al = at[l];
    const bool greater = ki > kl || (ki == kl && ai > al);
    if (greater == ((i & k) == 0)) {
        key[i] = kl;
        key[l] = ki;
        at[i] = al;
        at[l] = ai;
    }
}

// The steps whose partners lie inside one block of SORT_LOCAL elements, in LDS: for k = k_lo, 2 k_lo, .., k_hi the merges j = min(k / 2, SORT_LOCAL / 2)
// .. 1.  One launch with (2, min(n2, SORT_LOCAL)) sorts every block; for a larger k one launch with (k, k) finishes what the global steps j >= SORT_LOCAL began.
__global__ __launch_bounds__(SORT_LOCAL / 2) void bitonic_local_kernel(uint64_t* __restrict__ key, uint32_t* __restrict__ at, int64_t n2, int64_t k_lo, int64_t k_hi) {
    __shared__ uint64_t s_key[SORT_LOCAL];
    __shared__ uint32_t s_at[SORT_LOCAL];
    const int m = (int)(n2 < SORT_LOCAL ? n2 : SORT_LOCAL);  // a power of two; n2 is a multiple of it
    const int64_t base = (int64_t)blockIdx.x * m;
    const int t = (int)threadIdx.x;
    for (int e = t; e < m; e += SORT_LOCAL / 2) {
        s_key[e] = key[base + e];
        s_at[e] = at[base + e];
    }
    __syncthreads();
    for (int64_t k = k_lo; k <= k_hi; k <<= 1) {
        for (int j = (int)(k / 2 < m / 2 ? k / 2 : m / 2); j > 0; j >>= 1) {
            if (t < m / 2) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;  // the pair's lower and upper element
                const uint64_t ki = s_key[i], kl = s_key[l];
                const uint32_t ai = s_at[i], al = s_at[l];
                const bool greater = ki > kl || (ki == kl && ai > al);
                if (greater == (((base + i) & k) == 0)) {
                    s_key[i] = kl;
                    s_key[l] = ki;
                    s_at[i] = al;
                    s_at[l] = ai;
                }
            }
            __syncthreads();
        }
    }
    for (int e = t; e < m; e += SORT_LOCAL / 2) {
        key[base + e] = s_key[e];
        at[base + e] = s_at[e];
    }
}

__global__ __launch_bounds__(SORT_LANES) void sorted_kernel(const uint32_t* __restrict__ at, const int32_t* __restrict__ det_rank,
                                                             const double* __restrict__ det_score, int64_t n, int32_t* __restrict__ srt_rank,
                                                             double* __restrict__ srt_score) {
    const int64_t q = (int64_t)blockIdx.x * SORT_LANES + threadIdx.x;
    if (q >= n) return;
    const uint32_t p = min(at[q], (uint32_t)(n - 1));  // a permutation of 0 .. n2 - 1 whose first n entries are < n
    srt_rank[q] = det_rank[p];
    srt_score[q] = det_score[p];
}

// ---- the curves ------------------------------------------------------------------------------------------------------------------------------------
struct Counts {
    int in, tp, fp;  // detections of rank < max_dets[k]; of them matched and not ignored; unmatched and not ignored
};

struct CurveArgs {
    int64_t n;
    int T, R, A, M;
    int max_dets[VGHEV_MAX_MAX_DETS];
    const double* rec_thr;
    const int32_t* match;
    const uint8_t* ignore;
    const int32_t* n_pos;
    const uint32_t* at;
    const int32_t* srt_rank;
    const double* srt_score;
    double* precision;
    double* scores;
    double* recall;
};

// blockIdx.x = (t * A + a) * M + k
__global__ __launch_bounds__(CURVE_LANES) void curve_kernel(CurveArgs c) {
    __shared__ double s_thr[VGHEV_MAX_REC_THR], s_prec[VGHEV_MAX_REC_THR], s_score[VGHEV_MAX_REC_THR], s_pr[CURVE_LANES];
    __shared__ int64_t s_open[VGHEV_MAX_REC_THR];  // the sorted position a threshold opened at; -1 not yet, -2 its own chunk is accounted for
    __shared__ Counts s_wave[CURVE_LANES / WAVE];
    __shared__ double s_wmax[CURVE_LANES / WAVE];
    const int tid = (int)threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
    const int k = (int)(blockIdx.x % (unsigned)c.M), ar = (int)((blockIdx.x / (unsigned)c.M) % (unsigned)c.A), t = (int)(blockIdx.x / (unsigned)(c.M * c.A));
    const int n_pos = c.n_pos[ar], max_det = c.max_dets[k];
    const size_t rec_at = ((size_t)t * c.A + ar) * c.M + k;
    if (n_pos <= 0) {
        for (int r = tid; r < c.R; r += CURVE_LANES) {
            const size_t o = (((size_t)t * c.R + r) * c.A + ar) * c.M + k;
            c.precision[o] = -1.0;
            c.scores[o] = -1.0;
        }
        if (tid == 0) c.recall[rec_at] = -1.0;
        return;
    }
    for (int r = tid; r < c.R; r += CURVE_LANES) {
        s_thr[r] = c.rec_thr[r];
        s_prec[r] = 0.0;
        s_score[r] = 0.0;
        s_open[r] = -1;
    }
    const double npos = (double)n_pos;
    const size_t flags = ((size_t)ar * c.T + t) * (size_t)c.n;
    Counts base = {0, 0, 0};
    for (int64_t q0 = 0; q0 < c.n; q0 += CURVE_LANES) {
        const int64_t q = q0 + tid;
        Counts me = {0, 0, 0};
        double sc = 0.0;
        if (q < c.n && c.srt_rank[q] < max_det) {
            const size_t p = flags + min((int64_t)c.at[q], c.n - 1);
            const bool hit = c.match[p] >= 0, ign = c.ignore[p] != 0;
            me.in = 1;
            me.tp = (hit && !ign) ? 1 : 0;
            me.fp = (!hit && !ign) ? 1 : 0;
            sc = c.srt_score[q];
        }
        Counts sum = me;  // inclusive scan: the wave's, then the waves before
#pragma unroll
        for (int off = 1; off < WAVE; off <<= 1) {
            const int oi = __shfl_up(sum.in, off, WAVE), ot = __shfl_up(sum.tp, off, WAVE), of = __shfl_up(sum.fp, off, WAVE);
            if (lane >= off) {
                sum.in += oi;
                sum.tp += ot;
                sum.fp += of;
            }
        }
        __syncthreads();  // the previous chunk is done with s_wave, s_wmax and s_pr; the first: the thresholds are in LDS
        if (lane == WAVE - 1) s_wave[wave] = sum;
        __syncthreads();
        Counts total = base;
        for (int w = 0; w < CURVE_LANES / WAVE; ++w) {
            if (w == wave) {
                sum.in += total.in;
                sum.tp += total.tp;
                sum.fp += total.fp;
            }
            total.in += s_wave[w].in;
            total.tp += s_wave[w].tp;
            total.fp += s_wave[w].fp;
        }
        base = total;
        const double pr = me.in ? __ddiv_rn((double)sum.tp, __dadd_rn((double)(sum.fp + sum.tp), 2.220446049250313e-16)) : 0.0;  // pr >= 0: a 0 never wins
        s_pr[tid] = pr;
        double wmax = pr;
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) wmax = fmax(wmax, __shfl_xor(wmax, off, WAVE));
        if (lane == 0) s_wmax[wave] = wmax;
        if (me.in && (sum.in == 1 || me.tp)) {  // recall rises here (or this is the first position): the thresholds it reaches for the first time
            const double rc = __ddiv_rn((double)sum.tp, npos);
            const double rc_before = sum.in == 1 ? -INFINITY : __ddiv_rn((double)(sum.tp - me.tp), npos);
            for (int r = 0; r < c.R; ++r) {
                const double thr = s_thr[r];
                if (rc_before < thr && thr <= rc) {  // one position per threshold: the intervals do not overlap
                    s_open[r] = q;
                    s_score[r] = sc;
                }
            }
        }
        __syncthreads();
        double cmax = s_wmax[0];
        for (int w = 1; w < CURVE_LANES / WAVE; ++w) cmax = fmax(cmax, s_wmax[w]);
        for (int r = tid; r < c.R; r += CURVE_LANES) {
            const int64_t at = s_open[r];
            if (at >= 0) {  // opened in this chunk: pr's maximum from its position to the chunk's end
                double m = 0.0;
                for (int e = (int)(at - q0); e < CURVE_LANES; ++e) m = fmax(m, s_pr[e]);
                s_prec[r] = m;
                s_open[r] = -2;
            } else if (at == -2) {
                s_prec[r] = fmax(s_prec[r], cmax);
            }
        }
    }
    __syncthreads();
    for (int r = tid; r < c.R; r += CURVE_LANES) {
        const size_t o = (((size_t)t * c.R + r) * c.A + ar) * c.M + k;
        c.precision[o] = s_prec[r];
        c.scores[o] = s_score[r];
    }
    if (tid == 0) c.recall[rec_at] = base.in ? __ddiv_rn((double)base.tp, npos) : 0.0;
}

int64_t pow2_at_least(int64_t n) {
    int64_t p = 1;
    while (p < n) p <<= 1;
    return p;
}

// the scratch of vghev_pr_accumulate: keys u64 [n2], positions u32 [n2], sorted ranks i32 [n], sorted scores f64 [n]
struct ScratchPlan {
    int64_t n2;
    size_t key, at, rank, score, bytes;
};
ScratchPlan plan_scratch(int64_t n) {
    ScratchPlan p;
    p.n2 = pow2_at_least(n);
    p.key = 0;
    p.at = p.key + align16((size_t)p.n2 * sizeof(uint64_t));
    p.rank = p.at + align16((size_t)p.n2 * sizeof(uint32_t));
    p.score = p.rank + align16((size_t)n * sizeof(int32_t));
    p.bytes = p.score + align16((size_t)n * sizeof(double));
    return p;
}

int check_set(const vghev_box_set& s, const char* who) {
    CH_REQUIRE(s.n_images >= 0 && s.n_images <= VGHEV_MAX_IMAGES, "%s: n_images = %d outside 0 .. %d", who, s.n_images, VGHEV_MAX_IMAGES);
    CH_REQUIRE(s.n_dt >= 0 && s.n_gt >= 0, "%s: n_dt = %d and n_gt = %d must not be negative", who, s.n_dt, s.n_gt);
    CH_REQUIRE(s.max_gt >= 0 && s.max_gt <= VGHEV_MAX_GT_PER_IMAGE, "%s: max_gt = %d outside 0 .. %d ground truths per image", who, s.max_gt,
               VGHEV_MAX_GT_PER_IMAGE);
    return OK;
}

int check_set_pointers(const vghev_box_set& s, const char* who) {
    CH_REQUIRE(s.dt_offset_dev && s.gt_offset_dev, "%s: dt_offset_dev and gt_offset_dev must not be NULL", who);
    CH_REQUIRE(s.n_dt == 0 || s.dt_box_dev, "%s: dt_box_dev must not be NULL", who);
    CH_REQUIRE(s.n_gt == 0 || s.gt_box_dev, "%s: gt_box_dev must not be NULL", who);
    return OK;
}

}  // namespace

extern "C" VGHEV_API int64_t vghev_ap_scratch_bytes(int64_t n_kept) {
    CH_REQUIRE(n_kept >= 0 && n_kept <= VGHEV_MAX_KEPT, "ap_scratch_bytes: n_kept = %lld outside 0 .. %d", (long long)n_kept, VGHEV_MAX_KEPT);
    return (int64_t)plan_scratch(n_kept).bytes;
}

extern "C" VGHEV_API int vghev_box_iou(const vghev_box_iou_job* job, void* stream) {
    CH_REQUIRE(job != nullptr, "box_iou: job is NULL");
    const vghev_box_iou_job& j = *job;
    if (const int rc = check_set(j.set, "box_iou")) return rc;
    CH_REQUIRE(j.n_iou >= 0, "box_iou: n_iou = %lld must not be negative", (long long)j.n_iou);
    if (j.set.n_images == 0) return OK;
    if (const int rc = check_set_pointers(j.set, "box_iou")) return rc;
    CH_REQUIRE(j.iou_offset_dev && j.status_dev, "box_iou: iou_offset_dev and status_dev must not be NULL");
    CH_REQUIRE(j.n_iou == 0 || j.iou_dev, "box_iou: iou_dev must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    CH_HIP(hipMemsetAsync(j.status_dev, 0, sizeof(int32_t), st));
    // no image holds more than n_iou pairs: a set of many small images gets one workgroup per image
    const unsigned chunks = (unsigned)std::min<int64_t>(IOU_CHUNKS, std::max<int64_t>(1, (j.n_iou + IOU_LANES - 1) / IOU_LANES));
    hipLaunchKernelGGL(iou_kernel, dim3((unsigned)j.set.n_images, chunks), dim3(IOU_LANES), 0, st, j.set, j.iou_offset_dev, j.n_iou, j.iou_dev, j.status_dev);
    CH_HIP(hipGetLastError());
    return OK;
}

extern "C" VGHEV_API int vghev_box_match(const vghev_box_match_job* job, void* stream) {
    CH_REQUIRE(job != nullptr, "box_match: job is NULL");
    const vghev_box_match_job& j = *job;
    if (const int rc = check_set(j.set, "box_match")) return rc;
    CH_REQUIRE(j.n_iou_thr >= 1 && j.n_iou_thr <= VGHEV_MAX_IOU_THR, "box_match: n_iou_thr = %d outside 1 .. %d", j.n_iou_thr, VGHEV_MAX_IOU_THR);
    CH_REQUIRE(j.n_area >= 1 && j.n_area <= VGHEV_MAX_AREA_RNG, "box_match: n_area = %d outside 1 .. %d", j.n_area, VGHEV_MAX_AREA_RNG);
    CH_REQUIRE(j.max_det >= 1 && j.max_det <= VGHEV_MAX_DET, "box_match: max_det = %d outside 1 .. %d", j.max_det, VGHEV_MAX_DET);
    CH_REQUIRE(j.reserved == 0, "box_match: reserved must be 0");
    CH_REQUIRE(j.n_kept >= 0 && j.n_kept <= j.set.n_dt && j.n_kept <= VGHEV_MAX_KEPT, "box_match: n_kept = %lld outside 0 .. n_dt = %d", (long long)j.n_kept,
               j.set.n_dt);
    CH_REQUIRE(j.n_pos_dev && j.status_dev, "box_match: n_pos_dev and status_dev must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    if (j.set.n_images == 0) return OK;  // nothing is queued: n_pos and status stay as the caller left them
    if (const int rc = check_set_pointers(j.set, "box_match")) return rc;
    CH_REQUIRE(j.set.n_dt == 0 || j.set.dt_score_dev, "box_match: dt_score_dev must not be NULL");
    CH_REQUIRE(j.iou_thr_dev && j.area_rng_dev && j.kept_offset_dev, "box_match: iou_thr_dev, area_rng_dev and kept_offset_dev must not be NULL");
    CH_REQUIRE(j.n_kept == 0 || (j.match_dev && j.ignore_dev && j.det_image_dev && j.det_rank_dev && j.det_index_dev && j.det_score_dev),
               "box_match: match_dev, ignore_dev, det_image_dev, det_rank_dev, det_index_dev and det_score_dev must not be NULL");
    CH_HIP(hipMemsetAsync(j.n_pos_dev, 0, (size_t)j.n_area * sizeof(int32_t), st));
    CH_HIP(hipMemsetAsync(j.status_dev, 0, sizeof(int32_t), st));
    MatchArgs a = {j.set,       j.n_iou_thr, j.n_area,       j.max_det,      j.n_kept,        j.iou_thr_dev, j.area_rng_dev, j.kept_offset_dev,
                   j.match_dev, j.ignore_dev, j.det_image_dev, j.det_rank_dev, j.det_index_dev, j.det_score_dev, j.n_pos_dev,   j.status_dev};
    const dim3 grid((unsigned)j.set.n_images), block((unsigned)(j.n_iou_thr * WAVE));
    if (j.set.max_gt <= CAP_SMALL)
        hipLaunchKernelGGL(match_kernel<CAP_SMALL>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(match_kernel<CAP_LARGE>, grid, block, 0, st, a);
    CH_HIP(hipGetLastError());
    return OK;
}

extern "C" VGHEV_API int vghev_pr_accumulate(const vghev_pr_job* job, void* stream) {
    CH_REQUIRE(job != nullptr, "pr_accumulate: job is NULL");
    const vghev_pr_job& j = *job;
    CH_REQUIRE(j.n_kept >= 0 && j.n_kept <= VGHEV_MAX_KEPT, "pr_accumulate: n_kept = %lld outside 0 .. %d", (long long)j.n_kept, VGHEV_MAX_KEPT);
    CH_REQUIRE(j.n_iou_thr >= 1 && j.n_iou_thr <= VGHEV_MAX_IOU_THR, "pr_accumulate: n_iou_thr = %d outside 1 .. %d", j.n_iou_thr, VGHEV_MAX_IOU_THR);
    CH_REQUIRE(j.n_rec_thr >= 1 && j.n_rec_thr <= VGHEV_MAX_REC_THR, "pr_accumulate: n_rec_thr = %d outside 1 .. %d", j.n_rec_thr, VGHEV_MAX_REC_THR);
    CH_REQUIRE(j.n_area >= 1 && j.n_area <= VGHEV_MAX_AREA_RNG, "pr_accumulate: n_area = %d outside 1 .. %d", j.n_area, VGHEV_MAX_AREA_RNG);
    CH_REQUIRE(j.n_max_dets >= 1 && j.n_max_dets <= VGHEV_MAX_MAX_DETS, "pr_accumulate: n_max_dets = %d outside 1 .. %d", j.n_max_dets, VGHEV_MAX_MAX_DETS);
    for (int k = 0; k < j.n_max_dets; ++k) {
        CH_REQUIRE(j.max_dets[k] >= 1 && j.max_dets[k] <= VGHEV_MAX_DET, "pr_accumulate: max_dets[%d] = %d outside 1 .. %d", k, j.max_dets[k], VGHEV_MAX_DET);
        CH_REQUIRE(k == 0 || j.max_dets[k] >= j.max_dets[k - 1], "pr_accumulate: max_dets must ascend, got %d after %d", j.max_dets[k], j.max_dets[k - 1]);
    }
    const ScratchPlan p = plan_scratch(j.n_kept);
    CH_REQUIRE(j.scratch_bytes >= (int64_t)p.bytes, "pr_accumulate: %lld bytes of scratch, %zu are needed for %lld detections", (long long)j.scratch_bytes,
               p.bytes, (long long)j.n_kept);
    CH_REQUIRE(j.rec_thr_dev && j.n_pos_dev && j.precision_dev && j.scores_dev && j.recall_dev,
               "pr_accumulate: rec_thr_dev, n_pos_dev, precision_dev, scores_dev and recall_dev must not be NULL");
    CH_REQUIRE(j.n_kept == 0 || (j.match_dev && j.ignore_dev && j.det_rank_dev && j.det_score_dev && j.scratch_dev),
               "pr_accumulate: match_dev, ignore_dev, det_rank_dev, det_score_dev and scratch_dev must not be NULL");
    CH_REQUIRE(((uintptr_t)j.scratch_dev & 15) == 0, "pr_accumulate: scratch_dev must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    uint8_t* scratch = (uint8_t*)j.scratch_dev;
    uint64_t* key = (uint64_t*)(scratch + p.key);
    uint32_t* at = (uint32_t*)(scratch + p.at);
    int32_t* srt_rank = (int32_t*)(scratch + p.rank);
    double* srt_score = (double*)(scratch + p.score);
    if (j.n_kept > 0) {
        const unsigned blocks2 = (unsigned)((p.n2 + SORT_LANES - 1) / SORT_LANES), blocks = (unsigned)((j.n_kept + SORT_LANES - 1) / SORT_LANES);
        hipLaunchKernelGGL(sort_keys_kernel, dim3(blocks2), dim3(SORT_LANES), 0, st, j.det_score_dev, j.n_kept, p.n2, key, at);
        const int64_t local = std::min<int64_t>(p.n2, SORT_LOCAL);
        const dim3 local_grid((unsigned)(p.n2 / local)), local_block(SORT_LOCAL / 2);
        if (p.n2 > 1) hipLaunchKernelGGL(bitonic_local_kernel, local_grid, local_block, 0, st, key, at, p.n2, (int64_t)2, local);
        for (int64_t k = 2 * local; k <= p.n2; k <<= 1) {  // partners a block apart or more go through global memory, the rest of the merge through LDS
            for (int64_t h = k >> 1; h >= local; h >>= 1) hipLaunchKernelGGL(bitonic_kernel, dim3(blocks2), dim3(SORT_LANES), 0, st, key, at, p.n2, h, k);
            hipLaunchKernelGGL(bitonic_local_kernel, local_grid, local_block, 0, st, key, at, p.n2, k, k);
        }
        hipLaunchKernelGGL(sorted_kernel, dim3(blocks), dim3(SORT_LANES), 0, st, (const uint32_t*)at, j.det_rank_dev, j.det_score_dev, j.n_kept, srt_rank, srt_score);
    }
    CurveArgs c = {j.n_kept,    j.n_iou_thr,  j.n_rec_thr,  j.n_area,        j.n_max_dets,    {0, 0, 0, 0},    j.rec_thr_dev,   j.match_dev,
                   j.ignore_dev, j.n_pos_dev, at,           srt_rank,        srt_score,       j.precision_dev, j.scores_dev,    j.recall_dev};
    for (int k = 0; k < j.n_max_dets; ++k) c.max_dets[k] = j.max_dets[k];
    hipLaunchKernelGGL(curve_kernel, dim3((unsigned)(j.n_iou_thr * j.n_area * j.n_max_dets)), dim3(CURVE_LANES), 0, st, c);
    CH_HIP(hipGetLastError());
    return OK;
}
