// libvgheval.so (include/vgh_eval.h): the two neighbour searches behind the DAD-3DHeads mesh metrics of the reference
// (yolo_head_training/evaluation/dad_utils.py: calc_zn, calc_ch_dist), for all heads of a test set in one call.
//
//   rank     Z_n as the source computes it.  It sorts every column of the N x N distance matrix and then slices COLUMNS 1 .. top_k of the result, so the
//            partner of (i, j) is the point of rank i among the distances to vertex j + 1.  One workgroup per (head, column, 256 points): the distances
//            of ALL points to the column's vertex are the same for every lane, so they are computed once, 1024 at a time, into LDS, and every lane counts
//            how many of them order before its own point's (distance, index).  That count is the lane's rank = the i it is the partner of.
//   nearest  one query per lane, one workgroup per (head, 128 queries).  The head's points stream through LDS 512 at a time as float64 (transformed on
//            the way in when a similarity transform is given); a lane keeps its K1 best (distance, index) pairs sorted in registers.  K1 = 1 is
//            vghev_nearest, K1 = top_k + 1 the NEAREST mode of Z_n (rank 0 is dropped, as the source drops it).  Candidates arrive in index order and
//            only a strictly smaller distance moves ahead of an entry, so a tie keeps the lower index.
//   mean     one workgroup per head sums the head's distances in the fixed order include/vgh_eval.h states.
// Agreement counts are integers: a workgroup adds its lanes' counts in LDS and issues one integer atomic per workgroup.  There is no float atomic; every
// distance is float64 in the stated operation order with contraction off, so every output is bitwise reproducible and equal to a float64 restatement on
// the host (tests/mesh_metrics_ref.py).
#include <math.h>

#include "../../include/vgh_eval.h"
#include "companion_host.h"

#pragma clang fp contract(off)

namespace {

using namespace companion;
static_assert(VGHEV_OK == OK && VGHEV_ERR_INVALID == ERR_INVALID && VGHEV_ERR_HIP == ERR_HIP, "companion_host.h returns these codes");  // this library allocates nothing: its header has no NOMEM

constexpr int RANK_LANES = 256;   // points of one workgroup of rank_kernel
constexpr int RANK_TILE = 1024;   // column distances held in LDS at a time: 8 KB
constexpr int NEAR_LANES = 128;   // queries of one workgroup of the nearest kernels
constexpr int NEAR_TILE = 512;    // points held in LDS at a time as 3 x float64: 12 KB
constexpr int MEAN_LANES = 256;   // the fixed summation order of include/vgh_eval.h

// (dx * dx + dy * dy) + dz * dz, every operation rounded on its own
__device__ __forceinline__ double sqdist(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = __dsub_rn(ax, bx), dy = __dsub_rn(ay, by), dz = __dsub_rn(az, bz);
    return __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
}

// the lanes' counts -> one integer atomic of the workgroup
__device__ __forceinline__ void add_counts(int mine, int32_t* __restrict__ dst, int* s_count) {
    if (threadIdx.x == 0) *s_count = 0;
    __syncthreads();
    if (mine) atomicAdd(s_count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && *s_count) atomicAdd(dst, *s_count);
}

// ---- Z_n, REFERENCE mode ------------------------------------------------------------------------------------------------------------------------
// blockIdx.x = (head * top_k + (column - 1)) * tiles + tile
__global__ __launch_bounds__(RANK_LANES) void rank_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int N, int top_k, int tiles,
                                                           int32_t* __restrict__ agree) {
    __shared__ double s_d[RANK_TILE];
    __shared__ int s_count;
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const unsigned hc = blockIdx.x / (unsigned)tiles;
    const int col = (int)(hc % (unsigned)top_k) + 1;
    const size_t head = hc / (unsigned)top_k;
    const float* g = gt + head * (size_t)N * 3;
    const float* pr = pred + head * (size_t)N * 3;
    const double cx = g[3 * col], cy = g[3 * col + 1], cz = g[3 * col + 2];
    const int p = tile * RANK_LANES + (int)threadIdx.x;
    const bool live = p < N;
    const double dp = live ? sqdist(g[3 * (size_t)p], g[3 * (size_t)p + 1], g[3 * (size_t)p + 2], cx, cy, cz) : 0.0;
    int rank = 0;
    for (int base = 0; base < N; base += RANK_TILE) {
        const int m = min(RANK_TILE, N - base);
        __syncthreads();
        for (int k = (int)threadIdx.x; k < m; k += RANK_LANES) {
            const size_t q = (size_t)(base + k) * 3;
            s_d[k] = sqdist(g[q], g[q + 1], g[q + 2], cx, cy, cz);
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const double dq = s_d[k];
            rank += (dq < dp || (dq == dp && base + k < p)) ? 1 : 0;
        }
    }
    // rank <= N - 1 whatever the data: the point itself never counts
    int ok = 0;
    if (live) {
        const float gi = g[3 * (size_t)rank + 2], gp = g[3 * (size_t)p + 2], pi = pr[3 * (size_t)rank + 2], pp = pr[3 * (size_t)p + 2];
        ok = ((gi >= gp) == (pi >= pp)) ? 1 : 0;
    }
    add_counts(ok, agree + head, &s_count);
}

// ---- the streaming search ---------------------------------------------------------------------------------------------------------------------------
// The K1 best of a head's points for the lane's query (qx, qy, qz), sorted by (distance, index); unfilled entries keep index -1.  All lanes of the
// workgroup call it together.
template <int K1>
__device__ __forceinline__ void search(const float* __restrict__ pts, int P, const double* __restrict__ T, double s, double qx, double qy, double qz,
                                       double* s_x, double* s_y, double* s_z, double (&bd)[K1], int (&bi)[K1]) {
#pragma unroll
    for (int k = 0; k < K1; ++k) {
        bd[k] = INFINITY;
        bi[k] = -1;
    }
    double t[12];
    if (T) {
#pragma unroll
        for (int k = 0; k < 12; ++k) t[k] = T[k];
    }
    for (int base = 0; base < P; base += NEAR_TILE) {
        const int m = min(NEAR_TILE, P - base);
        __syncthreads();
        for (int k = (int)threadIdx.x; k < m; k += NEAR_LANES) {
            const size_t q = (size_t)(base + k) * 3;
            const double v0 = pts[q], v1 = pts[q + 1], v2 = pts[q + 2];
            if (T) {
                s_x[k] = __dadd_rn(__dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn(v0, t[0]), __dmul_rn(v1, t[1])), __dmul_rn(v2, t[2])), s), t[3]);
                s_y[k] = __dadd_rn(__dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn(v0, t[4]), __dmul_rn(v1, t[5])), __dmul_rn(v2, t[6])), s), t[7]);
                s_z[k] = __dadd_rn(__dmul_rn(__dadd_rn(__dadd_rn(__dmul_rn(v0, t[8]), __dmul_rn(v1, t[9])), __dmul_rn(v2, t[10])), s), t[11]);
            } else {
                s_x[k] = v0;
                s_y[k] = v1;
                s_z[k] = v2;
            }
        }
        __syncthreads();
        for (int k = 0; k < m; ++k) {
            const double d = sqdist(qx, qy, qz, s_x[k], s_y[k], s_z[k]);
            if (d < bd[K1 - 1]) {  // candidates come in index order: an equal distance never displaces an entry
                bd[K1 - 1] = d;
                bi[K1 - 1] = base + k;
#pragma unroll
                for (int r = K1 - 1; r > 0; --r) {
                    if (bd[r] < bd[r - 1]) {
                        const double td = bd[r];
                        bd[r] = bd[r - 1];
                        bd[r - 1] = td;
                        const int ti = bi[r];
                        bi[r] = bi[r - 1];
                        bi[r - 1] = ti;
                    }
                }
            }
        }
    }
}

// ---- Z_n, NEAREST mode: blockIdx.x = head * tiles + tile ------------------------------------------------------------------------------------------------
template <int K1>
__global__ __launch_bounds__(NEAR_LANES) void z_nearest_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int N, int tiles,
                                                                int32_t* __restrict__ agree) {
    __shared__ double s_x[NEAR_TILE], s_y[NEAR_TILE], s_z[NEAR_TILE];
    __shared__ int s_count;
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const size_t head = blockIdx.x / (unsigned)tiles;
    const float* g = gt + head * (size_t)N * 3;
    const float* pr = pred + head * (size_t)N * 3;
    const int i = tile * NEAR_LANES + (int)threadIdx.x;
    const bool live = i < N;
    const size_t at = (size_t)(live ? i : 0) * 3;
    const float gz = g[at + 2], pz = pr[at + 2];
    double bd[K1];
    int bi[K1];
    search<K1>(g, N, nullptr, 1.0, (double)g[at], (double)g[at + 1], (double)gz, s_x, s_y, s_z, bd, bi);
    int ok = 0;
    if (live) {
#pragma unroll
        for (int r = 1; r < K1; ++r) {
            const int p = bi[r];
            if (p >= 0) ok += ((gz >= g[3 * (size_t)p + 2]) == (pz >= pr[3 * (size_t)p + 2])) ? 1 : 0;
        }
    }
    add_counts(ok, agree + head, &s_count);
}

// ---- vghev_nearest: blockIdx.x = head * tiles + tile --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NEAR_LANES) void nearest_kernel(const float* __restrict__ query, const double* __restrict__ query_scale,
                                                              const float* __restrict__ points, const double* __restrict__ transform,
                                                              const double* __restrict__ point_scale, int M, int P, int tiles, double* __restrict__ sqd,
                                                              int32_t* __restrict__ index) {
    __shared__ double s_x[NEAR_TILE], s_y[NEAR_TILE], s_z[NEAR_TILE];
    const int tile = (int)(blockIdx.x % (unsigned)tiles);
    const size_t head = blockIdx.x / (unsigned)tiles;
    const int i = tile * NEAR_LANES + (int)threadIdx.x;
    const bool live = i < M;
    const size_t at = (head * (size_t)M + (size_t)(live ? i : 0)) * 3;
    double qx = query[at], qy = query[at + 1], qz = query[at + 2];
    if (query_scale) {
        const double qs = query_scale[head];
        qx = __dmul_rn(qx, qs);
        qy = __dmul_rn(qy, qs);
        qz = __dmul_rn(qz, qs);
    }
    double bd[1];
    int bi[1];
    search<1>(points + head * (size_t)P * 3, P, transform ? transform + head * 12 : nullptr, (transform && point_scale) ? point_scale[head] : 1.0, qx, qy, qz,
              s_x, s_y, s_z, bd, bi);
    if (live) {
        sqd[head * (size_t)M + i] = bd[0];
        index[head * (size_t)M + i] = bi[0];
    }
}

// ---- the mean of a head's distances, in a fixed order ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MEAN_LANES) void mean_kernel(const double* __restrict__ sqd, int M, double* __restrict__ mean) {
    __shared__ double s_part[MEAN_LANES];
    const double* row = sqd + (size_t)blockIdx.x * M;
    double acc = 0.0;
    for (int k = (int)threadIdx.x; k < M; k += MEAN_LANES) acc = __dadd_rn(acc, row[k]);
    s_part[threadIdx.x] = acc;
    __syncthreads();
    for (int h = MEAN_LANES / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_part[threadIdx.x] = __dadd_rn(s_part[threadIdx.x], s_part[threadIdx.x + h]);
        __syncthreads();
    }
    if (threadIdx.x == 0) mean[blockIdx.x] = s_part[0] / (double)M;
}

template <int K1>
void launch_z_nearest(unsigned grid, hipStream_t st, const vghev_z_order_job& j, int tiles) {
    hipLaunchKernelGGL(z_nearest_kernel<K1>, dim3(grid), dim3(NEAR_LANES), 0, st, j.pred_dev, j.gt_dev, j.n_points, tiles, j.agree_dev);
}

}  // namespace

extern "C" VGHEV_API const char* vghev_version(void) { return "vgheval 1 (gfx950)"; }

extern "C" VGHEV_API const char* vghev_last_error(void) { return last_error(); }

extern "C" VGHEV_API int vghev_z_order(const vghev_z_order_job* job, void* stream) {
    CH_REQUIRE(job != nullptr, "z_order: job is NULL");
    const vghev_z_order_job& j = *job;
    CH_REQUIRE(j.n_heads >= 0 && j.n_heads <= VGHEV_MAX_HEADS, "z_order: n_heads = %d outside 0 .. %d", j.n_heads, VGHEV_MAX_HEADS);
    CH_REQUIRE(j.top_k >= 1 && j.top_k <= VGHEV_MAX_TOP_K, "z_order: top_k = %d outside 1 .. %d", j.top_k, VGHEV_MAX_TOP_K);
    CH_REQUIRE(j.n_points >= j.top_k + 1 && j.n_points <= VGHEV_MAX_POINTS, "z_order: n_points = %d outside top_k + 1 = %d .. %d", j.n_points, j.top_k + 1,
               VGHEV_MAX_POINTS);
    CH_REQUIRE(j.mode == VGHEV_NEIGHBOURS_REFERENCE || j.mode == VGHEV_NEIGHBOURS_NEAREST, "z_order: unknown mode %d", j.mode);
    if (j.n_heads == 0) return OK;
    CH_REQUIRE(j.pred_dev && j.gt_dev && j.agree_dev, "z_order: pred_dev, gt_dev and agree_dev must not be NULL");
    const bool reference = j.mode == VGHEV_NEIGHBOURS_REFERENCE;
    const int tiles = (j.n_points + (reference ? RANK_LANES : NEAR_LANES) - 1) / (reference ? RANK_LANES : NEAR_LANES);
    const uint64_t groups = (uint64_t)j.n_heads * (uint64_t)tiles * (uint64_t)(reference ? j.top_k : 1);
    CH_REQUIRE(groups <= 0x7fffffffull, "z_order: %d heads of %d points need %llu workgroups, more than one launch holds", j.n_heads, j.n_points,
               (unsigned long long)groups);
    hipStream_t st = (hipStream_t)stream;
    CH_HIP(hipMemsetAsync(j.agree_dev, 0, (size_t)j.n_heads * sizeof(int32_t), st));
    if (reference) {
        hipLaunchKernelGGL(rank_kernel, dim3((unsigned)groups), dim3(RANK_LANES), 0, st, j.pred_dev, j.gt_dev, j.n_points, j.top_k, tiles, j.agree_dev);
    } else {
        switch (j.top_k) {
#define EV_CASE(K)                                         \
    case K:                                                \
        launch_z_nearest<K + 1>((unsigned)groups, st, j, tiles); \
        break;
            EV_CASE(1) EV_CASE(2) EV_CASE(3) EV_CASE(4) EV_CASE(5) EV_CASE(6) EV_CASE(7) EV_CASE(8)
            EV_CASE(9) EV_CASE(10) EV_CASE(11) EV_CASE(12) EV_CASE(13) EV_CASE(14) EV_CASE(15) EV_CASE(16)
#undef EV_CASE
        }
    }
    CH_HIP(hipGetLastError());
    return OK;
}

extern "C" VGHEV_API int vghev_nearest(const vghev_nearest_job* job, void* stream) {
    CH_REQUIRE(job != nullptr, "nearest: job is NULL");
    const vghev_nearest_job& j = *job;
    CH_REQUIRE(j.n_heads >= 0 && j.n_heads <= VGHEV_MAX_HEADS, "nearest: n_heads = %d outside 0 .. %d", j.n_heads, VGHEV_MAX_HEADS);
    CH_REQUIRE(j.n_queries >= 1 && j.n_queries <= VGHEV_MAX_POINTS, "nearest: n_queries = %d outside 1 .. %d", j.n_queries, VGHEV_MAX_POINTS);
    CH_REQUIRE(j.n_points >= 1 && j.n_points <= VGHEV_MAX_POINTS, "nearest: n_points = %d outside 1 .. %d", j.n_points, VGHEV_MAX_POINTS);
    CH_REQUIRE(j.reserved == 0, "nearest: reserved must be 0");
    CH_REQUIRE(j.transform_dev || !j.point_scale_dev, "nearest: point_scale_dev needs transform_dev");
    if (j.n_heads == 0) return OK;
    CH_REQUIRE(j.query_dev && j.points_dev && j.sqdist_dev && j.index_dev, "nearest: query_dev, points_dev, sqdist_dev and index_dev must not be NULL");
    const int tiles = (j.n_queries + NEAR_LANES - 1) / NEAR_LANES;
    const uint64_t groups = (uint64_t)j.n_heads * (uint64_t)tiles;
    CH_REQUIRE(groups <= 0x7fffffffull, "nearest: %d heads of %d queries need %llu workgroups, more than one launch holds", j.n_heads, j.n_queries,
               (unsigned long long)groups);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nearest_kernel, dim3((unsigned)groups), dim3(NEAR_LANES), 0, st, j.query_dev, j.query_scale_dev, j.points_dev, j.transform_dev,
                       j.point_scale_dev, j.n_queries, j.n_points, tiles, j.sqdist_dev, j.index_dev);
    if (j.mean_dev) hipLaunchKernelGGL(mean_kernel, dim3((unsigned)j.n_heads), dim3(MEAN_LANES), 0, st, (const double*)j.sqdist_dev, j.n_queries, j.mean_dev);
    CH_HIP(hipGetLastError());
    return OK;
}
