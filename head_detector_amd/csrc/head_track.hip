// libvghtrack.so (include/vgh_track.h): head tracking across the frames of a video.  The per-frame slabs of vgh_detect (up to 2 048 rows, live counts on the
// device) step a device-resident table of up to 2 048 tracks; the rule is stated once, in the header, and restated in NumPy by tests/head_track_ref.py.
//
//   assoc    ONE workgroup of 8 waves holds a frame's whole association in LDS: the predicted boxes of the slots, the image-coordinate boxes of the rows, the
//            taken flags and the picks.  Every thread owns the slots tid, tid + 512, ... and keeps their scalars in registers from the update to the store.
//              match   two stages of mutual-best rounds.  A wave takes a free slot, its lanes stride over the free rows of the stage's class, and a wave max
//                      of the 64-bit key (valid, iou bits, ~slot, ~row) is the slot's pick; the same with the roles swapped is a row's pick; mutual picks are
//                      matched; a round that matches nothing ends the stage.  A side looks again only if its pick was taken by someone else; the sides that look are
//                      listed first (one thread per side, an LDS counter), so a round costs what it has to do.  IoUs are recomputed from the boxes, never stored.  The key's order is the
//                      rule's total order, so the result is the greedy matching and does not depend on how the waves are scheduled.
//              update  the owner applies step 5 or 6 to its slots and frees what step 6 frees.
//              births  ballots of the free slots and of the unmatched HIGH rows; the k-th such row takes the k-th free slot (a rank and a select over 32
//                      words).
//              report  a ballot of the reported slots, the rank is the output row; the state, the outputs, the fill behind n_out and the four counters.
//   params   the 413 floats of every matched or born slot, one workgroup per slot over the chip: the smoothing, the copy into out_params and the zero
//            rows behind n_out.  What each slot needs comes from the two i32 per slot that assoc leaves in the workspace.
// Two launches per frame and one upload per call whatever the counts are.  Values are written with ordinary vector stores; integer atomics only (two LDS
// counters); every float operation in the stated order with contraction off.
#include <math.h>

#include <map>
#include <mutex>

#include "../../include/vgh_track.h"
#include "companion_host.h"

#pragma clang fp contract(off)

namespace {

using namespace companion;
static_assert(VGHT_OK == OK && VGHT_ERR_INVALID == ERR_INVALID && VGHT_ERR_HIP == ERR_HIP && VGHT_ERR_NOMEM == ERR_NOMEM, "companion_host.h returns these codes");

constexpr int WAVE = 64;
constexpr int LANES = 512;  // of the one workgroup of assoc_kernel: 8 waves, so that a thread's four slots stay in registers (no scratch)
constexpr int WAVES = LANES / WAVE;
constexpr int CAP = 2048;  // slots and rows held in LDS
constexpr int OWN = CAP / LANES;  // slots a thread owns
constexpr int WORDS = CAP / WAVE;  // ballot words of a compaction
constexpr int NP = VGHT_NUM_PARAMS;
constexpr int PARAM_LANES = 128;
constexpr int HIGH = 2, LOW = 1;
constexpr int LIVE = 1, FRESH = 2;  // s_flag: the slot is live; it had misses == 0 on entry
constexpr int PICK_UNKNOWN = -2;  // s_spick / s_rpick: not looked yet; -1 = looked and found no pair
constexpr int ACT_NONE = -1;  // workspace act[slot]: -1 nothing, r >= 0 matched with row r, -(r + 2) born from row r
static_assert(VGHT_MAX_TRACKS == CAP && VGHT_MAX_DETS == CAP && OWN * LANES == CAP, "assoc_kernel holds 2 048 slots and 2 048 rows in LDS");
static_assert(CAP <= 2048, "the key has 11 bits for a slot and 11 for a row");

__host__ __device__ inline size_t a16(size_t v) { return (v + 15) & ~(size_t)15; }

// the state as the header lays it out
struct StateAt {
    size_t id, hits, misses, age, det_row, score, box, vel, params, total;
    __host__ __device__ explicit StateAt(size_t M) {
        const size_t col = a16(4 * M);
        id = VGHT_STATE_HEADER_BYTES;
        hits = id + col;
        misses = hits + col;
        age = misses + col;
        det_row = age + col;
        score = det_row + col;
        box = score + col;
        vel = box + 16 * M;
        params = vel + 16 * M;
        total = params + a16(4 * (size_t)NP * M);
    }
};

struct Rule {
    int32_t keep_k, max_tracks, max_out, max_age, min_hits, report_misses;
    float S, high_thr, low_thr, match_thr, match_thr_low, box_gain, vel_gain;
};

struct FrameIO {  // one frame's rows of the job's arrays
    const float4* boxes;
    const float* scores;
    const int32_t* counts;
    const float* unpad;  // device copy of the frame's (pad_x, pad_y, scale)
    int32_t *n_out, *out_slot, *out_id, *out_det_row, *out_hits, *out_misses;
    float4* out_box;
    float* out_score;
    int32_t *det_id, *n_born, *n_freed, *n_dropped;
};

__device__ __forceinline__ float clip(float v, float S) { return fminf(fmaxf(v, 0.0f), S); }

__device__ __forceinline__ float box_area(const float4 b) { return fmaxf(0.0f, b.z - b.x) * fmaxf(0.0f, b.w - b.y); }

// a = the predicted box of a slot, b = a detection; the two kinds of entry of a round call these with the same arguments in the same places
__device__ __forceinline__ float inter_of(const float4 a, const float4 b) {
    const float w = fmaxf(0.0f, fminf(a.z, b.z) - fmaxf(a.x, b.x)), h = fmaxf(0.0f, fminf(a.w, b.w) - fmaxf(a.y, b.y));
    return w * h;
}

__device__ __forceinline__ float iou_of(const float4 a, const float4 b, const float inter) { return inter / ((box_area(a) + box_area(b)) - inter); }

// Does the pair pass `iou > thr`?  Boxes that do not overlap (inter == 0: the quotient is 0 or NaN) cannot pass a threshold >= 0, and most pairs of a frame
// are such: they leave before the areas and the division.  The value of every iou that is compared is the rule's, operation for operation.
__device__ __forceinline__ bool pair_passes(const float4 a, const float4 b, const float thr, float* iou) {
    const float inter = inter_of(a, b);
    if (!(inter > 0.0f) && thr >= 0.0f) return false;
    *iou = iou_of(a, b, inter);
    return *iou > thr;  // false for NaN
}

// larger key = earlier pair in (iou descending, slot ascending, row ascending); 0 = no pair.  An iou that passes a threshold test is not NaN, and it is never
// negative (inter <= either area, rounding is monotone), so its bit pattern orders like its value.
__device__ __forceinline__ uint64_t pair_key(float iou, int slot, int row) {
    return ((uint64_t)1 << 62) | ((uint64_t)__float_as_uint(iou) << 22) | ((uint64_t)(CAP - 1 - slot) << 11) | (uint64_t)(CAP - 1 - row);
}

__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
    for (int off = WAVE / 2; off; off >>= 1) {
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off), lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off);
        const uint64_t other = ((uint64_t)hi << 32) | lo;
        v = other > v ? other : v;
    }
    return v;
}

// set bits of `words` below position i
__device__ __forceinline__ int rank_of(const uint64_t* words, int i) {
    int n = 0;
#pragma unroll 1
    for (int w = 0; w < (i >> 6); ++w) n += __popcll(words[w]);
    return n + __popcll(words[i >> 6] & (((uint64_t)1 << (i & 63)) - 1));
}

// position of the k-th set bit (k from 0) of `words`; the caller knows there is one
__device__ __forceinline__ int select_of(const uint64_t* words, int k) {
    int w = 0;
#pragma unroll 1
    for (; w < WORDS - 1; ++w) {
        const int n = __popcll(words[w]);
        if (k < n) break;
        k -= n;
    }
    uint64_t m = words[w];
#pragma unroll 1
    for (; k > 0; --k) m &= m - 1;
    return w * WAVE + __ffsll((unsigned long long)m) - 1;
}

__device__ __forceinline__ float smooth(float from, float to, float gain) { return gain == 1.0f ? to : from + gain * (to - from); }

// ---- assoc ----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LANES) void assoc_kernel(const Rule R, const FrameIO io, uint8_t* __restrict__ state, int32_t* __restrict__ act, int32_t* __restrict__ out_pos) {
    __shared__ float4 s_pred[CAP];  // slot: the predicted box
    __shared__ float4 s_det[CAP];  // row: the detection in image coordinates
    __shared__ int32_t s_match[CAP];  // slot: its row, -1 = none
    __shared__ int32_t s_id[CAP];  // slot: id after step 6, then after step 7
    __shared__ int32_t s_rid[CAP];  // row: the id it was given
    __shared__ int16_t s_spick[CAP], s_rpick[CAP];
    __shared__ uint8_t s_cls[CAP], s_rtaken[CAP], s_flag[CAP];
    __shared__ uint64_t s_free[WORDS], s_cand[WORDS], s_rep[WORDS];
    __shared__ int16_t s_todo[2 * CAP];  // the sides that look in this round: a slot s, or CAP + a row
    __shared__ int32_t s_todo_n;
    __shared__ int32_t s_freed;

    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const int M = R.max_tracks, K = R.keep_k;
    const int n_det = min(max(*io.counts, 0), K);
    int32_t* hdr = (int32_t*)state;
    const int next_id0 = hdr[0], frame0 = hdr[1];  // rewritten by thread 0 behind the last barrier
    const StateAt at((size_t)M);
    int32_t* g_id = (int32_t*)(state + at.id);
    int32_t* g_hits = (int32_t*)(state + at.hits);
    int32_t* g_misses = (int32_t*)(state + at.misses);
    int32_t* g_age = (int32_t*)(state + at.age);
    int32_t* g_row = (int32_t*)(state + at.det_row);
    float* g_score = (float*)(state + at.score);
    float4* g_box = (float4*)(state + at.box);
    float4* g_vel = (float4*)(state + at.vel);

    // ---- load: steps 1 and 2.  Only the predicted box and the flags go to LDS here; the owner reads its slots' scalars again after the match, so that nothing
    // but the match's own values is live across its loops
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int s = tid + j * LANES;
        if (s >= M) continue;
        float4 p = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        uint8_t flag = 0;
        if (g_id[s] >= 0) {
            const float4 b = g_box[s], v = g_vel[s];
            p = make_float4(b.x + v.x, b.y + v.y, b.z + v.z, b.w + v.w);
            flag = (uint8_t)(LIVE | (g_misses[s] == 0 ? FRESH : 0));
        }
        s_pred[s] = p;
        s_flag[s] = flag;
        s_match[s] = -1;
    }
    {
        const float pad_x = io.unpad[0], pad_y = io.unpad[1], scale = io.unpad[2];
        for (int r = tid; r < K; r += LANES) {
            float4 d = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            uint8_t cls = 0;
            if (r < n_det) {
                const float4 b = io.boxes[r];
                d = make_float4((clip(b.x, R.S) - pad_x) / scale, (clip(b.y, R.S) - pad_y) / scale, (clip(b.z, R.S) - pad_x) / scale, (clip(b.w, R.S) - pad_y) / scale);
                const float sc = io.scores[r];
                cls = sc >= R.high_thr ? HIGH : sc >= R.low_thr ? LOW : 0;  // NaN: neither
            }
            s_det[r] = d;
            s_cls[r] = cls;
            s_rtaken[r] = 0;
            s_rid[r] = -1;
        }
    }
    if (tid == 0) s_freed = 0;
    __syncthreads();

    // ---- match: step 4
    for (int stage = 0; stage < 2; ++stage) {
        const int want = stage == 0 ? HIGH : LOW, need = stage == 0 ? LIVE : LIVE | FRESH;
        const float thr = stage == 0 ? R.match_thr : R.match_thr_low;
        // A pick outlives its round: the free sets only shrink, so a pick whose other side is still free is still the best, and a side that found no pair
        // never finds one.  Only a side whose pick was taken by someone else looks again.
        for (int s = tid; s < M; s += LANES) s_spick[s] = PICK_UNKNOWN;
        for (int r = tid; r < n_det; r += LANES) s_rpick[r] = PICK_UNKNOWN;
        __syncthreads();
        for (;;) {
            // who looks: one thread per side appends it to the list.  The order of the list is whatever the atomic gives; every entry is worked on its own, so
            // the picks do not depend on it
            if (tid == 0) s_todo_n = 0;
            __syncthreads();
            for (int s = tid; s < M; s += LANES) {
                if ((s_flag[s] & need) != need || s_match[s] >= 0) continue;
                const int had = s_spick[s];
                if (had == -1 || (had >= 0 && !s_rtaken[had])) continue;
                s_todo[atomicAdd(&s_todo_n, 1)] = (int16_t)s;
            }
            for (int r = tid; r < n_det; r += LANES) {
                if (s_cls[r] != want || s_rtaken[r]) continue;
                const int had = s_rpick[r];
                if (had == -1 || (had >= 0 && s_match[had] < 0)) continue;
                s_todo[atomicAdd(&s_todo_n, 1)] = (int16_t)(CAP + r);
            }
            __syncthreads();
            const int n_todo = s_todo_n;  // <= M + n_det <= 2 CAP
            for (int i = wave; i < n_todo; i += WAVES) {  // wave-uniform: an entry per wave
                const int item = s_todo[i];
                uint64_t best = 0;
                if (item < CAP) {  // a slot looks over the free rows of the class
                    const int s = item;
                    const float4 a = s_pred[s];
#pragma unroll 2
                    for (int r = lane; r < n_det; r += WAVE) {
                        if (s_cls[r] != want || s_rtaken[r]) continue;
                        float iou;
                        if (pair_passes(a, s_det[r], thr, &iou)) {
                            const uint64_t key = pair_key(iou, s, r);
                            best = key > best ? key : best;
                        }
                    }
                    best = wave_max(best);
                    if (lane == 0) s_spick[s] = best ? (int16_t)(CAP - 1 - (int)(best & (CAP - 1))) : (int16_t)-1;
                } else {  // a row looks over the free slots of the stage
                    const int r = item - CAP;
                    const float4 b = s_det[r];
#pragma unroll 2
                    for (int s = lane; s < M; s += WAVE) {
                        if ((s_flag[s] & need) != need || s_match[s] >= 0) continue;
                        float iou;
                        if (pair_passes(s_pred[s], b, thr, &iou)) {
                            const uint64_t key = pair_key(iou, s, r);
                            best = key > best ? key : best;
                        }
                    }
                    best = wave_max(best);
                    if (lane == 0) s_rpick[r] = best ? (int16_t)(CAP - 1 - (int)((best >> 11) & (CAP - 1))) : (int16_t)-1;
                }
            }
            __syncthreads();
            int any = 0;
            for (int s = tid; s < M; s += LANES) {
                if ((s_flag[s] & need) != need || s_match[s] >= 0) continue;
                const int r = s_spick[s];
                if (r >= 0 && s_rpick[r] == s) {  // a picked row is free and of this class, so its pick is current; one slot per row
                    s_match[s] = r;
                    s_rtaken[r] = 1;
                    any = 1;
                }
            }
            if (!__syncthreads_or(any)) break;
        }
    }

    // ---- update: steps 5 and 6
    int o_id[OWN], o_hits[OWN], o_misses[OWN], o_age[OWN], o_row[OWN], o_act[OWN];
    float o_score[OWN];
    float4 o_box[OWN], o_vel[OWN];
    bool o_was[OWN], o_rep[OWN];
    int freed = 0;
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int s = tid + j * LANES;
        o_id[j] = -1;
        o_hits[j] = o_misses[j] = o_age[j] = 0;
        o_row[j] = -1;
        o_score[j] = 0.0f;
        o_box[j] = o_vel[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        o_was[j] = false;
        if (s >= M) continue;
        if (s_flag[s] & LIVE) {
            o_id[j] = g_id[s];
            o_hits[j] = g_hits[s];
            o_misses[j] = g_misses[s];
            o_age[j] = g_age[s];
            o_score[j] = g_score[s];
            o_box[j] = g_box[s];
            o_vel[j] = g_vel[s];
            o_was[j] = true;
            const float4 p = s_pred[s];
            const int r = s_match[s];
            if (r >= 0) {
                const float4 d = s_det[r], b = o_box[j], v = o_vel[j];
                const float4 nb = make_float4(smooth(p.x, d.x, R.box_gain), smooth(p.y, d.y, R.box_gain), smooth(p.z, d.z, R.box_gain), smooth(p.w, d.w, R.box_gain));
                o_vel[j] = make_float4(smooth(v.x, nb.x - b.x, R.vel_gain), smooth(v.y, nb.y - b.y, R.vel_gain), smooth(v.z, nb.z - b.z, R.vel_gain),
                                       smooth(v.w, nb.w - b.w, R.vel_gain));
                o_box[j] = nb;
                o_hits[j] += 1;
                o_misses[j] = 0;
                o_score[j] = io.scores[r];
                o_row[j] = r;
                s_rid[r] = o_id[j];
            } else {
                o_box[j] = p;
                o_misses[j] += 1;
                o_row[j] = -1;
                if (o_hits[j] < R.min_hits || o_misses[j] > R.max_age) {  // freed: what vght_state_init leaves, but for the params
                    o_id[j] = -1;
                    o_hits[j] = o_misses[j] = o_age[j] = 0;
                    o_score[j] = 0.0f;
                    o_box[j] = o_vel[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    ++freed;
                }
            }
        }
        s_id[s] = o_id[j];
    }
    if (freed) atomicAdd(&s_freed, freed);
    __syncthreads();

    // ---- births: step 7
    for (int base = 0; base < CAP; base += LANES) {  // every thread, every pass: whole waves vote
        const int i = base + tid;
        const unsigned long long fm = __ballot(i < M && s_id[i] < 0);
        const unsigned long long cm = __ballot(i < n_det && s_cls[i] == HIGH && !s_rtaken[i]);
        if (lane == 0) {
            s_free[i >> 6] = fm;
            s_cand[i >> 6] = cm;
        }
    }
    __syncthreads();
    int n_free = 0, n_cand = 0;
    for (int w = 0; w < WORDS; ++w) {
        n_free += __popcll(s_free[w]);
        n_cand += __popcll(s_cand[w]);
    }
    const int n_born = min(n_free, n_cand);
    for (int r = tid; r < n_det; r += LANES) {
        if (s_cls[r] != HIGH || s_rtaken[r]) continue;
        const int k = rank_of(s_cand, r);
        if (k >= n_free) continue;  // dropped
        const int s = select_of(s_free, k);  // < M: only slots below M vote
        s_match[s] = r;
        s_id[s] = next_id0 + k;
        s_rid[r] = next_id0 + k;
    }
    __syncthreads();

    // ---- report: step 8
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int s = tid + j * LANES;
        o_act[j] = ACT_NONE;
        if (s < M) {
            if (o_id[j] < 0 && s_id[s] >= 0) {  // born here
                const int r = s_match[s];
                o_id[j] = s_id[s];
                o_hits[j] = 1;
                o_misses[j] = o_age[j] = 0;
                o_row[j] = r;
                o_score[j] = io.scores[r];
                o_box[j] = s_det[r];
                o_vel[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                o_act[j] = -(r + 2);
            } else if (o_id[j] >= 0 && o_row[j] >= 0) {
                o_act[j] = o_row[j];
            }
            if (o_id[j] >= 0) o_age[j] += 1;
        }
        o_rep[j] = s < M && o_id[j] >= 0 && o_hits[j] >= R.min_hits && o_misses[j] <= R.report_misses;
        const unsigned long long m = __ballot(o_rep[j]);
        if (lane == 0) s_rep[s >> 6] = m;
    }
    __syncthreads();
    int n_rep = 0;
    for (int w = 0; w < WORDS; ++w) n_rep += __popcll(s_rep[w]);
    const int n_out = min(n_rep, R.max_out);
#pragma unroll
    for (int j = 0; j < OWN; ++j) {
        const int s = tid + j * LANES;
        if (s >= M) continue;
        int pos = o_rep[j] ? rank_of(s_rep, s) : -1;
        if (pos >= R.max_out) pos = -1;
        if (pos >= 0) {
            io.out_slot[pos] = s;
            io.out_id[pos] = o_id[j];
            io.out_det_row[pos] = o_row[j];
            io.out_hits[pos] = o_hits[j];
            io.out_misses[pos] = o_misses[j];
            io.out_box[pos] = o_box[j];
            io.out_score[pos] = o_score[j];
        }
        act[s] = o_act[j];
        out_pos[s] = pos;
        if (o_was[j] || o_id[j] >= 0) {  // a slot that was free and stays free holds what it held
            g_id[s] = o_id[j];
            g_hits[s] = o_hits[j];
            g_misses[s] = o_misses[j];
            g_age[s] = o_age[j];
            g_row[s] = o_id[j] >= 0 ? o_row[j] : -1;
            g_score[s] = o_score[j];
            g_box[s] = o_box[j];
            g_vel[s] = o_vel[j];
        }
    }
    for (int p = n_out + tid; p < R.max_out; p += LANES) {
        io.out_slot[p] = -1;
        io.out_id[p] = -1;
        io.out_det_row[p] = -1;
        io.out_hits[p] = 0;
        io.out_misses[p] = 0;
        io.out_box[p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        io.out_score[p] = 0.0f;
    }
    if (io.det_id)
        for (int r = tid; r < K; r += LANES) io.det_id[r] = s_rid[r];
    if (tid == 0) {
        hdr[0] = next_id0 + n_born;
        hdr[1] = frame0 + 1;
        *io.n_out = n_out;
        *io.n_born = n_born;
        *io.n_freed = s_freed;
        *io.n_dropped = n_cand - n_born;
    }
}

// ---- params ---------------------------------------------------------------------------------------------------------------------------------------
// block b: slot b (if b < M) and output row b (if b < max_out and out_params)
__global__ __launch_bounds__(PARAM_LANES) void params_kernel(int M, int max_out, float gain, const float* __restrict__ flame, const int32_t* __restrict__ act,
                                                             const int32_t* __restrict__ out_pos, const int32_t* __restrict__ n_out, float* __restrict__ sparams,
                                                             float* __restrict__ out_params) {
    const int b = blockIdx.x;
    if (b < M) {
        const int a = act[b], pos = out_params ? out_pos[b] : -1;
        if (a != ACT_NONE || pos >= 0) {
            float* q_row = sparams + (size_t)b * NP;
            const float* x_row = flame + (size_t)(a >= 0 ? a : a <= -2 ? -(a + 2) : 0) * NP;
            for (int e = threadIdx.x; e < NP; e += PARAM_LANES) {
                float v = q_row[e];
                if (a >= 0) {
                    const float x = x_row[e];
                    if (isfinite(x)) v = smooth(v, x, gain);
                } else if (a <= -2) {
                    const float x = x_row[e];
                    v = isfinite(x) ? x : 0.0f;
                }
                if (a != ACT_NONE) q_row[e] = v;
                if (pos >= 0) out_params[(size_t)pos * NP + e] = v;
            }
        }
    }
    if (out_params && b < max_out && b >= *n_out)
        for (int e = threadIdx.x; e < NP; e += PARAM_LANES) out_params[(size_t)b * NP + e] = 0.0f;
}

std::mutex g_mutex;
std::map<int, Staging> g_staging;

bool sizes_ok(int32_t max_tracks) { return max_tracks >= 1 && max_tracks <= VGHT_MAX_TRACKS; }

}  // namespace

extern "C" VGHT_API const char* vght_version(void) { return "vghtrack 1 (gfx950)"; }

extern "C" VGHT_API const char* vght_last_error(void) { return last_error(); }

extern "C" VGHT_API int64_t vght_state_bytes(int32_t max_tracks) { return sizes_ok(max_tracks) ? (int64_t)StateAt((size_t)max_tracks).total : 0; }

extern "C" VGHT_API int64_t vght_workspace_bytes(int32_t max_tracks, int32_t keep_k) {
    if (!sizes_ok(max_tracks) || keep_k < 1 || keep_k > VGHT_MAX_DETS) return 0;
    return (int64_t)(2 * a16(4 * (size_t)max_tracks));
}

extern "C" VGHT_API int vght_state_init(void* state_dev, int32_t max_tracks, void* stream) {
    CH_REQUIRE(state_dev, "state_init: null state");
    CH_REQUIRE(((uintptr_t)state_dev & 15) == 0, "state_init: the state is not 16-byte aligned");
    CH_REQUIRE(sizes_ok(max_tracks), "state_init: max_tracks %d outside 1 .. %d", max_tracks, VGHT_MAX_TRACKS);
    const StateAt at((size_t)max_tracks);
    uint8_t* base = (uint8_t*)state_dev;
    hipStream_t st = (hipStream_t)stream;
    Queue q;
    Staging none;
    CH_QUEUE(q, hipMemsetAsync(base, 0, at.total, st));
    CH_QUEUE(q, hipMemsetAsync(base + at.id, 0xff, 4 * (size_t)max_tracks, st));
    CH_QUEUE(q, hipMemsetAsync(base + at.det_row, 0xff, 4 * (size_t)max_tracks, st));
    return finish(q, none, false, st, "state_init");
}

extern "C" VGHT_API int vght_track_frames(const vght_track_job* job, void* state_dev, void* workspace_dev, void* stream) {
    CH_REQUIRE(job, "track_frames: null job");
    const vght_track_job& j = *job;
    // everything is checked before anything is allocated, written or queued
    CH_REQUIRE(j.n_frames >= 1 && j.n_frames <= VGHT_MAX_FRAMES, "track_frames: n_frames %d outside 1 .. %d", j.n_frames, VGHT_MAX_FRAMES);
    CH_REQUIRE(j.keep_k >= 1 && j.keep_k <= VGHT_MAX_DETS, "track_frames: keep_k %d outside 1 .. %d", j.keep_k, VGHT_MAX_DETS);
    CH_REQUIRE(sizes_ok(j.max_tracks), "track_frames: max_tracks %d outside 1 .. %d", j.max_tracks, VGHT_MAX_TRACKS);
    CH_REQUIRE(j.image_size >= 1, "track_frames: image_size %d < 1", j.image_size);
    CH_REQUIRE(j.max_out >= 1 && j.max_out <= VGHT_MAX_TRACKS, "track_frames: max_out %d outside 1 .. %d", j.max_out, VGHT_MAX_TRACKS);
    CH_REQUIRE(j.max_age >= 0, "track_frames: max_age %d < 0", j.max_age);
    CH_REQUIRE(j.min_hits >= 1, "track_frames: min_hits %d < 1", j.min_hits);
    CH_REQUIRE(j.report_misses >= 0, "track_frames: report_misses %d < 0", j.report_misses);
    CH_REQUIRE(!isnan(j.high_thr), "track_frames: high_thr is NaN");
    CH_REQUIRE(!isnan(j.low_thr), "track_frames: low_thr is NaN");
    CH_REQUIRE(!isnan(j.match_thr), "track_frames: match_thr is NaN");
    CH_REQUIRE(!isnan(j.match_thr_low), "track_frames: match_thr_low is NaN");
    CH_REQUIRE(isfinite(j.box_gain), "track_frames: box_gain %g is not finite", (double)j.box_gain);
    CH_REQUIRE(isfinite(j.vel_gain), "track_frames: vel_gain %g is not finite", (double)j.vel_gain);
    CH_REQUIRE(isfinite(j.param_gain), "track_frames: param_gain %g is not finite", (double)j.param_gain);
    CH_REQUIRE(j.boxes_dev, "track_frames: null boxes_dev");
    CH_REQUIRE(j.scores_dev, "track_frames: null scores_dev");
    CH_REQUIRE(j.flame_dev, "track_frames: null flame_dev");
    CH_REQUIRE(j.counts_dev, "track_frames: null counts_dev");
    CH_REQUIRE(j.unpad, "track_frames: null unpad");
    CH_REQUIRE(j.n_out_dev, "track_frames: null n_out_dev");
    CH_REQUIRE(j.out_slot_dev, "track_frames: null out_slot_dev");
    CH_REQUIRE(j.out_id_dev, "track_frames: null out_id_dev");
    CH_REQUIRE(j.out_det_row_dev, "track_frames: null out_det_row_dev");
    CH_REQUIRE(j.out_hits_dev, "track_frames: null out_hits_dev");
    CH_REQUIRE(j.out_misses_dev, "track_frames: null out_misses_dev");
    CH_REQUIRE(j.out_box_dev, "track_frames: null out_box_dev");
    CH_REQUIRE(j.out_score_dev, "track_frames: null out_score_dev");
    CH_REQUIRE(j.n_born_dev, "track_frames: null n_born_dev");
    CH_REQUIRE(j.n_freed_dev, "track_frames: null n_freed_dev");
    CH_REQUIRE(j.n_dropped_dev, "track_frames: null n_dropped_dev");
    CH_REQUIRE(state_dev, "track_frames: null state");
    CH_REQUIRE(workspace_dev, "track_frames: null workspace");
    CH_REQUIRE(((uintptr_t)state_dev & 15) == 0, "track_frames: the state is not 16-byte aligned");
    CH_REQUIRE(((uintptr_t)workspace_dev & 15) == 0, "track_frames: the workspace is not 16-byte aligned");
    CH_REQUIRE(((uintptr_t)j.boxes_dev & 15) == 0 && ((uintptr_t)j.out_box_dev & 15) == 0, "track_frames: boxes_dev / out_box_dev are not 16-byte aligned");
    const int B = j.n_frames, M = j.max_tracks, K = j.keep_k, O = j.max_out;
    for (int f = 0; f < B; ++f) {
        const float* u = j.unpad + 3 * f;
        CH_REQUIRE(isfinite(u[0]) && isfinite(u[1]) && isfinite(u[2]) && u[2] > 0.0f, "track_frames: frame %d: unpad (%g, %g, %g) is not finite with a positive scale", f,
                   (double)u[0], (double)u[1], (double)u[2]);
    }
    hipStream_t st = (hipStream_t)stream;
    int device = 0;
    CH_HIP(hipGetDevice(&device));
    std::lock_guard<std::mutex> lock(g_mutex);
    Staging& s = g_staging[device];
    const size_t total = (size_t)B * 3 * sizeof(float);
    if (int rc = reserve(s, total, "track_frames")) return rc;  // also waits for this device's previous call
    for (int i = 0; i < 3 * B; ++i) ((float*)s.host)[i] = j.unpad[i];
    // from here on work is queued (companion_host.h, queue-then-record)
    const Rule R{K, M, O, j.max_age, j.min_hits, j.report_misses, (float)j.image_size, j.high_thr, j.low_thr, j.match_thr, j.match_thr_low, j.box_gain, j.vel_gain};
    uint8_t* state = (uint8_t*)state_dev;
    int32_t* act = (int32_t*)workspace_dev;
    int32_t* out_pos = (int32_t*)((uint8_t*)workspace_dev + a16(4 * (size_t)M));
    float* sparams = (float*)(state + StateAt((size_t)M).params);
    const unsigned param_blocks = (unsigned)(j.out_params_dev && O > M ? O : M);
    Queue q;
    CH_QUEUE(q, hipMemcpyAsync(s.dev, s.host, total, hipMemcpyHostToDevice, st));  // first: whatever follows, the event covers the staging block
    for (int f = 0; f < B && q.ok(); ++f) {
        const size_t o = (size_t)f * O, k = (size_t)f * K;
        const FrameIO io{(const float4*)j.boxes_dev + k, j.scores_dev + k, j.counts_dev + f, (const float*)s.dev + 3 * f, j.n_out_dev + f, j.out_slot_dev + o,
                         j.out_id_dev + o, j.out_det_row_dev + o, j.out_hits_dev + o, j.out_misses_dev + o, (float4*)j.out_box_dev + o, j.out_score_dev + o,
                         j.det_id_dev ? j.det_id_dev + k : nullptr, j.n_born_dev + f, j.n_freed_dev + f, j.n_dropped_dev + f};
        hipLaunchKernelGGL(assoc_kernel, dim3(1), dim3(LANES), 0, st, R, io, state, act, out_pos);
        hipLaunchKernelGGL(params_kernel, dim3(param_blocks), dim3(PARAM_LANES), 0, st, M, O, j.param_gain, j.flame_dev + k * NP, (const int32_t*)act, (const int32_t*)out_pos,
                           (const int32_t*)(j.n_out_dev + f), sparams, j.out_params_dev ? j.out_params_dev + o * NP : nullptr);
        CH_QUEUE(q, hipGetLastError());
    }
    return finish(q, s, true, st, "track_frames");
}
