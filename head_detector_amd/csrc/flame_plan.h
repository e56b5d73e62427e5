// Which kernels a FLAME decode runs.  Every vertex kernel of flame.hip produces the same bits, so this is a pure speed choice -- and a pure function: plain
// integers and booleans in, a FlamePlan out, no HIP in sight.  run_decode_on (flame.hip) fills the arguments, asks flame_plan, and switches over the answer;
// tests/flame_plan_host.hip pins the table at every threshold.  The measured numbers stand next to the conditions they justify.
#pragma once

constexpr int kLdsMinHeads = 1024;  // from here on: LDS-staged tiles with 128-head blocks
constexpr int kC3MaxHeads = 2048;   // ... component-split tiles up to here (r04; automatic mode, direct batches)
constexpr int kLdsMidHeads = 256;   // ... 64-head blocks (r02: the register-fed kernel ran n = 256 .. 1024 at 0.22 - 0.35 of the fp32 roof)

// One line per vertex-kernel instantiation the choice can reach: X(plan value, the launch that run_decode_on's switch makes for it).
#define FLAME_VERTEX_KERNELS(X)                                                                                               \
    X(C3Fused1, launch_c3<1, 0>(va, pa, st)) /* prologue waves inside the block: 1, 2, 4, 8 heads */                          \
    X(C3Fused2, launch_c3<2, 0>(va, pa, st))                                                                                  \
    X(C3Fused4, launch_c3<4, 0>(va, pa, st))                                                                                  \
    X(C3Fused8, launch_c3<8, 0>(va, pa, st))                                                                                  \
    X(C3Waves1, launch_c3<0, 1>(va, pa, st))       /* 32 vertices x 32 heads, 3 + 1 waves */                                  \
    X(C3V128, launch_c3<0, 0, 4>(va, pa, st))      /* 128 vertices x 32 heads, 12 compute waves */                            \
    X(C3Waves5, launch_c3<0, 5>(va, pa, st))       /* 32 vertices x 32 heads, 3 + 5 waves */                                  \
    X(C3V128H64, launch_c3<0, 0, 4, 2>(va, pa, st)) /* 128 vertices x 64 heads */                                             \
    X(C3V160, launch_c3<0, 0, 5>(va, pa, st))      /* 160 vertices x 32 heads, 15 compute waves */                            \
    X(Lds32, launch_mfma_lds<1, 32>(va, st))                                                                                  \
    X(Lds64, launch_mfma_lds<2, 64>(va, st))                                                                                  \
    X(Lds128, launch_mfma_lds<4, 128>(va, st))                                                                                \
    X(Mfma32, launch_mfma<1>(va, st)) /* one 32-head tile per wave: twice the waves, two resident per SIMD */                 \
    X(Mfma64, launch_mfma<2>(va, st))                                                                                         \
    X(ValuFused1, launch_vertex_cfg<1, 64, 1, true>(va, pa, st))    /* 79 blocks per head: the whole chip pulls the basis of one head */ \
    X(ValuFused4, launch_vertex_cfg<4, 64, 1, true>(va, pa, st))    /* 79 x ceil(m/4) blocks */                               \
    X(ValuFused4V4, launch_vertex_cfg<4, 64, 4, true>(va, pa, st))  /* 20 x ceil(m/4) */                                      \
    X(ValuFused8, launch_vertex_cfg<8, 256, 4, true>(va, pa, st))   /* 5 x ceil(m/8) */                                       \
    X(Valu4, launch_vertex_cfg<4, 64, 4, false>(va, pa, st))                                                                  \
    X(Valu8, launch_vertex_cfg<8, 256, 4, false>(va, pa, st))
#ifdef VGH_EXPERIMENTS
#define FLAME_QUAD_KERNELS(X)                               \
    X(QuadFused1, launch_c3<1, 0, 1, 1, 1>(va, pa, st))     \
    X(QuadFused2, launch_c3<2, 0, 1, 1, 1>(va, pa, st))     \
    X(QuadFused4, launch_c3<4, 0, 1, 1, 1>(va, pa, st))     \
    X(QuadFused8, launch_c3<8, 0, 1, 1, 1>(va, pa, st))     \
    X(QuadWaves5, launch_c3<0, 5, 1, 1, 1>(va, pa, st))     \
    X(QuadWaves1, launch_c3<0, 1, 1, 1, 1>(va, pa, st))
#else
#define FLAME_QUAD_KERNELS(X)
#endif

enum class FlameKernel {
    None,  // neither vertices nor projections are wanted: the prologue alone
#define FLAME_PLAN_VALUE(name, ...) name,
    FLAME_QUAD_KERNELS(FLAME_PLAN_VALUE) FLAME_VERTEX_KERNELS(FLAME_PLAN_VALUE)
#undef FLAME_PLAN_VALUE
};
enum class FlamePrologue { None, WavePerHead, Blocks16 };  // none: the vertex kernel computes its own heads' prologue

struct FlamePlan {
    FlamePrologue prologue;
    FlameKernel kernel;
};

struct FlamePlanIn {
    int mode;                    // vgh_flame_set_matrix_path
    int m;                       // heads of this chunk (the capacity when the count lives on the device)
    bool n_dev;                  // the live count lives on the device
    bool detector_mode;          // true: betas [0, shape_live) and [300, 300 + expr_live) are live; false: all of NB
    int shape_live, expr_live;
    int NB, K, NP, V;            // K = NB + NP
    bool basis8;                 // the model has the k-interleaved basis copy of the c3 tiles
    int ncu;                     // compute units (0: unknown, taken as 256)
    bool outputs;                // vertices or projections are wanted
};

inline FlamePlan flame_plan(const FlamePlanIn& in) {
    const int mode = in.mode, m = in.m;
    const bool n_dev = in.n_dev;
    // matrix-core path from a handful of heads on (or the live count is only known on the device) and the
    // live ranges have even length; tiny direct batches keep the fused VALU kernel (one launch, the whole chip on one head's basis)
    const bool even = ((in.shape_live | in.expr_live | in.NB | in.K) & 1) == 0;
    // (measured, profiles/r02_flame_sweep.json: the matrix-core kernel wins from a handful of heads up to a few thousand; at crowd scale the
    //  VALU kernel's 8-heads-per-basis-load reuse is ahead again; with a device-side count the launch is capacity-sized and mostly
    //  exits at once, so the tile count that matters is the live one)
    const int amode = (mode == 8 || mode == 9) ? 1 : mode;  // 8 / 9: the automatic choice with the quad tiles forced on / off
    const int npairs = ((in.detector_mode ? in.shape_live + in.expr_live : in.NB) + in.NP + 1) / 2;
    // crowd scale: operands staged through LDS (its k-pair table holds 256 entries: FLAME has 218; a model with more coefficients keeps the other kernels)
    // r04: 32-head blocks of the LDS-staged kernel (mode 5 only).  Hypothesis: the register-fed kernel keeps at most 63 dword loads (8 KB) in flight per wave
    // and runs 77 ns per k at n = 96, so 1-KiB LDS-DMA pieces should free it.  Measured (profiles/r04_flame_sweep.json): n = 96 / 192 with all 400
    // coefficients 63.0 / 64.5 us against 59.4 / 60.2 for the register-fed kernel -- the mid range is bound by its ~30 us of K-independent work (prologue
    // kernel, two launches, head-pack staging, per-head skinning epilogue), not by loads in flight.  Kept selectable (bit-identical), not automatic.
    const bool lds32 = even && npairs <= 248 && mode == 5;
    const bool lds = lds32 || (even && npairs <= 248 && (mode == 3 || mode == 4 || (amode == 1 && !n_dev && m >= kLdsMidHeads)));
    const bool mfma = lds || (even && (mode == 2 || (amode == 1 && (n_dev ? m <= 16384 : (m >= 5 && m < 2048)))));
    // c3 tiles (component-split waves, coefficient tile in LDS; K - NB pose features in one k-group run, NB a multiple of 8 so that the pose rows start a
    // group): mode 6 always with the prologue kernel, mode 7 the same with the fused variant (prologue waves inside the block) up to 8 heads.  Automatic
    // (measured, profiles/r04_flame_sweep.json; us per call, all 400 / L-live / M-live coefficients; old = the kernels above):
    //   n = 1: 22.4 / 18.2 / 16.5 (old 33.4 / 19.2 / 16.2)    n = 8: 27.0 / 21.3 / 18.4 (52.7 / 36.6 / 30.9)    n = 32: 27.7 / 23.0 / 20.2 (58.0 / 42.0 / 36.4)
    //   n = 96: 39.1 / 30.4 / 25.4 (59.0 / 43.3 / 37.3)       n = 128: 49.9 / 35.9 / 28.3 (59.8 / 43.8 / 37.9)  n = 192: 51.3 / 37.2 / 30.0 (60.5 / 44.9 / 38.9)
    //   n = 256: 82.7 / 56.9 / 44.1 (100.4 / 71.9 / 58.9)     n = 512: 122.4 / 83.4 / 63.8 (146.4 / 101.5 / 80.2)  n = 1024: 193.3 / 127.8 / 95.0 (249.7 / 163.3 / 123.4)
    //   n = 2048: 364 / 237 / 173 (387 / 245 / 180)   n = 3072: 536 / 348 / 253 (469 / 298 / 218: the 128-head LDS-staged blocks take over)   n = 8192: 1 400 / 900 / 653 (1 192 / 766 / 569)
    // -> direct batches up to kC3MaxHeads; with a device-side count the launch is capacity-sized and the dead tile rows exit at once: any capacity the
    //    register-fed kernel took (the live count of a detector batch is a few hundred at most: 4-wave blocks up to a capacity of 128, 128-vertex blocks beyond).
    const bool c3_ok = even && in.K - in.NB <= 64 && (in.NB & 7) == 0 && in.basis8;
    const bool c3_auto = amode == 1 && (n_dev ? m <= 16384 : m <= kC3MaxHeads) && !(m <= 2 && npairs < 100);  // (1 - 2 heads of the M set: the VALU kernel)
    const bool c3 = c3_ok && (mode == 6 || mode == 7 || c3_auto);
    const bool c3_fused = c3 && mode != 6 && !n_dev && m <= 8 && in.outputs;
    const bool fused = c3_fused || (!c3 && !mfma && !n_dev && m <= 256);  // the vertex kernel computes its own heads' prologue

    FlamePlan p{FlamePrologue::None, FlameKernel::None};
    if (!fused || !in.outputs)
        // (the c3 tiles fetch the rows by LDS-DMA either way: the one-wave-per-block prologue is ~5 us shorter below a few thousand heads)
        // 16-head blocks: coalesced coefficient rows (measured: 16 waves per block cost 17 us vs 9.5 us at n = 96, but 92 vs 112 us at n = 8192)
        p.prologue = m >= (c3 ? 4096 : 512) ? FlamePrologue::Blocks16 : FlamePrologue::WavePerHead;
    if (!in.outputs) return p;

    using FK = FlameKernel;
    // quad tiles (16 x 16 x 4 MFMAs, r06): measured and NOT adopted -- bit-identical, but no faster at one head (14.8 vs 15.0 us, M set; 19.4 vs 19.7 with all 400
    // coefficients) and 30 - 60 % slower from two heads on (profiles/r06_flame_quad_tiles.txt): a small decode is not its dependent MFMA chain long, it is the
    // basis stream per wave.  Kept in the -DVGH_EXPERIMENTS build (mode 8 forces them up to 128 heads; mode 9 = mode 1 = without them).
#ifdef VGH_EXPERIMENTS
    if (c3 && mode == 8 && m <= 128) {
        if (c3_fused) p.kernel = m <= 1 ? FK::QuadFused1 : m <= 2 ? FK::QuadFused2 : m <= 4 ? FK::QuadFused4 : FK::QuadFused8;
        else p.kernel = m <= 32 ? FK::QuadWaves5 : FK::QuadWaves1;
        return p;
    }
#endif
    if (c3_fused) {
        p.kernel = m <= 1 ? FK::C3Fused1 : m <= 2 ? FK::C3Fused2 : m <= 4 ? FK::C3Fused4 : FK::C3Fused8;
    } else if (c3) {
        // one head tile: 3 + 5 waves; up to 96 heads: 3 + 1 (two blocks per CU; n = 112: 51.1 vs 50.1 us for the 128-vertex blocks); beyond: 128-vertex blocks of 12 compute waves (64-vertex blocks of 6 measured
        // slower than both everywhere)
        if (n_dev) p.kernel = m <= 128 ? FK::C3Waves1 : FK::C3V128;  // (capacity, not the live count)
        else if (m <= 96) p.kernel = m <= 32 ? FK::C3Waves5 : FK::C3Waves1;
        else {
            // one block per CU: 128 vertices x 32 heads (12 compute waves), 160 x 32 (15 waves) or 128 x 64 (12 waves, two head tiles' chains per wave on one
            // basis operand) -- whichever needs the least time in ROUNDS of blocks over the CUs, a round costing 1.0 / 1.3 / 1.72 of the first's (measured,
            // all 400 coefficients: n = 256 59.7 vs 82.9 us for 160- vs 128-vertex blocks, 384 100.8 vs 86.0, 512 103.2 vs 118.3 (64-head blocks 134.2),
            // 1 024 189.4 vs 190.2 (196.8), 2 048 361.9 vs 364.3 (323.5))
            const int vgroups = (in.V + 31) / 32, hg = (m + 31) / 32, ncu = in.ncu > 0 ? in.ncu : 256;
            const int r4 = (hg * ((vgroups + 3) / 4) + ncu - 1) / ncu, r5 = (hg * ((vgroups + 4) / 5) + ncu - 1) / ncu, r2 = ((hg + 1) / 2 * ((vgroups + 3) / 4) + ncu - 1) / ncu;
            const int c4 = 100 * r4, c5 = 130 * r5, c2 = 172 * r2;
            p.kernel = c2 < c4 && c2 < c5 ? FK::C3V128H64 : c5 < c4 ? FK::C3V160 : FK::C3V128;
        }
    } else if (lds) {
        // 128-head blocks at crowd scale; 64-head blocks (twice the blocks) below it and in mode 4.
        // `mode == 1`, not `amode == 1` as everywhere else: mode 9 ("= mode 1") therefore takes 128-head blocks where mode 1 takes 64-head ones (256 .. 1023 direct
        // heads of a model the c3 tiles cannot run).  Same bits; kept as it was found -- which of the two mode 9 should run has not been decided.
        p.kernel = lds32 ? FK::Lds32 : (mode == 4 || (mode == 1 && m < kLdsMinHeads)) ? FK::Lds64 : FK::Lds128;
    } else if (mfma) {
        p.kernel = n_dev || m <= 512 ? FK::Mfma32 : FK::Mfma64;
    } else if (fused) {
        p.kernel = m <= 4 ? FK::ValuFused1 : m <= 32 ? FK::ValuFused4 : m <= 96 ? FK::ValuFused4V4 : FK::ValuFused8;
    } else {
        p.kernel = m <= 24 ? FK::Valu4 : FK::Valu8;
    }
    return p;
}
