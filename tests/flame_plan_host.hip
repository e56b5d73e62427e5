// Stand-alone check of csrc/flame_plan.h (which kernels a FLAME decode runs) and csrc/per_device.h (the once-per-device routine and the slot function).
// tests/test_flame_plan_host.py builds it with the host sanitizers (address, undefined), as the product and with -DVGH_EXPERIMENTS, and runs it on its own.
// It makes no HIP call.
#include <stdio.h>
#include <stdlib.h>

#include "../head_detector_amd/csrc/flame_plan.h"
#include "../head_detector_amd/csrc/per_device.h"

static int failures = 0;
#define EXPECT(cond, ...)                 \
    do {                                  \
        if (!(cond)) {                    \
            ++failures;                   \
            printf("FAILED %s: ", #cond); \
            printf(__VA_ARGS__);          \
            printf("\n");                 \
            if (failures > 20) exit(1);   \
        }                                 \
    } while (0)

using P = FlamePrologue;
using K = FlameKernel;

static const char* name(K k) {
    switch (k) {
#define NAME(value, ...) \
    case K::value: return #value;
        FLAME_QUAD_KERNELS(NAME) FLAME_VERTEX_KERNELS(NAME)
#undef NAME
        case K::None: return "None";
    }
    return "?";
}
static const char* name(P p) { return p == P::None ? "None" : p == P::WavePerHead ? "WavePerHead" : "Blocks16"; }

// THE EXPECTED VALUES WERE NOT TAKEN FROM flame_plan: they were printed by a program holding the if-chain that run_decode_on had before flame_plan.h existed,
// verbatim, with every launch replaced by its name (the same program compared the two over 102 405 120 cases: profiles/launch_paths_refactor.txt).
// V = 5023 throughout; NP = 9 (NJ - 1), K = NB + NP.
struct Row {
    int mode, m, n_dev, detector_mode, shape_live, expr_live, NB, NJ, basis8, ncu, outputs;
    P prologue;
    K kernel;
};
static const Row kTable[] = {
    {1, 1, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused1},
    {1, 2, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused2},
    {1, 3, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused4},
    {1, 4, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused4},
    {1, 5, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused8},
    {1, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused8},
    {1, 9, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {1, 24, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {1, 25, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {1, 32, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {1, 33, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves1},
    {1, 96, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves1},
    {1, 97, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 255, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 256, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 257, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 1023, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 1024, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 2047, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 2048, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 2049, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::Lds128},
    {1, 1, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::None, K::ValuFused1},
    {1, 2, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::None, K::ValuFused1},
    {1, 3, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::None, K::ValuFused1},
    {1, 4, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::None, K::ValuFused1},
    {1, 5, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 8, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 9, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 24, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 25, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 32, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 33, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 96, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 97, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 255, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 256, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Lds64},
    {1, 257, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Lds64},
    {1, 1023, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds64},
    {1, 1024, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds128},
    {1, 2047, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds128},
    {1, 2048, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds128},
    {1, 2049, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds128},
    {1, 511, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Lds64},
    {1, 512, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds64},
    {1, 513, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds64},
    {0, 4, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused1},
    {0, 5, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused4},
    {0, 24, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused4},
    {0, 25, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused4},
    {0, 32, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused4},
    {0, 33, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused4V4},
    {0, 96, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused4V4},
    {0, 97, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused8},
    {0, 256, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::ValuFused8},
    {0, 257, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::Valu8},
    {0, 511, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::Valu8},
    {0, 512, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::Valu8},
    {1, 128, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves1},
    {1, 129, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 4095, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 4096, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::C3V128},
    {1, 16384, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::C3V128},
    {1, 16385, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::Valu8},
    {1, 16, 1, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 511, 1, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 512, 1, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Mfma32},
    {1, 16384, 1, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Mfma32},
    {1, 16385, 1, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Valu8},
    {6, 4095, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {6, 4096, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::C3V128H64},
    {0, 1, 0, 1, 300, 100, 400, 5, 1, 256, 0, P::WavePerHead, K::None},
    {0, 511, 0, 1, 300, 100, 400, 5, 1, 256, 0, P::WavePerHead, K::None},
    {0, 512, 0, 1, 300, 100, 400, 5, 1, 256, 0, P::Blocks16, K::None},
    {1, 8, 0, 1, 300, 100, 400, 5, 1, 256, 0, P::WavePerHead, K::None},
    {1, 4095, 0, 1, 300, 100, 400, 5, 1, 256, 0, P::Blocks16, K::None},
    {1, 4096, 0, 1, 300, 100, 400, 5, 1, 256, 0, P::Blocks16, K::None},
    {1, 1, 0, 1, 64, 32, 400, 5, 1, 256, 1, P::None, K::ValuFused1},
    {1, 2, 0, 1, 64, 32, 400, 5, 1, 256, 1, P::None, K::ValuFused1},
    {1, 3, 0, 1, 64, 32, 400, 5, 1, 256, 1, P::None, K::C3Fused4},
    {1, 1, 0, 1, 128, 64, 400, 5, 1, 256, 1, P::None, K::C3Fused1},
    {1, 2, 0, 1, 128, 64, 400, 5, 1, 256, 1, P::None, K::C3Fused2},
    {1, 3, 0, 1, 128, 64, 400, 5, 1, 256, 1, P::None, K::C3Fused4},
    {1, 1, 0, 1, 127, 63, 400, 5, 1, 256, 1, P::None, K::ValuFused1},
    {1, 8, 0, 1, 127, 63, 400, 5, 1, 256, 1, P::None, K::ValuFused4},
    {1, 96, 0, 1, 127, 63, 400, 5, 1, 256, 1, P::None, K::ValuFused4V4},
    {1, 300, 0, 1, 127, 63, 400, 5, 1, 256, 1, P::WavePerHead, K::Valu8},
    {1, 2048, 0, 1, 127, 63, 400, 5, 1, 256, 1, P::Blocks16, K::Valu8},
    {1, 192, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 193, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 384, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 385, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 512, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 513, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 608, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 609, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 768, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 769, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 1025, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 1216, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 1217, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 1280, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V160},
    {1, 1281, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 1600, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 1601, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 1632, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 1633, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
    {1, 97, 0, 1, 300, 100, 400, 5, 1, 64, 1, P::WavePerHead, K::C3V160},
    {1, 128, 0, 1, 300, 100, 400, 5, 1, 64, 1, P::WavePerHead, K::C3V160},
    {1, 129, 0, 1, 300, 100, 400, 5, 1, 64, 1, P::WavePerHead, K::C3V128H64},
    {1, 256, 0, 1, 300, 100, 400, 5, 1, 64, 1, P::WavePerHead, K::C3V128},
    {1, 97, 0, 1, 300, 100, 400, 5, 1, 0, 1, P::WavePerHead, K::C3V128},
    {1, 256, 0, 1, 300, 100, 400, 5, 1, 0, 1, P::WavePerHead, K::C3V160},
    {9, 255, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Mfma32},
    {9, 256, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::WavePerHead, K::Lds128},
    {9, 1023, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds128},
    {9, 1024, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::Blocks16, K::Lds128},
    {2, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::Mfma32},
    {2, 512, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::Mfma32},
    {2, 513, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::Blocks16, K::Mfma64},
    {3, 10, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::Lds128},
    {4, 10, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::Lds64},
    {5, 10, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::Lds32},
    {3, 10, 0, 0, 300, 100, 600, 5, 1, 256, 1, P::None, K::ValuFused4},
    {6, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {7, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused8},
    {6, 9, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {7, 9, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {6, 32, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {7, 32, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves5},
    {6, 33, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves1},
    {7, 33, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves1},
    {7, 8, 1, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3Waves1},
    {9, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused8},
    {9, 100, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {8, 129, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {1, 8, 0, 1, 300, 100, 400, 9, 1, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 100, 0, 1, 300, 100, 400, 9, 1, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 8, 0, 0, 0, 0, 12, 5, 1, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 100, 0, 0, 0, 0, 12, 5, 1, 256, 1, P::WavePerHead, K::Mfma32},
    {1, 8, 0, 0, 0, 0, 400, 5, 1, 256, 1, P::None, K::C3Fused8},
    {1, 300, 0, 0, 0, 0, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128H64},
#ifdef VGH_EXPERIMENTS  // mode 8 forces the quad tiles up to 128 heads
    {8, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::QuadFused8},
    {8, 100, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::QuadWaves1},
    {8, 128, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::QuadWaves1},
#else
    {8, 8, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::C3Fused8},
    {8, 100, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
    {8, 128, 0, 1, 300, 100, 400, 5, 1, 256, 1, P::WavePerHead, K::C3V128},
#endif
};

static FlamePlanIn input(const Row& r) {
    const int NP = 9 * (r.NJ - 1);
    return {r.mode, r.m, r.n_dev != 0, r.detector_mode != 0, r.shape_live, r.expr_live, r.NB, r.NB + NP, NP, 5023, r.basis8 != 0, r.ncu, r.outputs != 0};
}

static void check_plan_table() {
    for (const Row& r : kTable) {
        const FlamePlan p = flame_plan(input(r));
        EXPECT(p.prologue == r.prologue && p.kernel == r.kernel, "mode %d, %d heads (n_dev %d), live %d: %d + %d, NB %d, NJ %d, basis8 %d, %d CUs, outputs %d: %s | %s, expected %s | %s", r.mode, r.m,
               r.n_dev, r.detector_mode, r.shape_live, r.expr_live, r.NB, r.NJ, r.basis8, r.ncu, r.outputs, name(p.prologue), name(p.kernel), name(r.prologue), name(r.kernel));
    }
    // mode 9 is documented as "= mode 1", and is except here: 256 .. 1023 direct heads of a model the c3 tiles cannot run (see the comment in flame_plan)
    Row r{1, 300, 0, 1, 300, 100, 400, 5, 0, 256, 1, P::None, K::None};
    EXPECT(flame_plan(input(r)).kernel == K::Lds64, "mode 1");
    r.mode = 9;
    EXPECT(flame_plan(input(r)).kernel == K::Lds128, "mode 9");
    EXPECT(kLdsMidHeads == 256 && kLdsMinHeads == 1024 && kC3MaxHeads == 2048, "thresholds");
}

// for the test model (FLAME: NB 400, NJ 5, V 5023, basis8 present) on 256 CUs, automatic mode, all coefficients live: the smallest head count (direct) or
// capacity (count on the device) that reaches each plan value -- what the GPU bit-identity tests have to run to cover the choice
static void print_first_heads() {
    for (int n_dev = 0; n_dev < 2; ++n_dev) {
        bool seen[64] = {};
        for (int m = 1; m <= 20000; ++m) {
            const Row r{1, m, n_dev, 1, 300, 100, 400, 5, 1, 256, 1, P::None, K::None};
            const FlamePlan p = flame_plan(input(r));
            if (seen[(int)p.kernel]) continue;
            seen[(int)p.kernel] = true;
            printf("first %s of %5d: %s after prologue %s\n", n_dev ? "capacity" : "batch", m, name(p.kernel), name(p.prologue));
        }
    }
    for (int m = 1; m <= 2; ++m) printf("M-live set (64 + 32), batch of %d: %s\n", m, name(flame_plan(input({1, m, 0, 1, 64, 32, 400, 5, 1, 256, 1, P::None, K::None})).kernel));
}

static void check_per_device() {
    EXPECT(device_slot(hipSuccess, 0) == 0 && device_slot(hipSuccess, 15) == 15, "slots 0 and 15");
    EXPECT(device_slot(hipSuccess, -1) == kNoSlot && device_slot(hipSuccess, 16) == kNoSlot && device_slot(hipSuccess, kMaxDevices) == kNoSlot, "ids outside the table");
    EXPECT(device_slot(hipErrorInvalidDevice, 0) == kNoSlot && device_slot(hipErrorNoDevice, 3) == kNoSlot, "a failed query");
    static PerDevice state;
    int calls = 0;
    const auto seven = [&] { return ++calls, 7; };
    EXPECT(once_per_device(state, 0, seven) == 7 && calls == 1, "first call on slot 0 runs");
    EXPECT(once_per_device(state, 0, seven) == 7 && calls == 1, "second call on slot 0 does not");
    EXPECT(once_per_device(state, 3, seven) == 7 && calls == 2, "another slot runs");
    EXPECT(once_per_device(state, 3, seven) == 7 && calls == 2, "... once");
    for (int i = 0; i < 3; ++i) EXPECT(once_per_device(state, kNoSlot, seven) == 7 && calls == 3 + i, "no slot: every time");
    EXPECT(once_per_device(state, device_slot(hipSuccess, 16), seven) == 7 && calls == 6, "device 16 borrows nobody's slot");
    int tries = 0;
    const auto second_time_lucky = [&] { return ++tries >= 2 ? 1 : 0; };
    EXPECT(once_per_device(state, 5, second_time_lucky) == 0 && tries == 1, "a failure is reported");
    EXPECT(once_per_device(state, 5, second_time_lucky) == 1 && tries == 2, "... and retried");
    EXPECT(once_per_device(state, 5, second_time_lucky) == 1 && tries == 2, "... until it succeeds");
    for (int s = 0; s < kMaxDevices; ++s) EXPECT(state.v[s].load() == (s == 0 || s == 3 ? 7 : s == 5 ? 1 : 0), "slot %d", s);
}

int main() {
    check_plan_table();
    check_per_device();
    print_first_heads();
    if (failures) return 1;
    printf("flame_plan and per_device host checks passed (%d plan rows)\n", (int)(sizeof(kTable) / sizeof(kTable[0])));
    return 0;
}
