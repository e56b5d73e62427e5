// Host side of the letterbox: a C++ port of head_detector_amd/letterbox.py::geometry / ::axis_tables (the Python module is the spec).
// The tables must be BIT-IDENTICAL to the Python ones (the canvas of VGH_IMG_U8_RAW equals letterbox.letterbox() byte for byte): the same
// double / float32 operation order, glibc's sin / cos as Python's math module calls them, rint (half to even) and the int16 clamp, and no
// contraction of a * b + c into an FMA.  Plain C++ (no HIP): tests/ compile it with the system compiler to compare with the Python tables.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

namespace vgh_lb {

// detector.py:41-46,48-49 -> (new_h, new_w, pad_x, pad_y, scale); new_h or new_w < 1: the image is too elongated for an S x S letterbox
struct Geometry {
    int new_h, new_w, pad_x, pad_y;
    double scale;
};

inline Geometry geometry(int h, int w, int S) {
    Geometry g;
    // Python: int(w * S / h) -- an exact integer product, one correctly rounded division, truncation
    if (h > w) {
        g.new_h = S;
        g.new_w = (int)((double)((int64_t)w * S) / (double)h);
    } else {
        g.new_h = (int)((double)((int64_t)h * S) / (double)w);
        g.new_w = S;
    }
    g.pad_x = (S - g.new_w) / 2;  // S - new_* >= 0: floor division == truncation
    g.pad_y = (S - g.new_h) / 2;
    g.scale = (double)S / (double)(h > w ? h : w);
    return g;
}

// resize.cpp's 8-bit LANCZOS4 tables of one axis: ofs[dst] (floor source coordinate), coef[dst][8] (weights * 2048 as int16)
struct AxisTables {
    std::vector<int32_t> ofs;
    std::vector<int16_t> coef;
};

#ifdef __clang__
#pragma clang fp contract(off)  // (a compiler without the pragma is run with -ffp-contract=off, as the test does)
#endif

// interpolateLanczos4: float weights of the 8 taps for the fractional position x (letterbox.py::_lanczos4)
inline void lanczos4(double x, float c[8]) {
    for (int i = 0; i < 8; ++i) c[i] = 0.0f;
    if ((float)x < 1.1920928955078125e-07f) {  // np.finfo(np.float32).eps (x holds a float32 value)
        c[3] = 1.0f;
        return;
    }
    static const double s45 = 0.70710678118654752440084436210485;
    static const double cs[8][2] = {{1, 0}, {-s45, -s45}, {0, 1}, {s45, -s45}, {-1, 0}, {s45, s45}, {0, -1}, {-s45, s45}};
    const double pi = 3.141592653589793;  // math.pi
    const double y0 = -(x + 3) * pi * 0.25;
    const double s0 = sin(y0), c0 = cos(y0);
    float total = 0.0f;
    for (int i = 0; i < 8; ++i) {
        const double y = -(x + 3 - i) * pi * 0.25;
        const double num = cs[i][0] * s0;
        const double num2 = cs[i][1] * c0;
        c[i] = (float)((num + num2) / (y * y));
        total = total + c[i];
    }
    const float inv = 1.0f / total;
    for (int i = 0; i < 8; ++i) c[i] = c[i] * inv;
}

inline AxisTables axis_tables(int src, int dst) {
    AxisTables t;
    t.ofs.resize(dst);
    t.coef.resize((size_t)dst * 8);
    const double scale = 1.0 / ((double)dst / (double)src);
    for (int d = 0; d < dst; ++d) {
        const double pos = (d + 0.5) * scale;
        const float f = (float)(pos - 0.5);
        const int s = (int)floor((double)f);
        t.ofs[d] = s;
        float w[8];
        lanczos4((double)(f - (float)s), w);
        for (int k = 0; k < 8; ++k) {
            double v = rint((double)(w[k] * 2048.0f));
            v = v < -32768.0 ? -32768.0 : (v > 32767.0 ? 32767.0 : v);
            t.coef[(size_t)d * 8 + k] = (int16_t)v;
        }
    }
    return t;
}

}  // namespace vgh_lb
