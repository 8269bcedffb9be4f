// render_device.hpp - what more than one of the rasterizer's units (render_scene.hip, render_pre.hip, render.hip) inlines or shares:
// the launch geometry, the JavaScript number semantics, the label edits' tables and the viewer's matrices.  Every unit that
// includes it is compiled with -ffp-contract=off (JavaScript never fuses).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/gsx.h"

namespace gsx {

static constexpr int kRB = 256;
static inline unsigned grid_for(long long n) { return (unsigned)((n + kRB - 1) / kRB); }

// ---- JavaScript number semantics -----------------------------------------------------------------
__device__ __forceinline__ unsigned js_u8clamp(double x) {  // Uint8ClampedArray store
    if (!(x > 0.0)) return 0u;
    if (x >= 255.0) return 255u;
    const double f = floor(x);
    if (f + 0.5 < x) return (unsigned)(f + 1.0);
    if (x < f + 0.5) return (unsigned)f;
    return (unsigned)(fmod(f, 2.0) == 0.0 ? f : f + 1.0);
}

__device__ __forceinline__ int js_toint32(double x) {  // `x | 0`
    if (!(fabs(x) <= 1.7976931348623157e308)) return 0;  // NaN, +-Infinity
    const double t = trunc(x);
    if (t >= -2147483648.0 && t <= 2147483647.0) return (int)t;
    double m = fmod(t, 4294967296.0);
    if (m < 0) m += 4294967296.0;
    return (int)(unsigned)m;
}

__device__ __forceinline__ unsigned js_float_to_half(double v) {  // gs.js:248-275
    const float fl = (float)v;
    const int f = __float_as_int(fl);
    const int sign = (f >> 31) & 0x0001;
    const int exp = (f >> 23) & 0x00ff;
    int frac = f & 0x007fffff;
    int newExp;
    if (exp == 0) {
        newExp = 0;
    } else if (exp < 113) {
        newExp = 0;
        frac |= 0x00800000;
        frac = frac >> ((113 - exp) & 31);  // JS shift counts are taken mod 32
        if (frac & 0x01000000) {
            newExp = 1;
            frac = 0;
        }
    } else if (exp < 142) {
        newExp = exp - 112;
    } else {
        newExp = 31;
        frac = 0;
    }
    return (unsigned)((sign << 15) | (newExp << 10) | (frac >> 13));
}

__device__ __forceinline__ float half_to_float(unsigned h) {  // unpackHalf2x16: exact
    const unsigned s = (h >> 15) & 1u, e = (h >> 10) & 31u, m = h & 1023u;
    float v;
    if (e == 0) v = (float)m * 5.9604644775390625e-08f;  // 2^-24
    else if (e == 31) v = m ? __int_as_float(0x7fc00000) : __int_as_float(0x7f800000);
    else v = __int_as_float((int)(((e + 112u) << 23) | (m << 13)));
    return s ? -v : v;
}

// a splat's tile rectangle is tx0 | tx1 << 8 | ty0 << 16 | ty1 << 24.  (edge_min_q / tile_touches - the exact "does the ellipse
// reach this tile?" test - live in tile_test.hpp: the blend kernel uses them too)
static constexpr uint32_t kEmptyRect = 1u;  // tx0 = 1 > tx1 = 0: covers no tile

// ---- label edits (include/gsx.h: gsx_render_set_edits) ----------------------------------------------------------------------
// The shaders run two 100-entry loops per splat per frame (getDisplacement gs.js:686-693, getCustomColor gs.js:772-780).  Here
// edit_code_kernel resolves them ONCE per state into 16 bits per splat; the pre kernels' EDIT instantiations read the code and
// the tables (a 2.5 KB device struct: the flags and u_customColor are wave-uniform scalar loads, a table row is indexed by the
// splat's slot).
//   code bits 0-6: slot + 1 in the colour table (0: none), 7-13: slot + 1 in the displacement table, 14: hidden, 15: the label
//   equals uSelectedLabel
static constexpr unsigned kEditHidden = 1u << 14, kEditSelected = 1u << 15;
struct EditTables {
    float colour[GSX_EDIT_TABLE_MAX][3];
    float disp[GSX_EDIT_TABLE_MAX][3];
    int colour_label[GSX_EDIT_TABLE_MAX];
    int disp_label[GSX_EDIT_TABLE_MAX];
    float custom[3];
    int n_colour, n_disp;
    int selection_mode, enable_custom, enable_disp;
    int selected;
    int n_hidden;
};

// the vertex shader's displacement of a splat (gs.js:701-704): the table row, or vec3(0.0) without one; nothing is added
// while u_enableDisplacement is off
__device__ __forceinline__ void edit_displacement(unsigned code, const EditTables& e, float& dx, float& dy, float& dz) {
    const unsigned slot = (code >> 7) & 127u;
    dx = dy = dz = 0.f;
    if (e.enable_disp != 0 && slot != 0u) dx = e.disp[slot - 1][0], dy = e.disp[slot - 1][1], dz = e.disp[slot - 1][2];
}

__device__ __forceinline__ float glsl_mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }

// fragment shader, gs.js:786-797, on the splat's colour (it does not depend on the pixel): col[0..2] = vColor.rgb, faded.
// Hidden: the alpha BYTE is 0 (gs.js:320), vColor.a = fade * 0 / 255.
__device__ __forceinline__ void edit_colour(float col[4], unsigned code, const EditTables& e, float fade) {
    const unsigned slot = code & 127u;
    if (slot != 0u) {
#pragma unroll
        for (int k = 0; k < 3; ++k) col[k] = glsl_mix(col[k], e.colour[slot - 1][k], 0.6f);
    }
    if (code & kEditSelected) {
        if (e.enable_custom != 0) {
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = e.custom[k];
        }
        if (e.selection_mode != 0) {
            col[0] = glsl_mix(col[0], 1.0f, 0.5f);
            col[1] = glsl_mix(col[1], 0.0f, 0.5f);
            col[2] = glsl_mix(col[2], 0.0f, 0.5f);
        }
    }
    if (code & kEditHidden) col[3] = fade * 0.0f / 255.0f;
}

// ---- the viewer's matrices (host): gs.js:81-107 and 66-79, fp64 exactly as the JavaScript evaluates them ----------------------
inline void js_view_matrix(const gsx_camera* cam, double out[16]) {
    const double* R = cam->R;
    const double* p = cam->p;
    for (int i = 0; i < 3; ++i) {
        out[4 * i + 0] = R[3 * i + 0];
        out[4 * i + 1] = R[3 * i + 1];
        out[4 * i + 2] = R[3 * i + 2];
        out[4 * i + 3] = 0.0;
    }
    for (int i = 0; i < 3; ++i) out[12 + i] = -p[0] * R[i] - p[1] * R[i + 3] - p[2] * R[i + 6];
    out[15] = 1.0;
}

inline void js_proj_matrix(double fx, double fy, double width, double height, double out[16]) {
    const double Z_FAR = 200.0, Z_NEAR = 0.2;
    const double zRange = Z_FAR - Z_NEAR;
    for (int k = 0; k < 16; ++k) out[k] = 0.0;
    out[0] = (2 * fx) / width;
    out[5] = -(2 * fy) / height;
    out[10] = Z_FAR / zRange;
    out[11] = 1.0;
    out[14] = -(Z_FAR * Z_NEAR) / zRange;
}

inline void js_multiply4(const double A[16], const double B[16], double out[16]) {
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            out[4 * i + j] = B[4 * i] * A[j] + B[4 * i + 1] * A[j + 4] + B[4 * i + 2] * A[j + 8] + B[4 * i + 3] * A[j + 12];
}

}  // namespace gsx
