// render_pre.hip - the rasterizer's per-view per-splat pass: runSort's depth keys and 16-bit buckets (gs.js:432-447), the vertex
// shader (gs.js:696-750, fp32) and the SH colour.  Compiled with -ffp-contract=off: JS never fuses, and the vertex stage must
// produce bit-identical axes to the oracle so that the fragment `discard` (A < -4) decides identically.
//
// HBM layout, one PreSet per view in flight: depth int[n], rect u32[n] (kEmptyRect: the splat reaches no pixel), pre int[4] and
//   rec        3 x float4 per splat per view, ONE 48-byte record: (cx, cy, g0x, g0y) (g1x, g1y, r, g) (b, a, -, -).  (Rounds 1-2 and
//              most of round 3 kept three arrays: a blend gather then touched three 64-byte segments per record instead of 1.5.)
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gsx_ctx.hpp"
#include "render_device.hpp"

namespace gsx {

// ---- spherical-harmonics colour (degrees 1..3; not in the reference, see oracle/render_oracle.c; planes: sh_pack_kernel) -----
// colour of one splat seen from the camera position: clamp(0.5 + SH(dir), 0, 1) per channel.
// Coef: where coefficient (k, c) of the splat comes from - CoefMem reads the planes (one view at a time), CoefRegs holds the
// splat's coefficients in registers (pre_multi_kernel: read once, used by every view of the group).  Same operations in the
// same order either way.
struct CoefMem {
    const float* __restrict__ coef;
    long long n, i;
    __device__ __forceinline__ float get(int k, int c) const { return coef[((size_t)k * 3 + c) * (size_t)n + (size_t)i]; }
};
struct CoefRegs {
    float v[48];
    __device__ __forceinline__ float get(int k, int c) const { return v[3 * k + c]; }
};

// real SH basis function k of the unit direction (x, y, z): ONE set of expressions for every caller, so that the colour of a
// splat does not depend on which kernel evaluated it (no contraction in this file; k is a compile-time constant wherever
// this is called, the switch folds away)
__device__ __forceinline__ float sh_basis(int k, float x, float y, float z) {
    const float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    const float C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
    const float C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f, 0.3731763325901154f,
                         -0.4570457994644658f, 1.445305721320277f, -0.5900435899266435f};
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    switch (k) {
        case 0: return C0;
        case 1: return -C1 * y;
        case 2: return C1 * z;
        case 3: return -C1 * x;
        case 4: return C2[0] * xy;
        case 5: return C2[1] * yz;
        case 6: return C2[2] * (2.0f * zz - xx - yy);
        case 7: return C2[3] * xz;
        case 8: return C2[4] * (xx - yy);
        case 9: return C3[0] * y * (3.0f * xx - yy);
        case 10: return C3[1] * xy * z;
        case 11: return C3[2] * y * (4.0f * zz - xx - yy);
        case 12: return C3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy);
        case 13: return C3[4] * x * (4.0f * zz - xx - yy);
        case 14: return C3[5] * z * (xx - yy);
        default: return C3[6] * x * (xx - 3.0f * yy);
    }
}

// unit vector from the camera position to the splat
__device__ __forceinline__ void sh_dir(float px, float py, float pz, float cpx, float cpy, float cpz, float& x, float& y, float& z) {
    const float dx = px - cpx, dy = py - cpy, dz = pz - cpz;
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    x = dx / len, y = dy / len, z = dz / len;
}

__device__ __forceinline__ float sh_clamp(float acc) {
    const float v = acc + 0.5f;
    return v < 0.0f ? 0.0f : (v > 1.0f ? 1.0f : v);
}

template <class Coef>
__device__ __forceinline__ void sh_color(const Coef& cf, int deg, float px, float py, float pz, float cpx, float cpy, float cpz,
                                         float rgb[3]) {
    float x, y, z;
    sh_dir(px, py, pz, cpx, cpy, cpz, x, y, z);
    const int K = (deg + 1) * (deg + 1);
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        if (k < K) {
            const float b = sh_basis(k, x, y, z);
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = k == 0 ? b * cf.get(0, c) : acc[c] + b * cf.get(k, c);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = sh_clamp(acc[c]);
}

// ---- per view ------------------------------------------------------------------------------------------
struct ViewUniforms {
    double vp2, vp6, vp10;  // row 2 of proj*view (gs.js:437)
    float view[16];         // uniforms as the GPU sees them: f32
    float proj[16];
    float fx, fy, W, H;
    int tiles_x, tiles_y;
};

// One splat in one view, everything but the colour: depth key (gs.js:436-441: ((vp2 x + vp6 y + vp10 z) * 4096) | 0, fp64),
// vertex shader (gs.js:696-750, fp32 in the oracle's operation order) and the tile rectangle of the ellipse's bounding box.
// colour: the splat reaches a pixel of this view (r0, g1 and fade are valid, a colour is wanted).
struct PreGeom {
    int depth;
    uint32_t rect;
    float4 r0;       // (cx, cy, g0x, g0y)
    float g1x, g1y;  // second axis: the first half of r1
    float fade;
    bool colour;
};

// DISP (label edits): (dx, dy, dz) is added to the centre the VERTEX SHADER sees (gs.js:701-704) - the depth key above it stays
// that of the texture position, as runSort's buffer is never displaced (include/gsx.h).  Without DISP: the code as it was.
template <bool DISP = false>
__device__ __forceinline__ PreGeom pre_geom(const uint4 t0, const uint4 t1, const ViewUniforms& u, float dx_ = 0.f, float dy_ = 0.f,
                                            float dz_ = 0.f) {
    PreGeom o;
    float cx_ = __uint_as_float(t0.x), cy_ = __uint_as_float(t0.y), cz_ = __uint_as_float(t0.z);
    o.depth = js_toint32((u.vp2 * (double)cx_ + u.vp6 * (double)cy_ + u.vp10 * (double)cz_) * 4096.0);
    if (DISP) cx_ = cx_ + dx_, cy_ = cy_ + dy_, cz_ = cz_ + dz_;
    o.rect = kEmptyRect;
    o.r0 = make_float4(0.f, 0.f, 0.f, 0.f);
    o.g1x = o.g1y = o.fade = 0.f;
    o.colour = false;
    // ---- vertex shader, fp32 ----
    float cam[4], p2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) cam[k] = u.view[k] * cx_ + u.view[4 + k] * cy_ + u.view[8 + k] * cz_ + u.view[12 + k] * 1.0f;
#pragma unroll
    for (int k = 0; k < 4; ++k) p2[k] = u.proj[k] * cam[0] + u.proj[4 + k] * cam[1] + u.proj[8 + k] * cam[2] + u.proj[12 + k] * cam[3];
    const float clip = 1.2f * p2[3];
    bool drawn = !(p2[2] < -clip || p2[0] < -clip || p2[0] > clip || p2[1] < -clip || p2[1] > clip);
    if (drawn) {
        const float u1x = half_to_float(t1.x & 0xffffu), u1y = half_to_float(t1.x >> 16);
        const float u2x = half_to_float(t1.y & 0xffffu), u2y = half_to_float(t1.y >> 16);
        const float u3x = half_to_float(t1.z & 0xffffu), u3y = half_to_float(t1.z >> 16);
        const float V[3][3] = {{u1x, u1y, u2x}, {u1y, u2y, u3x}, {u2x, u3x, u3y}};
        const float ja = u.fx / cam[2], jb = -(u.fx * cam[0]) / (cam[2] * cam[2]);
        const float jc = -u.fy / cam[2], jd = (u.fy * cam[1]) / (cam[2] * cam[2]);
        float ta[3], tb[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            ta[k] = u.view[4 * k + 0] * ja + u.view[4 * k + 1] * 0.0f + u.view[4 * k + 2] * jb;
            tb[k] = u.view[4 * k + 0] * 0.0f + u.view[4 * k + 1] * jc + u.view[4 * k + 2] * jd;
        }
        float a0[3], a1[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            a0[k] = ta[0] * V[k][0] + ta[1] * V[k][1] + ta[2] * V[k][2];
            a1[k] = tb[0] * V[k][0] + tb[1] * V[k][1] + tb[2] * V[k][2];
        }
        const float c00 = a0[0] * ta[0] + a0[1] * ta[1] + a0[2] * ta[2];
        const float c01 = a1[0] * ta[0] + a1[1] * ta[1] + a1[2] * ta[2];
        const float c11 = a1[0] * tb[0] + a1[1] * tb[1] + a1[2] * tb[2];
        const float mid = (c00 + c11) / 2.0f;
        const float hx = (c00 - c11) / 2.0f;
        const float radius = sqrtf(hx * hx + c01 * c01);
        const float l1 = mid + radius, l2 = mid - radius;
        if (l2 < 0.0f) drawn = false;  // gs.js:736
        const float dx = c01, dy = l1 - c00;
        const float dl = sqrtf(dx * dx + dy * dy);
        const float ux = dx / dl, uy = dy / dl;
        const float s1 = fminf(sqrtf(2.0f * l1), 1024.0f), s2 = fminf(sqrtf(2.0f * l2), 1024.0f);
        const float mx = s1 * ux, my = s1 * uy;    // majorAxis
        const float nx = s2 * uy, ny = s2 * -ux;   // minorAxis
        float fade = p2[2] / p2[3] + 1.0f;
        fade = fade < 0.0f ? 0.0f : (fade > 1.0f ? 1.0f : fade);
        const float ndcx = p2[0] / p2[3], ndcy = p2[1] / p2[3];
        const float wcx = (ndcx + 1.0f) * 0.5f * u.W;  // GL window coordinates, y up
        const float wcy = (ndcy + 1.0f) * 0.5f * u.H;
        const float m2 = mx * mx + my * my, n2 = nx * nx + ny * ny;
        const float big = 3.0e38f;
        if (!(m2 > 0.0f) || !(n2 > 0.0f) || !(m2 < big) || !(n2 < big) || !(fabsf(wcx) < big) || !(fabsf(wcy) < big)) drawn = false;
        if (drawn) {
            // pixels whose CENTRE can satisfy |vPosition| <= 2: the bounding box of the ellipse with the orthogonal half-axes m
            // and n (vPosition = (2 d.m/|m|^2, 2 d.n/|n|^2)), i.e. |x + 0.5 - cx| <= sqrt(mx^2 + nx^2), + 1/64 px for the fp32
            // rounding of the per-pixel evaluation (which is good to ~1e-6 of the extent; cx itself to 1.2e-4 px at 1920).
            // (Rounds 1-2 took a whole pixel of slack and floor() on both sides: 1.5 px too wide on every side, i.e. one more
            // tile column or row for every sixth splat - 12 % more (tile, splat) pairs to bin, sort and stage.)
            const float ex = sqrtf(mx * mx + nx * nx) + 0.015625f, ey = sqrtf(my * my + ny * ny) + 0.015625f;
            const float top = u.H - wcy;  // image row coordinate of the centre
            int x0 = (int)ceilf(fminf(fmaxf(wcx - ex - 0.5f, -1.0f), u.W)), x1 = (int)floorf(fminf(fmaxf(wcx + ex - 0.5f, -1.0f), u.W));
            int y0 = (int)ceilf(fminf(fmaxf(top - ey - 0.5f, -1.0f), u.H)), y1 = (int)floorf(fminf(fmaxf(top + ey - 0.5f, -1.0f), u.H));
            x0 = max(x0, 0);
            y0 = max(y0, 0);
            x1 = min(x1, (int)u.W - 1);
            y1 = min(y1, (int)u.H - 1);
            if (x1 >= x0 && y1 >= y0) {
                const uint32_t tx0 = x0 >> 4, tx1 = x1 >> 4, ty0 = y0 >> 4, ty1 = y1 >> 4;
                o.rect = tx0 | (tx1 << 8) | (ty0 << 16) | (ty1 << 24);
                o.r0 = make_float4(wcx, wcy, 2.0f * mx / m2, 2.0f * my / m2);
                o.g1x = 2.0f * nx / n2;
                o.g1y = 2.0f * ny / n2;
                o.fade = fade;
                o.colour = true;
            }
        }
    }
    return o;
}

// the reference's colour: fade * rgba8 / 255 (gs.js:741-742); the SH colour replaces its first three channels
__device__ __forceinline__ float rgba8_channel(const uint4 t1, int k, float fade) { return fade * (float)((t1.w >> (8 * k)) & 0xffu) / 255.0f; }

// One splat in one view, complete (pre_kernel).  The colour is only needed for splats that reach a pixel: 192 B of SH
// coefficients per splat.  (Deferring it further, to the splats a depth phase really bins, was measured: those are visited in
// DEPTH order, the coefficient reads become gathers and cost 9x what the skipped splats save.)
struct PreOut {
    int depth;
    uint32_t rect;
    float4 r0, r1;
    float2 r2;
};

template <bool EDIT, class Coef>
__device__ __forceinline__ PreOut pre_one(const uint4 t0, const uint4 t1, const ViewUniforms& u, bool sh_on, int sh_deg, float cpx,
                                          float cpy, float cpz, const Coef& cf, unsigned code, const EditTables* ep) {
    float ddx = 0.f, ddy = 0.f, ddz = 0.f;
    if (EDIT) edit_displacement(code, *ep, ddx, ddy, ddz);
    // (u_enableDisplacement off: + 0 here where the shader adds nothing - only a -0.0 coordinate could tell, and no output does)
    const PreGeom g = EDIT ? pre_geom<true>(t0, t1, u, ddx, ddy, ddz) : pre_geom(t0, t1, u);
    PreOut o;
    o.depth = g.depth;
    o.rect = g.rect;
    o.r0 = g.r0;
    o.r1 = make_float4(0.f, 0.f, 0.f, 0.f);
    o.r2 = make_float2(0.f, 0.f);
    if (g.colour) {
        float col[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) col[k] = rgba8_channel(t1, k, g.fade);
        if (sh_on) {
            float rgb[3];
            sh_color(cf, sh_deg, __uint_as_float(t0.x), __uint_as_float(t0.y), __uint_as_float(t0.z), cpx, cpy, cpz, rgb);
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = g.fade * rgb[k];
        }
        if (EDIT) edit_colour(col, code, *ep, g.fade);
        o.r1 = make_float4(g.g1x, g.g1y, col[0], col[1]);
        o.r2 = make_float2(col[2], col[3]);
    }
    return o;
}

// workgroup-wide min / max of the depth keys -> one atomic pair per workgroup (same-address atomics serialise in L2)
__device__ __forceinline__ void depth_range_to(int lo, int hi, int* __restrict__ pre, int* slo /*[4]*/, int* shi /*[4]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, __shfl_xor(lo, o));
        hi = max(hi, __shfl_xor(hi, o));
    }
    __syncthreads();  // (the previous view's values have been read)
    if ((threadIdx.x & 63) == 0) {
        slo[threadIdx.x >> 6] = lo;
        shi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(&pre[0], min(min(slo[0], slo[1]), min(slo[2], slo[3])));
        atomicMax(&pre[1], max(max(shi[0], shi[1]), max(shi[2], shi[3])));
    }
}

// One pass over the texel pairs per view.  pre[4] = {min depth, max depth, splat 0's tile rectangle, -}: min / max over ALL
// splats (gs.js:436-441); the rectangle of splat 0 is kept apart because the blend's epilogue draws splat 0 again even when
// bucket_kernel drops it (and clears its entry of tile_rect).
// EDIT: the label edits' instantiation (code: edit_code_kernel's 16 bits per splat); without it the kernel is what it was.
template <bool EDIT>
__global__ __launch_bounds__(kRB) void pre_kernel(const uint4* __restrict__ tex, long long n, ViewUniforms u,
                                                   const float* __restrict__ sh_coef, int sh_deg, float cpx, float cpy, float cpz,
                                                   int* __restrict__ depth, int* __restrict__ pre,
                                                   float4* __restrict__ rec, uint32_t* __restrict__ tile_rect,
                                                   const uint16_t* __restrict__ code, const EditTables* __restrict__ ep) {
    __shared__ int slo[4], shi[4];
    int lo = 2147483647, hi = -2147483647 - 1;
    // grid-stride: the launch is capped at 2048 workgroups, i.e. 4096 same-address atomics per frame (one pair per
    // workgroup of a 12 k-workgroup launch kept the L2 busy for 0.2 ms after the last wave had finished)
    for (long long i = (long long)blockIdx.x * kRB + threadIdx.x; i < n; i += (long long)gridDim.x * kRB) {
        const uint4 t0 = tex[2 * i], t1 = tex[2 * i + 1];
        const CoefMem cf{sh_coef, n, i};
        const PreOut o = pre_one<EDIT>(t0, t1, u, sh_coef != nullptr, sh_deg, cpx, cpy, cpz, cf, EDIT ? (unsigned)code[i] : 0u, ep);
        depth[i] = o.depth;
        lo = min(lo, o.depth);
        hi = max(hi, o.depth);
        if (o.rect != kEmptyRect || i == 0) {  // a record is read only through a list the splat was binned into - and splat 0's by the epilogue
            rec[3 * i] = o.r0;
            rec[3 * i + 1] = o.r1;
            rec[3 * i + 2] = make_float4(o.r2.x, o.r2.y, 0.f, 0.f);
        }
        tile_rect[i] = o.rect;
        if (i == 0) pre[2] = (int)o.rect;
    }
    depth_range_to(lo, hi, pre, slo, shi);
}

// The same for NV views (1 .. kPreViews) in ONE pass over the scene: a splat's texel pair and its SH coefficients (224 B at
// degree 3) are read ONCE - gsx_render_views keeps several frames in flight, and each of them used to stream the whole scene
// again (4 x 816 MB at 3 M splats).  The loop is turned inside out for that: first the geometry of every view (pre_geom, the
// code pre_kernel runs), then one pass over the coefficients in which every view that draws the splat accumulates its own
// colour - three accumulators and a direction per view, the basis function recomputed from the direction when its
// coefficient arrives (sh_basis: the expressions of sh_color).  Per view the operations are pre_kernel's in pre_kernel's
// order, on the same operands: the frames are bit-identical.  (Two earlier forms, both measured: the view loop around
// pre_one with the coefficients re-read through L2 - they had left the 4 MB L2 by the next view, 2.2 GB fetched per 4-view
// launch instead of 0.67 - and with the coefficients held in 48 registers across the views - spills.)
static constexpr int kPreViews = kMaxFrames;
struct PreMultiArgs {
    ViewUniforms u[kPreViews];
    float cam[kPreViews][3];
    int* depth[kPreViews];
    int* pre[kPreViews];
    float4* rec[kPreViews];
    uint32_t* rect[kPreViews];
    int nv;
    // label edits (read by the EDIT instantiations only; behind everything else: the other offsets are what they were)
    const uint16_t* code;
    const EditTables* edits;
};

template <int NV, bool EDIT>
__global__ __launch_bounds__(kRB) void pre_multi_kernel(const uint4* __restrict__ tex, long long n, const float* __restrict__ sh_coef,
                                                         int sh_deg, const PreMultiArgs* __restrict__ ap) {
    // (the arguments live in device memory: the views' uniforms are scalar loads)
    const PreMultiArgs& a = *ap;
    __shared__ int slo[4], shi[4];
    int lo[NV], hi[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) lo[v] = 2147483647, hi[v] = -2147483647 - 1;
    const int K = (sh_deg + 1) * (sh_deg + 1);
    for (long long i = (long long)blockIdx.x * kRB + threadIdx.x; i < n; i += (long long)gridDim.x * kRB) {
        const uint4 t0 = tex[2 * i], t1 = tex[2 * i + 1];
        const float px = __uint_as_float(t0.x), py = __uint_as_float(t0.y), pz = __uint_as_float(t0.z);
        unsigned code = 0u;  // label edits: the splat's code and its displacement, the same for every view
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;
        if (EDIT) {
            code = a.code[i];
            edit_displacement(code, *a.edits, ddx, ddy, ddz);
        }
        // ---- geometry of every view: depth key, rectangle and the first record go out at once; what the colour needs stays
        float g1x[NV], g1y[NV], fade[NV];
        unsigned want = 0;  // bit v: view v wants a colour for this splat
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            // (the pointer is laundered so that a view's 44 uniforms are scalar loads HERE, dead after its vertex shader: hoisted out
            // of the splat loop as invariants, the uniforms of four views are 375 spilled SGPRs)
            const PreMultiArgs* av = ap;
            asm volatile("" : "+s"(av));
            const PreGeom g = EDIT ? pre_geom<true>(t0, t1, av->u[v], ddx, ddy, ddz) : pre_geom(t0, t1, av->u[v]);
            __builtin_nontemporal_store(g.depth, &a.depth[v][i]);  // streaming stores: the records are not read again here
            lo[v] = min(lo[v], g.depth);
            hi[v] = max(hi[v], g.depth);
            // (ordinary stores: the three 16-byte pieces of a record meet in the L2 before they leave it; a splat without a
            // rectangle - two in five on the bench scene - is in no list and writes none: only splat 0's is read regardless, by the epilogue)
            if (g.rect != kEmptyRect || i == 0) a.rec[v][3 * i] = g.r0;
            __builtin_nontemporal_store(g.rect, &a.rect[v][i]);
            if (i == 0) a.pre[v][2] = (int)g.rect;
            g1x[v] = g.g1x, g1y[v] = g.g1y, fade[v] = g.fade;
            want |= g.colour ? 1u << v : 0u;
            __builtin_amdgcn_sched_barrier(0);  // one view after the other: interleaved, the six vertex shaders need 256 VGPRs
        }
        // ---- colour: the coefficients are read ONCE (if any view draws the splat) and every view accumulates its own sum, in
        // sh_color's order: acc = b_0 p_0, then acc += b_k p_k for k = 1 .. K-1, the basis recomputed from the view's direction
        float acc[NV][3], dx[NV], dy[NV], dz[NV];
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            acc[v][0] = acc[v][1] = acc[v][2] = 0.f;
            sh_dir(px, py, pz, a.cam[v][0], a.cam[v][1], a.cam[v][2], dx[v], dy[v], dz[v]);
        }
        if (sh_coef != nullptr && want != 0u) {
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                if (k < K) {
                    float p[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) p[c] = sh_coef[((size_t)k * 3 + c) * (size_t)n + (size_t)i];
#pragma unroll
                    for (int v = 0; v < NV; ++v) {
                        const float b = sh_basis(k, dx[v], dy[v], dz[v]);
#pragma unroll
                        for (int c = 0; c < 3; ++c) acc[v][c] = k == 0 ? b * p[c] : acc[v][c] + b * p[c];
                    }
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            float4 r1 = make_float4(0.f, 0.f, 0.f, 0.f);
            float2 r2 = make_float2(0.f, 0.f);
            if ((want >> v) & 1u) {
                float col[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) col[k] = rgba8_channel(t1, k, fade[v]);
                if (sh_coef != nullptr) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) col[c] = fade[v] * sh_clamp(acc[v][c]);
                }
                if (EDIT) edit_colour(col, code, *a.edits, fade[v]);
                r1 = make_float4(g1x[v], g1y[v], col[0], col[1]);
                r2 = make_float2(col[2], col[3]);
            }
            if (((want >> v) & 1u) || i == 0) {  // (want <=> the view gave the splat a rectangle)
                a.rec[v][3 * i + 1] = r1;
                a.rec[v][3 * i + 2] = make_float4(r2.x, r2.y, 0.f, 0.f);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) depth_range_to(lo[v], hi[v], a.pre[v], slo, shi);
}

// 16-bit depth bucket (gs.js:443-447) once the depth range is known; doubles as the (key, value) initialisation of the
// level-1 sort.  The JS's typed arrays silently drop a bucket outside [0, 65535] (the farthest splat always gets
// 65536): such a splat is never drawn, it sorts to the end and loses its tile rectangle here.
__global__ __launch_bounds__(kRB) void bucket_kernel(const int* __restrict__ depth, long long n, const int* __restrict__ minmax,
                                                      uint32_t* __restrict__ bucket, uint32_t* __restrict__ key,
                                                      uint32_t* __restrict__ idx, uint32_t* __restrict__ tile_rect,
                                                      int* __restrict__ dropped, int compact) {
    const long long i = (long long)blockIdx.x * kRB + threadIdx.x;
    bool drop = false;
    if (i < n) {
        const double minDepth = (double)minmax[0], maxDepth = (double)minmax[1];
        const double depthInv = (256.0 * 256.0) / (maxDepth - minDepth);
        const int b = js_toint32(((double)depth[i] - minDepth) * depthInv);
        const bool in_range = b >= 0 && b < 65536;
        const uint32_t v = in_range ? (uint32_t)b : 65536u;
        bucket[i] = v;
        // 16-bit sort key: a dropped splat covers no tile, where it sorts does not matter.  compact: a splat that covers no tile
        // (dropped, or without a rectangle in this view: behind the camera, off the frame, between the pixel centres) gets the
        // key the level-1 sort leaves out (radix_sort_pairs_drop) - the bin kernels then see the others only, in their order
        const bool seen = in_range && tile_rect[i] != kEmptyRect;
        key[i] = compact ? (seen ? v : 0xffffffffu) : (in_range ? v : 65535u);
        idx[i] = (uint32_t)i;
        drop = !in_range;
        if (drop) tile_rect[i] = kEmptyRect;
    }
    const unsigned long long m = __ballot(drop);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(dropped, (int)__popcll(m));
}

static const int kPreInit[4] = {2147483647, -2147483647 - 1, (int)kEmptyRect, 0};  // depth min / max, splat 0's rectangle (static: outlives the copy)

int ensure_pre_set(Ctx* c, PreSet& ps, long long n) {
    const size_t n4 = 4 * (size_t)n;
    GSX_HIP(c, ps.depth.ensure(n4));
    GSX_HIP(c, ps.rect.ensure(n4));
    GSX_HIP(c, ps.rec.ensure(48 * (size_t)n));
    GSX_HIP(c, ps.pre.ensure(16));
    return GSX_OK;
}

static ViewUniforms view_uniforms(const gsx_camera* cam, int W, int H) {
    ViewUniforms u{};
    double view[16], proj[16], vp[16];
    js_view_matrix(cam, view);
    js_proj_matrix(cam->fx, cam->fy, (double)W, (double)H, proj);
    js_multiply4(proj, view, vp);
    u.vp2 = vp[2];
    u.vp6 = vp[6];
    u.vp10 = vp[10];
    for (int k = 0; k < 16; ++k) {  // gl.uniformMatrix4fv: JS numbers -> f32
        u.view[k] = (float)view[k];
        u.proj[k] = (float)proj[k];
    }
    u.fx = (float)cam->fx;
    u.fy = (float)cam->fy;
    u.W = (float)W;
    u.H = (float)H;
    u.tiles_x = (W + 15) / 16;
    u.tiles_y = (H + 15) / 16;
    return u;
}

// ---- the launches of the per-splat pre pass (one place: gsx_ctx.hpp) ----
static unsigned pre_grid(long long n) { return std::min<unsigned>(grid_for(n), 2048u); }

// one view: pre[] is reset, then pre_kernel writes depth[n], rect[n], rec[3n] (where it writes a record at all) and pre[0..2]
int launch_pre(Ctx* c, const gsx_camera* cam, int W, int H, const PreSet& to) {
    const RenderScene& s = c->scene;
    const ViewUniforms u = view_uniforms(cam, W, H);
    int* pre = to.pre.as<int>();
    GSX_HIP(c, hipMemcpyAsync(pre, kPreInit, sizeof kPreInit, hipMemcpyHostToDevice, c->stream));
    ProfScope ps(c, "render_pre");
    hipLaunchKernelGGL(s.edits_on ? pre_kernel<true> : pre_kernel<false>, dim3(pre_grid(s.rn)), dim3(kRB), 0, c->stream,
                       s.tex.as<uint4>(), (long long)s.rn, u, s.sh_on ? s.shc.as<float>() : nullptr, s.sh_deg, (float)cam->p[0],
                       (float)cam->p[1], (float)cam->p[2], to.depth.as<int>(), pre, to.rec.as<float4>(), to.rect.as<uint32_t>(),
                       s.edits_on ? s.edit_code.as<uint16_t>() : (const uint16_t*)nullptr,
                       s.edits_on ? s.edit_tab.as<EditTables>() : (const EditTables*)nullptr);
    return GSX_OK;
}

// nv views (1 .. kPreViews) in one launch of pre_multi_kernel: view v writes into *sets[v].  The arguments go through slot `slot`
// of r_pre_args; their host copy lives in the context too, one slot per record set, because the asynchronous copy may read it
// after this function has returned (gsx_render_views rewrites a slot three groups later)
int launch_pre_multi(Ctx* c, int nv, const gsx_camera* cams, int W, int H, PreSet* const* sets, int slot) {
    GSX_HIP(c, c->r_pre_args.ensure(sizeof(PreMultiArgs) * kPreSets));
    c->r_pre_args_host.resize((sizeof(PreMultiArgs) * kPreSets + 7) / 8);
    PreMultiArgs& a = reinterpret_cast<PreMultiArgs*>(c->r_pre_args_host.data())[slot];
    PreMultiArgs* a_dev = c->r_pre_args.as<PreMultiArgs>() + slot;
    const RenderScene& s = c->scene;
    a = PreMultiArgs{};
    a.nv = nv;
    for (int v = 0; v < nv; ++v) {
        const gsx_camera* cam = cams + v;
        PreSet& ps = *sets[v];
        a.u[v] = view_uniforms(cam, W, H);
        for (int k = 0; k < 3; ++k) a.cam[v][k] = (float)cam->p[k];
        a.depth[v] = ps.depth.as<int>();
        a.pre[v] = ps.pre.as<int>();
        a.rec[v] = ps.rec.as<float4>();
        a.rect[v] = ps.rect.as<uint32_t>();
        a.code = s.edits_on ? s.edit_code.as<uint16_t>() : nullptr;
        a.edits = s.edits_on ? s.edit_tab.as<EditTables>() : nullptr;
        GSX_HIP(c, hipMemcpyAsync(ps.pre.p, kPreInit, sizeof kPreInit, hipMemcpyHostToDevice, c->stream));
    }
    GSX_HIP(c, hipMemcpyAsync(a_dev, &a, sizeof a, hipMemcpyHostToDevice, c->stream));
    using PK = void (*)(const uint4*, long long, const float*, int, const PreMultiArgs*);
    static const PK kernels[2][kPreViews] = {
        {pre_multi_kernel<1, false>, pre_multi_kernel<2, false>, pre_multi_kernel<3, false>, pre_multi_kernel<4, false>,
         pre_multi_kernel<5, false>, pre_multi_kernel<6, false>},
        {pre_multi_kernel<1, true>, pre_multi_kernel<2, true>, pre_multi_kernel<3, true>, pre_multi_kernel<4, true>,
         pre_multi_kernel<5, true>, pre_multi_kernel<6, true>}};  // [1]: the label edits' instantiations
    static_assert(kPreViews == 6, "one instantiation per group size");
    hipLaunchKernelGGL(kernels[s.edits_on ? 1 : 0][nv - 1], dim3(pre_grid(s.rn)), dim3(kRB), 0, c->stream, s.tex.as<uint4>(),
                       (long long)s.rn, s.sh_on ? s.shc.as<float>() : nullptr, s.sh_deg, a_dev);
    GSX_HIP(c, hipGetLastError());
    return GSX_OK;
}

// depth buckets and level-1 sort keys of one view from its depth keys and range; dropped splats lose their rectangle
void launch_bucket(Ctx* c, const PreSet& ps, uint32_t* bucket, uint32_t* key, uint32_t* idx, int* dropped, int compact) {
    ProfScope scope(c, "render_bucket");
    hipLaunchKernelGGL(bucket_kernel, dim3(grid_for(c->scene.rn)), dim3(kRB), 0, c->stream, ps.depth.as<int>(), (long long)c->scene.rn,
                       ps.pre.as<int>(), bucket, key, idx, ps.rect.as<uint32_t>(), dropped, compact);
}

// gsx_debug_render_pre: the product's pre pass (launch_pre per view, or ONE launch_pre_multi) and bucket_kernel into buffers
// of the call's own - the context's record sets, its frame buffers and its counters are not touched
int debug_render_pre(Ctx* c, int nv, const gsx_camera* cams, int W, int H, int multi, int compact, const gsx_debug_pre_view* out) {
    GSX_HIP(c, hipSetDevice(c->device));
    if (nv < 1 || nv > kPreViews || !cams || !out || W < 1 || H < 1) return fail(c, GSX_E_INVALID, "debug_render_pre: bad arguments");
    if ((W + 15) / 16 > 256 || (H + 15) / 16 > 256) return fail(c, GSX_E_UNSUPPORTED, "debug_render_pre: %dx%d exceeds 4096 pixels per side", W, H);
    const long long n = c->scene.rn;
    if (n <= 0) return fail(c, GSX_E_STATE, "debug_render_pre before upload_splats");
    const size_t n4 = 4 * (size_t)n;
    PreSet sets[kPreViews];
    PreSet* setp[kPreViews];
    DevBuf bucket, key, idx, dropped;
    for (int v = 0; v < nv; ++v) {
        const int rc = ensure_pre_set(c, sets[v], n);
        if (rc) return rc;
        setp[v] = &sets[v];
        // sentinel: what the pass does not write stays 0xFF bytes
        GSX_HIP(c, hipMemsetAsync(sets[v].depth.p, 0xFF, n4, c->stream));
        GSX_HIP(c, hipMemsetAsync(sets[v].rect.p, 0xFF, n4, c->stream));
        GSX_HIP(c, hipMemsetAsync(sets[v].rec.p, 0xFF, 48 * (size_t)n, c->stream));
    }
    GSX_HIP(c, bucket.ensure(n4));
    GSX_HIP(c, key.ensure(n4));
    GSX_HIP(c, idx.ensure(n4));
    GSX_HIP(c, dropped.ensure(sizeof(int)));
    int rc = GSX_OK;
    if (multi) {
        rc = launch_pre_multi(c, nv, cams, W, H, setp, 0);
    } else {
        for (int v = 0; v < nv && rc == GSX_OK; ++v) rc = launch_pre(c, cams + v, W, H, sets[v]);
        if (rc == GSX_OK) GSX_HIP(c, hipGetLastError());
    }
    for (int v = 0; v < nv && rc == GSX_OK; ++v) {
        const gsx_debug_pre_view& o = out[v];
        PreSet& ps = sets[v];
        if (o.depth) GSX_HIP(c, hipMemcpyAsync(o.depth, ps.depth.p, n4, hipMemcpyDeviceToHost, c->stream));
        if (o.rect) GSX_HIP(c, hipMemcpyAsync(o.rect, ps.rect.p, n4, hipMemcpyDeviceToHost, c->stream));
        if (o.rec) GSX_HIP(c, hipMemcpyAsync(o.rec, ps.rec.p, 48 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        if (o.pre) GSX_HIP(c, hipMemcpyAsync(o.pre, ps.pre.p, 16, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipMemsetAsync(dropped.p, 0, sizeof(int), c->stream));
        launch_bucket(c, ps, bucket.as<uint32_t>(), key.as<uint32_t>(), idx.as<uint32_t>(), dropped.as<int>(), compact);
        GSX_HIP(c, hipGetLastError());
        if (o.bucket) GSX_HIP(c, hipMemcpyAsync(o.bucket, bucket.p, n4, hipMemcpyDeviceToHost, c->stream));
        if (o.key) GSX_HIP(c, hipMemcpyAsync(o.key, key.p, n4, hipMemcpyDeviceToHost, c->stream));
        if (o.rect_bucket) GSX_HIP(c, hipMemcpyAsync(o.rect_bucket, ps.rect.p, n4, hipMemcpyDeviceToHost, c->stream));
        if (o.dropped) GSX_HIP(c, hipMemcpyAsync(o.dropped, dropped.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));  // (a view's outputs are on the host before the next view reuses bucket / key / dropped)
    }
    GSX_HIP(c, hipStreamSynchronize(c->stream));  // nothing of this call is in flight when its buffers are freed
    return rc;
}

}  // namespace gsx
