// vote_device.hpp — what the labeler kernels of vote.hip and the map kernels of handover.hip share: the block size, and the
// fp64 projection + seg-map addressing every labeler kernel inlines (project() restates project_gaussian,
// deep_learning_segmentation.py:43-82, operation for operation).
// Include this header ONLY from .hip files compiled with -ffp-contract=off: every fma below is explicit and every other
// product/sum must round separately, exactly as the reference's Python floats do.
#pragma once
#include <hip/hip_runtime.h>

#include "gsx_ctx.hpp"

namespace gsx {

static constexpr int kBlock = 256;
static constexpr int kMaxBatch = 255;  // views per fused launch: LDS counters are 8 bit
static inline unsigned grid_for(long long n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// -------------------------------------------------------------------------------------------------
// device: project_gaussian + seg-map addressing
// -------------------------------------------------------------------------------------------------
// One view's hot fields, held in SGPRs.  load_view() pins all of them behind ONE batch of scalar loads: left
// to itself hipcc sinks every s_load next to its first use, behind the early-out branches, and each view
// then pays ~5 exposed scalar-cache round trips (the kernel was waiting, not computing).
struct ViewRegs {
    double R[9], t[3], fx, fy, half_w, half_h, width, height;
    long long seg_off;
    int seg_w, unit_scale, seg_row_bytes, cam_w, cam_h;
    int coarse_row_bytes;
    unsigned coarse_delta;
    float hw32, hh32;
};

typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v2i __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double chunk_f64(const v16i& v, int k) {
    v2i t;
    t.x = v[2 * k];
    t.y = v[2 * k + 1];
    return __builtin_bit_cast(double, t);
}

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));
// The hot 184 bytes of a ViewDesc as four scalar loads (x16, x16, x8, x8), pinned as whole register tuples: the
// fields below are sub-registers of those tuples, no scalar move is spent on them.  (Pinning the 24 fields one
// by one cost 15 s_mov per view; the scalar unit is shared by the four SIMDs of a CU and every wave issues at
// most one instruction per turn, so scalar bookkeeping was costing as much as the fp64 arithmetic.)
__device__ __forceinline__ void unpack_core(ViewRegs& r, const v16i& a, const v16i& b) {
#pragma unroll
    for (int k = 0; k < 8; ++k) r.R[k] = chunk_f64(a, k);
    r.R[8] = chunk_f64(b, 0);
#pragma unroll
    for (int k = 0; k < 3; ++k) r.t[k] = chunk_f64(b, 1 + k);
    r.fx = chunk_f64(b, 4);
    r.fy = chunk_f64(b, 5);
    r.seg_off = __builtin_bit_cast(long long, chunk_f64(b, 6));
    r.seg_row_bytes = b[14];
    r.unit_scale = b[15];
}

__device__ __forceinline__ ViewRegs load_view(const ViewDesc* __restrict__ vp) {
    static_assert(offsetof(ViewDesc, R) == 0 && offsetof(ViewDesc, t) == 72 && offsetof(ViewDesc, fx) == 96 &&
                      offsetof(ViewDesc, seg_off) == 112 && offsetof(ViewDesc, seg_row_bytes) == 120 &&
                      offsetof(ViewDesc, unit_scale) == 124 && offsetof(ViewDesc, half_w) == 128 &&
                      offsetof(ViewDesc, width) == 144 && offsetof(ViewDesc, seg_w) == 160 &&
                      offsetof(ViewDesc, cam_w) == 168 && offsetof(ViewDesc, coarse_row_bytes) == 176 &&
                      offsetof(ViewDesc, coarse_delta) == 180 && offsetof(ViewDesc, hw32) == 184 && sizeof(ViewDesc) % 64 == 0,
                  "load_view reads the hot part of ViewDesc as 64 + 64 + 32 + 32 bytes");
    const char* q = reinterpret_cast<const char*>(vp);
    v16i a = *reinterpret_cast<const v16i*>(q);
    v16i b = *reinterpret_cast<const v16i*>(q + 64);
    v8i c = *reinterpret_cast<const v8i*>(q + 128);
    v8i d = *reinterpret_cast<const v8i*>(q + 160);
    asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d));
    ViewRegs r;
    unpack_core(r, a, b);
    v2i t;
    t.x = c[0], t.y = c[1];
    r.half_w = __builtin_bit_cast(double, t);
    t.x = c[2], t.y = c[3];
    r.half_h = __builtin_bit_cast(double, t);
    t.x = c[4], t.y = c[5];
    r.width = __builtin_bit_cast(double, t);
    t.x = c[6], t.y = c[7];
    r.height = __builtin_bit_cast(double, t);
    r.seg_w = d[0];
    r.cam_w = d[2];
    r.cam_h = d[3];
    r.coarse_row_bytes = d[4];
    r.coarse_delta = (unsigned)d[5];
    const int hw_bits = d[6], hh_bits = d[7];  // (a bit_cast straight from a vector element reads element 0)
    r.hw32 = __builtin_bit_cast(float, hw_bits);
    r.hh32 = __builtin_bit_cast(float, hh_bits);
    return r;
}

// OpenBLAS dgemv association of `R @ v` for a C-contiguous 3x3 (oracle/vote_oracle.c, header)
__device__ __forceinline__ double row_dot(const double* Rr, double v0, double v1, double v2) {
    return __builtin_fma(Rr[2], v2, __builtin_fma(Rr[0], v0, Rr[1] * v1));
}

// project_gaussian (dls.py:43-82).  Returns false where the reference returns None (:72-73, :80-82).
//
// DIV == kDivExact: the two IEEE-754 divisions of dls.py:76-77, operation for operation.
// (A certified form, the same results from ONE reciprocal, option "fast_div", was measured and removed: DESIGN.md.)
// DIV == kDivFlat: the exact divisions again, but as ONE straight-line block: all three rows and both quotients are
//   evaluated unconditionally and the reference's tests (:72, :80) become a single predicate at the end.  The
//   branchy form serialises ~45 dependent fp64 instructions behind three divergent branches; here the three rows
//   and the two quotients are independent chains the scheduler interleaves.  Same operations, same operands,
//   same results; lanes the reference rejects early merely compute values nobody reads.
// DIV == kDivFlatSimple: kDivFlat for a batch whose views ALL have unit scale and tiled maps (the host checks): the
//   two wave-uniform tests per view disappear from the instruction stream.
// DIV == kDivFlatCoarse: kDivFlatSimple for a batch whose maps all carry a coarse level (see gather_chunk).
// DIV == kDivFiltCoarse: kDivFlatCoarse with the fp32 filter of project_filtered() in front of the two divisions.
enum { kDivExact = 0, kDivFlat = 1, kDivFlatSimple = 2, kDivFlatCoarse = 3, kDivFiltCoarse = 4 };

// Two IEEE-754 divisions by the same denominator, bit-identical to `ax / b` and `ay / b`.
// hipcc expands an fp64 division into div_scale(den), rcp, two Newton steps, div_scale(num), mul, fma, div_fmas,
// div_fixup.  Everything up to the refined reciprocal depends only on the SCALED denominator, which is the same
// for both quotients unless v_div_scale rescales for an extreme exponent gap; so the reciprocal chain (v_rcp_f64,
// which costs as much as 3.4 fp64 FMAs on gfx950, plus 4 FMAs) is evaluated once.  Lanes whose two scaled
// denominators differ redo the second quotient with the plain division (extreme-exponent tests only).
__device__ __forceinline__ void div2_shared(double ax, double ay, double b, double& qx, double& qy) {
    bool unused, vx, vy;
    const double sdx = __builtin_amdgcn_div_scale(ax, b, false, &unused);
    const double sdy = __builtin_amdgcn_div_scale(ay, b, false, &unused);
    const double nsd = -sdx;
    double r = __builtin_amdgcn_rcp(sdx);
    r = __builtin_fma(r, __builtin_fma(nsd, r, 1.0), r);
    r = __builtin_fma(r, __builtin_fma(nsd, r, 1.0), r);
    const double snx = __builtin_amdgcn_div_scale(ax, b, true, &vx);
    const double mx = snx * r;
    qx = __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(nsd, mx, snx), r, mx, vx), b, ax);
    const double sny = __builtin_amdgcn_div_scale(ay, b, true, &vy);
    const double my = sny * r;
    qy = __builtin_amdgcn_div_fixup(__builtin_amdgcn_div_fmas(__builtin_fma(nsd, my, sny), r, my, vy), b, ay);
    // wave-uniform test on purpose: behind a per-lane `if` the compiler turns the fallback into a select and
    // evaluates the second reciprocal chain unconditionally
    const bool differ = __double_as_longlong(sdx) != __double_as_longlong(sdy);
    if (__builtin_expect(__builtin_amdgcn_ballot_w64(differ) != 0, 0)) {
        const double slow = ay / b;
        qy = differ ? slow : qy;
    }
}

template <int DIV>
__device__ __forceinline__ bool project(const ViewRegs& vd, double X, double Y, double Z, int& xi, int& yi) {
    const double pc2 = row_dot(vd.R + 6, X, Y, Z) + vd.t[2];
    if (DIV == kDivFlat || DIV == kDivFlatSimple || DIV == kDivFlatCoarse) {
        // one wave-uniform early-out keeps what matters of the branchy form: a wave whose 64 Gaussians are all
        // behind the camera (Morton order makes that the common way to be culled) skips the view
        if (__builtin_amdgcn_ballot_w64(pc2 > 0.0) == 0) return false;
        const double q0 = row_dot(vd.R + 0, X, Y, Z) + vd.t[0];
        const double q1 = row_dot(vd.R + 3, X, Y, Z) + vd.t[1];
        double qx, qy;
        div2_shared(vd.fx * q0, vd.fy * q1, pc2, qx, qy);
        const double fpx = qx + vd.half_w;  // dls.py:76
        const double fpy = qy + vd.half_h;  // dls.py:77
        const bool vis = (pc2 > 0.0) & (0.0 <= fpx) & (fpx < vd.width) & (0.0 <= fpy) & (fpy < vd.height);  // :72, :80
        if (!vis) return false;
        xi = (int)fpx;  // :81
        yi = (int)fpy;
        return true;
    }
    if (!(pc2 > 0.0)) return false;  // `pc2 <= 0` -> None; a NaN depth fails the bounds test below anyway
    const double pc0 = row_dot(vd.R + 0, X, Y, Z) + vd.t[0];
    const double pc1 = row_dot(vd.R + 3, X, Y, Z) + vd.t[1];
    const double ax = vd.fx * pc0, ay = vd.fy * pc1;
    const double px = ax / pc2 + vd.half_w;  // dls.py:76
    const double py = ay / pc2 + vd.half_h;  // dls.py:77
    if (!((0.0 <= px) && (px < vd.width) && (0.0 <= py) && (py < vd.height))) return false;  // :80
    xi = (int)px;  // int() truncation, :81
    yi = (int)py;
    return true;
}

// ---- filtered exact projection ------------------------------------------------------------------------------------------
// project<kDivFlatSimple>() spends two thirds of its time on the two IEEE-754 divisions of dls.py:76-77 (v_div_scale, v_rcp_f64,
// two Newton steps, v_div_fmas, v_div_fixup: ~43 ns of ~95 per wave and view, tools/valu_rate.hip) to obtain px, py to the last
// bit - of which only floor() and the comparison with the frame are ever used.  Here the camera-space point (pc0, pc1, pc2) and
// the products ax = fx * pc0, ay = fy * pc1 are the reference's own fp64 values as before, but the perspective division runs
// in fp32: one v_rcp_f32 and two v_fma_f32 give px^, py^ with a PROVEN error bound E, and a lane whose px^ and py^ are both
// farther than E from every integer has floor(px^) == floor(px), floor(py^) == floor(py) for certain - which decides the
// visibility test (an integer frame: 0 <= px < W  <=>  0 <= floor(px) <= W - 1) and the pixel.  If any lane of the wave is
// closer than that to an integer (or its depth lies outside [2^-40, 2^40)), the whole wave takes the exact divisions for
// this view behind a wave-uniform branch: ~4 E of the lanes, i.e. one (wave, view) pair in ten at 1080p.  Bit-exact by
// construction; the bound:
//   u = 2^-24.  a^ = fl32(a) = a (1 + e1), z^ = fl32(pc2) = pc2 (1 + e2), |e1|, |e2| <= u (round to nearest; pc2 in
//   [2^-40, 2^40) keeps z^ and r^ normal, and the 2^-126 absolute error of an a below the normal range is < 2^-86 after the
//   multiplication by r^ <= 2^40); r^ = v_rcp_f32(z^) = (1 + e3) / z^ with |e3| <= 3 u (1 ulp by the ISA manual; the
//   exhaustive check gsx_debug_filter_check() measures it on the device, and the GPU suite asserts <= 3 u);
//   px^ = fl32(a^ r^ + hw) (fused, hw = W / 2 exact in fp32) = (a^ r^ + hw)(1 + e4), |e4| <= u.  With P = a / pc2 + hw:
//   |px^ - P| <= |P - hw| ((1 + u)(1 + 3u) / (1 - u) - 1) + u |px^| / (1 - u) <= 5.01 u |P - hw| + 1.01 u |px^|.
//   The reference's px = fl64(fl64(a / pc2) + hw) differs from P by <= 2^-52 (|P| + hw).
//   Inside or within one pixel of the frame, |P - hw| <= W / 2 + 1 and |px^| <= W + 1:  |px^ - px| < 3.6 W u.
//   E = 4 D u (kFilterK; D = the larger side of the largest frame of the batch, at least 64) leaves 10 % - 0.4 D u >= 2^-20 -
//   for the terms dropped above (a few u) and for the rounding of fract() on (-1, 0) and of `fract - 0.5` (<= 2^-25 each).
//   Outside that band no bound is needed: a lane is declared invisible only when floor(px^) lies outside [0, W - 1] while
//   px^ is at least E away from the integers, and then P is on the same side of the frame (for px^ >= W + 1 or px^ <= -1
//   the relative error 6.02 u cannot move P across the frame edge; between, the bound above applies); infinities saturate
//   the conversion and fail the range test, NaNs fail the comparison with E and send the wave to the exact path.
static constexpr double kFilterK = 4.0;
__device__ __forceinline__ int cvt_floor_i32(float v) {
    int k;
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(k) : "v"(v));  // floor + saturating conversion in one instruction (NaN -> 0)
    return k;
}

// filt_h = 0.5 - E.  Returns what project<kDivFlatSimple>() returns, bit for bit.
__device__ __forceinline__ bool project_filtered(const ViewRegs& vd, float filt_h, double X, double Y, double Z, int& xi, int& yi) {
    const double pc2 = row_dot(vd.R + 6, X, Y, Z) + vd.t[2];
    const bool pos = pc2 > 0.0;  // dls.py:72
    if (__builtin_amdgcn_ballot_w64(pos) == 0) return false;
    const double q0 = row_dot(vd.R + 0, X, Y, Z) + vd.t[0];
    const double q1 = row_dot(vd.R + 3, X, Y, Z) + vd.t[1];
    const double ax = vd.fx * q0, ay = vd.fy * q1;
    {
        const float zf = (float)pc2, axf = (float)ax, ayf = (float)ay;
        const float r = __builtin_amdgcn_rcpf(zf);
        const float pxf = __builtin_fmaf(axf, r, vd.hw32), pyf = __builtin_fmaf(ayf, r, vd.hh32);
        const float dx = __builtin_amdgcn_fractf(pxf) - 0.5f, dy = __builtin_amdgcn_fractf(pyf) - 0.5f;
        // 2^-40 <= pc2 < 2^40, on the high word (a negative, zero, infinite or NaN depth fails)
        const bool zrange = (unsigned)(__double2hiint(pc2) - 0x3D700000) < (unsigned)(0x42700000 - 0x3D700000);
        const bool cert = zrange & (__builtin_fabsf(dx) <= filt_h) & (__builtin_fabsf(dy) <= filt_h);  // false for NaN
        const int kx = cvt_floor_i32(pxf), ky = cvt_floor_i32(pyf);
        if (__builtin_expect(__builtin_amdgcn_ballot_w64(pos & !cert) == 0, 1)) {
            xi = kx;
            yi = ky;
            return cert & ((unsigned)kx < (unsigned)vd.cam_w) & ((unsigned)ky < (unsigned)vd.cam_h);
        }
    }
    // some lane is too close to a pixel boundary: the exact divisions for the whole wave (dls.py:76-81)
    double qx, qy;
    div2_shared(ax, ay, pc2, qx, qy);
    const double fpx = qx + vd.half_w, fpy = qy + vd.half_h;
    const bool vis = pos & (0.0 <= fpx) & (fpx < vd.width) & (0.0 <= fpy) & (fpy < vd.height);
    if (!vis) return false;
    xi = (int)fpx;
    yi = (int)fpy;
    return true;
}

// The vote of one Gaussian in one view: the map byte (bin = label + 1) under its projection, or -1 where the
// reference skips the pair (dls.py:278-279).  All in-map offsets are 32-bit (maps are <= 65535 x 65535, checked in
// vote_view), added to the view's wave-uniform base pointer: the gather is `global_load_ubyte v, v_off, s[base]`.
template <int DIV>
__device__ __forceinline__ int seg_bin_regs(const ViewRegs& vd, const ViewDesc* __restrict__ vp,
                                            const uint8_t* __restrict__ pool, double X, double Y, double Z) {
    int xi, yi;
    int bin = -1;
    if (project<DIV>(vd, X, Y, Z, xi, yi)) {
        constexpr bool kSimple = DIV == kDivFlatSimple;
        if (!kSimple && !vd.unit_scale) {
            const double xs = trunc((double)xi * vp->wscale);  // :281
            const double ys = trunc((double)yi * vp->hscale);  // :282
            const int seg_h = vp->seg_h;
            xi = xs > (double)(vd.seg_w - 1) ? vd.seg_w - 1 : (int)xs;  // :285 (xs >= 0 always)
            yi = ys > (double)(seg_h - 1) ? seg_h - 1 : (int)ys;        // :286
        }
        unsigned off;
        if (kSimple || vd.seg_row_bytes) {
            // strips of 16 pixel columns, rows of a strip back to back (16 B each): any 8 consecutive rows of a strip
            // are one 128-B line, so a compact patch of pixels is a compact set of cache lines, and the offset is
            // (xi>>4) * strip_bytes + (yi<<4) + (xi&15): four integer instructions
            off = __umul24((unsigned)xi >> 4, (unsigned)vd.seg_row_bytes) + ((unsigned)xi & 15u) + ((unsigned)yi << 4);
        } else {
            off = __umul24((unsigned)yi, (unsigned)vd.seg_w) + (unsigned)xi;
        }
        // the device copy of the descriptor holds the map's absolute address; say "global" explicitly, a pointer made
        // from an integer would otherwise be a FLAT one (flat loads also count in lgkmcnt and stall the scalar waits)
        typedef const __attribute__((address_space(1))) uint8_t* global_u8;
        bin = ((global_u8)(unsigned long long)vd.seg_off)[off];
    }
    return bin;
}

template <int DIV>
__device__ __forceinline__ int seg_bin(const ViewDesc* __restrict__ vp, const uint8_t* __restrict__ pool, double X, double Y,
                                       double Z) {
    const ViewRegs vd = load_view(vp);
    return seg_bin_regs<DIV>(vd, vp, pool, X, Y, Z);
}

// Workgroups b and b+8 run on the same XCD (round-robin dispatch; a speed heuristic, never needed for
// correctness).  swizzle == 1: XCD x takes the x-th contiguous eighth of the Morton curve.  swizzle == C >= 2: the
// curve is cut into chunks of C workgroups and chunk k goes to XCD k % 8: an XCD still works on compact pieces
// of space (its L2 serves compact patches of every segmentation map), but every XCD sees every part of the scene, so
// the eight of them finish together even when visibility differs from one region to the next.  Bijective for any grid.
__device__ __forceinline__ unsigned logical_block(unsigned b, unsigned nwg, int swizzle) {
    if (!swizzle) return b;
    if (swizzle == 1) {
        const unsigned q = nwg >> 3, r = nwg & 7u, xcd = b & 7u;
        return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (b >> 3);
    }
    const unsigned C = (unsigned)swizzle, super = 8u * C;
    if (b >= nwg / super * super) return b;  // the ragged tail keeps its order
    const unsigned j = b >> 3;
    return (j / C) * super + (b & 7u) * C + j % C;
}

}  // namespace gsx
