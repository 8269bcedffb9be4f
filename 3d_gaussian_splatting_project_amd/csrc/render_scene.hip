// render_scene.hip - what the rasterizer keeps once per scene (RenderScene): the upload (processPlyBuffer gs.js:513-582 in fp64
// like JS numbers, generateTexture gs.js:301-354 with 4*Sigma as truncated fp16), the label edits' codes and the hit test
// (performHitTesting gs.js:361-395).  Compiled with -ffp-contract=off: JS never fuses.
//
// HBM layout
//   tex        uint4[2n]   the viewer's RGBA32UI texel pairs: [x y z label][h01 h23 h45 rgba8], importance order
//   buffer     u8[32n]     the viewer's .splat rows (pos, exp(scale), rgba8, quat8)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "gsx_ctx.hpp"
#include "render_device.hpp"

namespace gsx {

// ---- pack: processPlyBuffer + generateTexture --------------------------------------------------------
// importance (gs.js:520-522) as a sort key: ascending ~bits == descending float (values are >= 0)
__global__ __launch_bounds__(kRB) void splat_importance_kernel(const float* __restrict__ scale,
                                                                const float* __restrict__ opacity, long long n,
                                                                uint32_t* __restrict__ key, uint32_t* __restrict__ idx) {
    const long long r = (long long)blockIdx.x * kRB + threadIdx.x;
    if (r >= n) return;
    const double size = exp((double)scale[3 * r]) * exp((double)scale[3 * r + 1]) * exp((double)scale[3 * r + 2]);
    const double op = 1.0 / (1.0 + exp(-(double)opacity[r]));
    const float imp = (float)(size * op);  // Float32Array store
    key[r] = ~__float_as_uint(imp);
    idx[r] = (uint32_t)r;
}

__global__ __launch_bounds__(kRB) void iota_kernel(uint32_t* __restrict__ idx, long long n) {
    const long long r = (long long)blockIdx.x * kRB + threadIdx.x;
    if (r < n) idx[r] = (uint32_t)r;
}

__global__ __launch_bounds__(kRB) void splat_pack_kernel(const uint32_t* __restrict__ order, long long n,
                                                          const float* __restrict__ xyz, const float* __restrict__ scale,
                                                          const float* __restrict__ rot, const float* __restrict__ opacity,
                                                          const float* __restrict__ f_dc, const int* __restrict__ labels,
                                                          uint4* __restrict__ buffer /*2 per splat*/,
                                                          uint4* __restrict__ tex /*2 per splat*/) {
    const long long j = (long long)blockIdx.x * kRB + threadIdx.x;
    if (j >= n) return;
    const long long r = order[j];
    const float px = xyz[3 * r], py = xyz[3 * r + 1], pz = xyz[3 * r + 2];
    float sc[3];
    unsigned q[4];
    if (scale) {
        const double r0 = rot[4 * r], r1 = rot[4 * r + 1], r2 = rot[4 * r + 2], r3 = rot[4 * r + 3];
        const double qlen = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);  // gs.js:549
        q[0] = js_u8clamp((r0 / qlen) * 128.0 + 128.0);
        q[1] = js_u8clamp((r1 / qlen) * 128.0 + 128.0);
        q[2] = js_u8clamp((r2 / qlen) * 128.0 + 128.0);
        q[3] = js_u8clamp((r3 / qlen) * 128.0 + 128.0);
        sc[0] = (float)exp((double)scale[3 * r]);
        sc[1] = (float)exp((double)scale[3 * r + 1]);
        sc[2] = (float)exp((double)scale[3 * r + 2]);
    } else {  // gs.js:559-563
        sc[0] = sc[1] = sc[2] = (float)0.01;
        q[0] = 255u;
        q[1] = q[2] = q[3] = 0u;
    }
    const double SH_C0 = 0.28209479177387814;
    unsigned c[4];
    for (int k = 0; k < 3; ++k) c[k] = js_u8clamp((0.5 + SH_C0 * (double)f_dc[3 * r + k]) * 255.0);  // gs.js:567-569
    c[3] = opacity ? js_u8clamp((1.0 / (1.0 + exp(-(double)opacity[r]))) * 255.0) : 255u;           // gs.js:576
    const unsigned rgba = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    const unsigned quat = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
    buffer[2 * j] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), __float_as_uint(sc[0]));
    buffer[2 * j + 1] = make_uint4(__float_as_uint(sc[1]), __float_as_uint(sc[2]), rgba, quat);

    // generateTexture, gs.js:322-353: covariance from the QUANTISED quaternion and the f32 scales, in fp64
    double rt[4];
    for (int k = 0; k < 4; ++k) rt[k] = ((double)q[k] - 128.0) / 128.0;
    double M[9] = {
        1.0 - 2.0 * (rt[2] * rt[2] + rt[3] * rt[3]), 2.0 * (rt[1] * rt[2] + rt[0] * rt[3]), 2.0 * (rt[1] * rt[3] - rt[0] * rt[2]),
        2.0 * (rt[1] * rt[2] - rt[0] * rt[3]), 1.0 - 2.0 * (rt[1] * rt[1] + rt[3] * rt[3]), 2.0 * (rt[2] * rt[3] + rt[0] * rt[1]),
        2.0 * (rt[1] * rt[3] + rt[0] * rt[2]), 2.0 * (rt[2] * rt[3] - rt[0] * rt[1]), 1.0 - 2.0 * (rt[1] * rt[1] + rt[2] * rt[2]),
    };
#pragma unroll
    for (int k = 0; k < 9; ++k) M[k] = M[k] * (double)sc[k / 3];
    const double s0 = M[0] * M[0] + M[3] * M[3] + M[6] * M[6];
    const double s1 = M[0] * M[1] + M[3] * M[4] + M[6] * M[7];
    const double s2 = M[0] * M[2] + M[3] * M[5] + M[6] * M[8];
    const double s3 = M[1] * M[1] + M[4] * M[4] + M[7] * M[7];
    const double s4 = M[1] * M[2] + M[4] * M[5] + M[7] * M[8];
    const double s5 = M[2] * M[2] + M[5] * M[5] + M[8] * M[8];
    const unsigned h01 = js_float_to_half(4 * s0) | (js_float_to_half(4 * s1) << 16);
    const unsigned h23 = js_float_to_half(4 * s2) | (js_float_to_half(4 * s3) << 16);
    const unsigned h45 = js_float_to_half(4 * s4) | (js_float_to_half(4 * s5) << 16);
    const float lab = (float)(labels ? labels[r] : -999999);  // NO_SELECTION, gs.js:6,579; texdata_f[..+3] = label
    tex[2 * j] = make_uint4(__float_as_uint(px), __float_as_uint(py), __float_as_uint(pz), __float_as_uint(lab));
    tex[2 * j + 1] = make_uint4(h01, h23, h45, rgba);
}

// ---- spherical-harmonics colour (degrees 1..3; not in the reference, see oracle/render_oracle.c) ----------
// coefficients re-laid at upload as coef[k][c][i] (k = 0 is f_dc), importance order: per view every thread reads
// its 3K coefficients from 3K planes, each load a fully used 256-B run per wave (as [k][i][c] the 12-byte stride
// made every load instruction straddle six lines).
__global__ __launch_bounds__(kRB) void sh_pack_kernel(const uint32_t* __restrict__ order, long long n,
                                                       const float* __restrict__ f_dc, const float* __restrict__ f_rest,
                                                       int K, float* __restrict__ coef) {
    const long long j = (long long)blockIdx.x * kRB + threadIdx.x;
    if (j >= n) return;
    const long long r = order[j];
    const int K1 = K - 1;
    for (int c = 0; c < 3; ++c) {
        coef[((size_t)0 * 3 + c) * n + j] = f_dc[3 * r + c];
        for (int k = 1; k < K; ++k) coef[((size_t)k * 3 + c) * n + j] = f_rest[(size_t)r * 3 * K1 + (size_t)c * K1 + (k - 1)];
    }
}

// hidden: the labels hidden, SORTED (exact int32: the worker's Map key); everything else compares the label the shaders see,
// int(uintBitsToFloat(cen.w))
__global__ __launch_bounds__(kRB) void edit_code_kernel(const uint4* __restrict__ tex, const int* __restrict__ labels, long long n,
                                                         const EditTables* __restrict__ ep, const int* __restrict__ hidden,
                                                         uint16_t* __restrict__ code, unsigned long long* __restrict__ n_hidden_out) {
    const EditTables& e = *ep;
    const long long i = (long long)blockIdx.x * kRB + threadIdx.x;
    bool hid = false;
    if (i < n) {
        const int vlabel = (int)__uint_as_float(tex[2 * i].w);
        unsigned c = 0;
        for (int k = e.n_colour - 1; k >= 0; --k)  // descending: the FIRST match is the one that stays
            if (e.colour_label[k] == vlabel) c = (c & ~127u) | (unsigned)(k + 1);
        for (int k = e.n_disp - 1; k >= 0; --k)
            if (e.disp_label[k] == vlabel) c = (c & ~(127u << 7)) | ((unsigned)(k + 1) << 7);
        if (vlabel == e.selected) c |= kEditSelected;
        const int lab = labels[i];
        int lo = 0, hi = e.n_hidden;  // first entry >= lab
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (hidden[mid] < lab) lo = mid + 1;
            else hi = mid;
        }
        hid = lo < e.n_hidden && hidden[lo] == lab;
        if (hid) c |= kEditHidden;
        code[i] = (uint16_t)c;
    }
    const unsigned long long m = __ballot(hid);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(n_hidden_out, (unsigned long long)__popcll(m));
}

// the exact int32 labels in importance order (the worker's labelData): the texture word holds them rounded to fp32
__global__ __launch_bounds__(kRB) void labels_pack_kernel(const uint32_t* __restrict__ order, long long n, const int* __restrict__ labels,
                                                           int* __restrict__ out) {
    const long long j = (long long)blockIdx.x * kRB + threadIdx.x;
    if (j < n) out[j] = labels ? labels[order[j]] : -999999;
}

int upload_splats(Ctx* c, int64_t n, const float* xyz, const float* scale, const float* rot, const float* opacity,
                  const float* f_dc, const int32_t* labels) {
    GSX_HIP(c, hipSetDevice(c->device));
    c->scene.rn = 0;
    c->scene.sh_on = false;     // the SH planes were laid out in the order that goes away here, also when n == 0
    c->scene.edits_on = false;  // the edit codes were resolved against the labels that go away here
    c->scene.edit_hidden_n = 0;
    if (n < 0 || (n > 0 && (!xyz || !f_dc || (scale && (!rot || !opacity)))))
        return fail(c, GSX_E_INVALID, "upload_splats: xyz and f_dc are required; scale needs rot and opacity");
    if (n > ((int64_t)1 << 30)) return fail(c, GSX_E_UNSUPPORTED, "upload_splats: n > 2^30");
    if (n == 0) return GSX_OK;
    DevBuf dxyz, dscale, drot, dop, dlab, key0, key1, idx0, idx1;
    DevBuf& ddc = c->scene.fdc;  // kept (source order): gsx_upload_sh re-lays it with f_rest
    c->scene.sh_deg = 0;
    auto up = [&](DevBuf& b, const void* src, size_t bytes) -> hipError_t {
        hipError_t e = b.ensure(bytes);
        if (e != hipSuccess) return e;
        return hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream);
    };
    GSX_HIP(c, up(dxyz, xyz, sizeof(float) * 3 * n));
    GSX_HIP(c, up(ddc, f_dc, sizeof(float) * 3 * n));
    if (scale) {
        GSX_HIP(c, up(dscale, scale, sizeof(float) * 3 * n));
        GSX_HIP(c, up(drot, rot, sizeof(float) * 4 * n));
    }
    if (opacity) GSX_HIP(c, up(dop, opacity, sizeof(float) * n));
    if (labels) GSX_HIP(c, up(dlab, labels, sizeof(int32_t) * n));
    GSX_HIP(c, key0.ensure(4 * n));
    GSX_HIP(c, key1.ensure(4 * n));
    GSX_HIP(c, idx0.ensure(4 * n));
    GSX_HIP(c, idx1.ensure(4 * n));
    GSX_HIP(c, c->scene.order.ensure(4 * n));
    GSX_HIP(c, c->scene.buffer.ensure(32 * n));
    GSX_HIP(c, c->scene.tex.ensure(32 * n));
    int where = 0;
    if (scale) {
        hipLaunchKernelGGL(splat_importance_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, dscale.as<float>(),
                           dop.as<float>(), (long long)n, key0.as<uint32_t>(), idx0.as<uint32_t>());
        GSX_HIP(c, hipGetLastError());
        int rc = radix_sort_pairs(c, key0.as<uint32_t>(), idx0.as<uint32_t>(), key1.as<uint32_t>(), idx1.as<uint32_t>(), n, 32,
                                  &where);
        if (rc) return rc;
    } else {
        hipLaunchKernelGGL(iota_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, idx0.as<uint32_t>(), (long long)n);
    }
    GSX_HIP(c, hipMemcpyAsync(c->scene.order.p, where ? idx1.p : idx0.p, 4 * n, hipMemcpyDeviceToDevice, c->stream));
    {
        ProfScope ps(c, "splat_pack");
        hipLaunchKernelGGL(splat_pack_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, c->scene.order.as<uint32_t>(),
                           (long long)n, dxyz.as<float>(), scale ? dscale.as<float>() : nullptr,
                           scale ? drot.as<float>() : nullptr, opacity ? dop.as<float>() : nullptr, ddc.as<float>(),
                           labels ? dlab.as<int>() : nullptr, c->scene.buffer.as<uint4>(), c->scene.tex.as<uint4>());
    }
    GSX_HIP(c, c->scene.labels.ensure(4 * n));
    hipLaunchKernelGGL(labels_pack_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, c->scene.order.as<uint32_t>(), (long long)n,
                       labels ? dlab.as<int>() : nullptr, c->scene.labels.as<int>());
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    c->scene.rn = n;
    return GSX_OK;
}

// gsx_render_set_edits: validate, resolve the tables into one code per splat (edit_code_kernel), keep the tables on the device
int render_set_edits(Ctx* c, const gsx_render_edits* e) {
    if (!e) {  // clear
        c->scene.edits_on = false;
        c->scene.edit_hidden_n = 0;
        return GSX_OK;
    }
    if (e->num_colors < 0 || e->num_colors > GSX_EDIT_TABLE_MAX)
        return fail(c, GSX_E_INVALID, "render_set_edits: num_colors %d outside [0, %d]", e->num_colors, GSX_EDIT_TABLE_MAX);
    if (e->num_displacements < 0 || e->num_displacements > GSX_EDIT_TABLE_MAX)
        return fail(c, GSX_E_INVALID, "render_set_edits: num_displacements %d outside [0, %d]", e->num_displacements, GSX_EDIT_TABLE_MAX);
    if (e->num_hidden < 0 || e->num_hidden > ((int64_t)1 << 30) || (e->num_hidden > 0 && !e->hidden_labels))
        return fail(c, GSX_E_INVALID, "render_set_edits: num_hidden %lld without hidden_labels, or outside [0, 2^30]", (long long)e->num_hidden);
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(e->custom_color[k])) return fail(c, GSX_E_INVALID, "render_set_edits: custom_color is not finite");
    for (int i = 0; i < e->num_colors; ++i)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(e->colors[i][k])) return fail(c, GSX_E_INVALID, "render_set_edits: colors[%d] is not finite", i);
    for (int i = 0; i < e->num_displacements; ++i)
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(e->displacements[i][k]))
                return fail(c, GSX_E_INVALID, "render_set_edits: displacements[%d] is not finite", i);
    if (c->scene.rn <= 0) return fail(c, GSX_E_STATE, "render_set_edits before upload_splats");
    GSX_HIP(c, hipSetDevice(c->device));
    EditTables t{};
    for (int i = 0; i < e->num_colors; ++i) {
        t.colour_label[i] = e->color_labels[i];
        for (int k = 0; k < 3; ++k) t.colour[i][k] = e->colors[i][k];
    }
    for (int i = 0; i < e->num_displacements; ++i) {
        t.disp_label[i] = e->displacement_labels[i];
        for (int k = 0; k < 3; ++k) t.disp[i][k] = e->displacements[i][k];
    }
    for (int k = 0; k < 3; ++k) t.custom[k] = e->custom_color[k];
    t.n_colour = e->num_colors;
    t.n_disp = e->num_displacements;
    t.selection_mode = e->selection_mode != 0;
    t.enable_custom = e->enable_custom_color != 0;
    t.enable_disp = e->enable_displacement != 0;
    t.selected = e->selected_label;
    std::vector<int> hidden(e->hidden_labels, e->hidden_labels + e->num_hidden);
    hidden.erase(std::remove(hidden.begin(), hidden.end(), -999999), hidden.end());  // NO_SELECTION is never hidden, gs.js:619
    std::sort(hidden.begin(), hidden.end());
    hidden.erase(std::unique(hidden.begin(), hidden.end()), hidden.end());
    t.n_hidden = (int)hidden.size();
    const long long n = c->scene.rn;
    c->scene.edits_on = false;
    c->scene.edit_hidden_n = 0;
    GSX_HIP(c, c->scene.edit_code.ensure(2 * (size_t)n));
    constexpr size_t kCountAt = (sizeof(EditTables) + 7) / 8 * 8;  // a u64 behind the tables: the splats hidden
    GSX_HIP(c, c->scene.edit_tab.ensure(kCountAt + 8));
    GSX_HIP(c, c->scene.edit_hidden.ensure(4 * std::max<size_t>(hidden.size(), 1)));
    unsigned long long* count_dev = reinterpret_cast<unsigned long long*>(c->scene.edit_tab.as<char>() + kCountAt);
    unsigned long long count = 0;
    GSX_HIP(c, hipMemcpyAsync(c->scene.edit_tab.p, &t, sizeof t, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemsetAsync(count_dev, 0, 8, c->stream));
    if (!hidden.empty()) GSX_HIP(c, hipMemcpyAsync(c->scene.edit_hidden.p, hidden.data(), 4 * hidden.size(), hipMemcpyHostToDevice, c->stream));
    {
        ProfScope ps(c, "render_edit_code");
        hipLaunchKernelGGL(edit_code_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, c->scene.tex.as<uint4>(), c->scene.labels.as<int>(), n,
                           c->scene.edit_tab.as<EditTables>(), c->scene.edit_hidden.as<int>(), c->scene.edit_code.as<uint16_t>(), count_dev);
    }
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipMemcpyAsync(&count, count_dev, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));  // (the host copies above live until here)
    c->scene.edit_hidden_n = (int64_t)count;
    c->scene.edits_on = true;
    return GSX_OK;
}

int upload_sh(Ctx* c, const float* f_rest, int deg) {
    GSX_HIP(c, hipSetDevice(c->device));
    if (deg < 0 || deg > 3) return fail(c, GSX_E_INVALID, "upload_sh: degree %d outside [0,3]", deg);
    if (c->scene.rn == 0) return fail(c, GSX_E_STATE, "upload_sh before upload_splats");
    if (deg > 0 && !f_rest) return fail(c, GSX_E_INVALID, "upload_sh: f_rest is NULL");
    const long long n = c->scene.rn;
    const int K = (deg + 1) * (deg + 1);
    DevBuf drest;
    if (K > 1) {
        GSX_HIP(c, drest.ensure(sizeof(float) * 3 * (size_t)(K - 1) * n));
        GSX_HIP(c, hipMemcpyAsync(drest.p, f_rest, sizeof(float) * 3 * (size_t)(K - 1) * n, hipMemcpyHostToDevice, c->stream));
    }
    GSX_HIP(c, c->scene.shc.ensure(sizeof(float) * 3 * (size_t)K * n));
    hipLaunchKernelGGL(sh_pack_kernel, dim3(grid_for(n)), dim3(kRB), 0, c->stream, c->scene.order.as<uint32_t>(), n,
                       c->scene.fdc.as<float>(), K > 1 ? drest.as<float>() : nullptr, K, c->scene.shc.as<float>());
    GSX_HIP(c, hipGetLastError());
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    c->scene.sh_deg = deg;
    c->scene.sh_on = true;
    return GSX_OK;
}

// ---- hit test: performHitTesting, gs.js:361-395 -------------------------------------------------------------
// An arg-min reduction over all splats of the key (dist, depth, index): the sequential JS loop keeps the
// first splat that is strictly nearer, or equally near and strictly less deep.  fp64, JS operation order.
struct HitKey {
    double dist, depth;
    long long idx;  // -1: none
};

__device__ __forceinline__ bool hit_better(const HitKey& a, const HitKey& b) {  // a replaces b?
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    if (a.dist < b.dist) return true;
    if (a.dist > b.dist) return false;
    if (a.depth < b.depth) return true;
    if (a.depth > b.depth) return false;
    return a.idx < b.idx;
}

__device__ __forceinline__ double js_hypot2(double a, double b) {  // V8 Math.hypot for two finite-or-not doubles
    const double big = __longlong_as_double(0x7ff0000000000000LL);
    if (fabs(a) == big || fabs(b) == big) return big;
    if (a != a || b != b) return a + b;
    const double v0 = fabs(a), v1 = fabs(b);
    const double mx = v0 > v1 ? v0 : v1;
    if (mx == 0.0) return 0.0;
    double sum = 0.0, comp = 0.0;
    {
        const double q = v0 / mx;
        const double summand = (q * q) - comp;
        const double pre = sum + summand;
        comp = (pre - sum) - summand;
        sum = pre;
    }
    {
        const double q = v1 / mx;
        const double summand = (q * q) - comp;
        const double pre = sum + summand;
        comp = (pre - sum) - summand;
        sum = pre;
    }
    return sqrt(sum) * mx;
}

struct HitUniforms {
    double m[16];  // proj * view, gs.js:364
    double x, y, vw, vh;
};

__device__ __forceinline__ HitKey hit_reduce_block(HitKey k, HitKey* sh /*[4]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        HitKey other;
        other.dist = __shfl_xor(k.dist, o);
        other.depth = __shfl_xor(k.depth, o);
        other.idx = __shfl_xor(k.idx, o);
        if (hit_better(other, k)) k = other;
    }
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = k;
    __syncthreads();
    HitKey r = sh[0];
    for (int w = 1; w < 4; ++w)
        if (hit_better(sh[w], r)) r = sh[w];
    return r;
}

__global__ __launch_bounds__(kRB) void hit_partial_kernel(const uint4* __restrict__ tex, long long n, HitUniforms u,
                                                           HitKey* __restrict__ partial) {
    __shared__ HitKey sh[4];
    HitKey best{0.0, 0.0, -1};
    for (long long i = (long long)blockIdx.x * kRB + threadIdx.x; i < n; i += (long long)gridDim.x * kRB) {
        const uint4 t = tex[2 * i];
        const double p0 = (double)__uint_as_float(t.x), p1 = (double)__uint_as_float(t.y), p2 = (double)__uint_as_float(t.z);
        double r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) r[k] = p0 * u.m[k] + p1 * u.m[k + 4] + p2 * u.m[k + 8] + 1.0 * u.m[k + 12];
        if (r[3] <= 0.0) continue;  // gs.js:402
        const double sx = (r[0] / r[3] + 1.0) * 0.5 * u.vw;
        const double sy = (r[1] / r[3] + 1.0) * 0.5 * u.vh;
        const double depth = r[2] / r[3];
        const double dist = js_hypot2(sx - u.x, sy - u.y);
        if (dist < 10.0) {  // gs.js:387
            const HitKey k{dist, depth, i};
            if (hit_better(k, best)) best = k;
        }
    }
    best = hit_reduce_block(best, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = best;
}

// labels: the exact int32 labels in importance order (labels_pack_kernel), the worker's labelData - not the texture word,
// which holds the label rounded to fp32
__global__ __launch_bounds__(kRB) void hit_final_kernel(const HitKey* __restrict__ partial, int m,
                                                         const int* __restrict__ labels, long long* __restrict__ out) {
    __shared__ HitKey sh[4];
    HitKey best{0.0, 0.0, -1};
    for (int t = threadIdx.x; t < m; t += kRB)
        if (hit_better(partial[t], best)) best = partial[t];
    best = hit_reduce_block(best, sh);
    if (threadIdx.x == 0) {
        out[0] = best.idx;
        out[1] = best.idx >= 0 ? (long long)labels[best.idx] : -999999LL;  // labelData[i], gs.js:390
    }
}

int hit_test(Ctx* c, const gsx_camera* cam, int W, int H, double x, double y, int32_t* label_out, int64_t* index_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    if (!cam || W < 1 || H < 1) return fail(c, GSX_E_INVALID, "hit_test: bad arguments");
    long long res[2] = {-1, -999999};
    if (c->scene.rn > 0) {
        HitUniforms u{};
        double view[16], proj[16];
        js_view_matrix(cam, view);
        js_proj_matrix(cam->fx, cam->fy, (double)W, (double)H, proj);
        js_multiply4(proj, view, u.m);
        u.x = x;
        u.y = y;
        u.vw = (double)W;
        u.vh = (double)H;
        const int blocks = (int)std::min<long long>(1024, (c->scene.rn + kRB - 1) / kRB);
        GSX_HIP(c, c->frame.scan.ensure(sizeof(HitKey) * (size_t)blocks + 16));
        HitKey* partial = c->frame.scan.as<HitKey>();
        long long* out = reinterpret_cast<long long*>(partial + blocks);
        {
            ProfScope ps(c, "hit_test");
            hipLaunchKernelGGL(hit_partial_kernel, dim3(blocks), dim3(kRB), 0, c->stream, c->scene.tex.as<uint4>(), (long long)c->scene.rn, u,
                               partial);
            hipLaunchKernelGGL(hit_final_kernel, dim3(1), dim3(kRB), 0, c->stream, partial, blocks, c->scene.labels.as<int>(), out);
        }
        GSX_HIP(c, hipGetLastError());
        GSX_HIP(c, hipMemcpyAsync(res, out, sizeof res, hipMemcpyDeviceToHost, c->stream));
        GSX_HIP(c, hipStreamSynchronize(c->stream));
    }
    if (index_out) *index_out = res[0];
    if (label_out) *label_out = (int32_t)res[1];
    return GSX_OK;
}

int render_debug(Ctx* c, uint8_t* buffer_out, uint32_t* order_out, uint32_t* tex_out, uint32_t* bucket_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->scene.rn;
    if (n == 0) return GSX_OK;
    if (buffer_out) GSX_HIP(c, hipMemcpyAsync(buffer_out, c->scene.buffer.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    if (order_out) GSX_HIP(c, hipMemcpyAsync(order_out, c->scene.order.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (tex_out) GSX_HIP(c, hipMemcpyAsync(tex_out, c->scene.tex.p, 32 * n, hipMemcpyDeviceToHost, c->stream));
    if (bucket_out) {
        if (c->frame.bucket.cap < 4 * n) return fail(c, GSX_E_STATE, "render_debug: no view has been rendered yet");
        GSX_HIP(c, hipMemcpyAsync(bucket_out, c->frame.bucket.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    }
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

// gsx_debug_render_scene: what labels_pack_kernel and sh_pack_kernel wrote at upload, and the SH state
int debug_render_scene(Ctx* c, int32_t* labels_out, float* sh_out, int32_t* sh_degree_out) {
    GSX_HIP(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->scene.rn;
    const bool sh = n > 0 && c->scene.sh_on;
    if (sh_degree_out) *sh_degree_out = sh ? c->scene.sh_deg : -1;
    if (n == 0) return GSX_OK;
    if (labels_out) GSX_HIP(c, hipMemcpyAsync(labels_out, c->scene.labels.p, 4 * n, hipMemcpyDeviceToHost, c->stream));
    if (sh_out && sh) {
        const size_t K = (size_t)(c->scene.sh_deg + 1) * (size_t)(c->scene.sh_deg + 1);
        GSX_HIP(c, hipMemcpyAsync(sh_out, c->scene.shc.p, sizeof(float) * 3 * K * n, hipMemcpyDeviceToHost, c->stream));
    }
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}


}  // namespace gsx
