// libgsx.so — C ABI entry points (include/gsx.h): context, scene upload, profiling, dispatch.
// No exception crosses the boundary; every entry returns a gsx_status.
#include <cstring>
#include <exception>
#include <new>

#include "gsx_ctx.hpp"

namespace gsx {

static thread_local std::string g_err;

void set_global_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
}

int fail(Ctx* c, int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    else g_err = buf;
    return code;
}

ProfScope::ProfScope(Ctx* ctx, const char* name, hipStream_t on) : c(ctx), st(on ? on : ctx->stream) {
    if (!c->prof_on) return;
    int id = -1;
    for (size_t i = 0; i < c->prof_names.size(); ++i)
        if (c->prof_names[i] == name) id = (int)i;
    if (id < 0) {
        c->prof_names.emplace_back(name);
        id = (int)c->prof_names.size() - 1;
    }
    auto get = [&](hipEvent_t& e) {
        if (!c->event_pool.empty()) {
            e = c->event_pool.back();
            c->event_pool.pop_back();
            return true;
        }
        return hipEventCreate(&e) == hipSuccess;
    };
    if (!get(ev.start) || !get(ev.stop)) return;
    ev.name_id = id;
    active = hipEventRecord(ev.start, st) == hipSuccess;
}

ProfScope::~ProfScope() {
    if (!active) return;
    (void)hipEventRecord(ev.stop, st);
    c->prof_events.push_back(ev);
}

static void prof_drain(Ctx* c) {
    for (auto& e : c->prof_events) {
        float ms = 0.f;
        if (hipEventSynchronize(e.stop) == hipSuccess && hipEventElapsedTime(&ms, e.start, e.stop) == hipSuccess) {
            auto& acc = c->prof_acc[c->prof_names[e.name_id]];
            acc.first += 1;
            acc.second += ms;
        }
        c->event_pool.push_back(e.start);
        c->event_pool.push_back(e.stop);
    }
    c->prof_events.clear();
}

// No exception may cross the C boundary: std::bad_alloc from a host-side vector sized by the caller's counts,
// std::system_error from a worker thread that cannot be started, ... become a status + gsx_last_error text.
template <class F>
static int guard(Ctx* c, const char* who, F f) {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(c, GSX_E_INVALID, "%s: out of host memory", who);
    } catch (const std::exception& e) {
        return fail(c, GSX_E_INVALID, "%s: %s", who, e.what());
    } catch (...) {
        return fail(c, GSX_E_INVALID, "%s: unknown failure", who);
    }
}

}  // namespace gsx

using gsx::Ctx;

#define CTX_OR_FAIL(ctx)                                                     \
    Ctx* c = reinterpret_cast<Ctx*>(ctx);                                    \
    if (!c) return gsx::fail(nullptr, GSX_E_INVALID, "%s: ctx is NULL", __func__)

extern "C" {

int gsx_abi_version(void) { return GSX_ABI_VERSION; }

int gsx_device_count(void) {
    int count = 0;
    return hipGetDeviceCount(&count) == hipSuccess ? count : 0;
}

int gsx_create(int device_id, gsx_ctx** out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "gsx_create: out is NULL");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return gsx::fail(nullptr, GSX_E_HIP, "gsx_create: no HIP device (%s); libgsx has no CPU fallback",
                         e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= count)
        return gsx::fail(nullptr, GSX_E_INVALID, "gsx_create: device %d out of range [0,%d)", device_id, count);
    hipDeviceProp_t prop;
    GSX_HIP(nullptr, hipGetDeviceProperties(&prop, device_id));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return gsx::fail(nullptr, GSX_E_HIP, "gsx_create: device %d is %s; this library carries gfx950 code only",
                         device_id, prop.gcnArchName);
    GSX_HIP(nullptr, hipSetDevice(device_id));
    Ctx* c = new (std::nothrow) Ctx();
    if (!c) return gsx::fail(nullptr, GSX_E_INVALID, "gsx_create: out of host memory");
    c->device = device_id;
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return gsx::fail(nullptr, GSX_E_HIP, "hipStreamCreate failed: %s", hipGetErrorString(e));
    }
    *out = reinterpret_cast<gsx_ctx*>(c);
    return GSX_OK;
}

void gsx_destroy(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);  // an early vote stage may still read the buffers ~Ctx frees
    gsx::prof_drain(c);
    for (auto ev : c->event_pool) (void)hipEventDestroy(ev);
    gsx::render_release_twin(c);
    gsx::vote_release_host(c);
    (void)hipStreamDestroy(c->stream);
    // ~Ctx frees the pinned buffers and destroys the events (PinBuf, Event) after the streams are gone.  Legal: both streams were
    // synchronised above and nothing was queued since, so no copy reads a pinned block and no event is waited for any more; and
    // neither hipHostFree nor hipEventDestroy takes a stream.
    delete c;
}

const char* gsx_last_error(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? c->err.c_str() : gsx::g_err.c_str();
}

void* gsx_stream(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return c ? (void*)c->stream : nullptr;
}

int gsx_set_option(gsx_ctx* ctx, const char* name, int64_t value) {
    CTX_OR_FAIL(ctx);
    if (!name) return gsx::fail(c, GSX_E_INVALID, "set_option: name is NULL");
    const std::string k(name);
    if (k == "spatial_sort") c->vopt.spatial_sort = value != 0;
    else if (k == "nn_brute") c->opt_nn_brute = value != 0;
    else if (k == "smooth_search") c->opt_smooth_search = value != 0;
    else if (k == "iou_table_lds") c->opt_iou_table_lds = value != 0;
    else if (k == "xcd_swizzle") {
        if (value < 0 || value > 65536) return gsx::fail(c, GSX_E_INVALID, "set_option: xcd_swizzle must be in [0,65536]");
        c->vopt.xcd_swizzle = (int)value;
    }
    else if (k == "seg_tiled") c->vopt.seg_tiled = value != 0;
    else if (k == "tile_lpt") c->ropt.tile_lpt = value != 0;
    else if (k == "exact_cull") c->ropt.exact_cull = value != 0;
    else if (k == "render_phases") {
        if (value < 1 || value > 8) return gsx::fail(c, GSX_E_INVALID, "set_option: render_phases must be in [1,8]");
        c->ropt.phases = (int)value;
    } else if (k == "render_phase_ratio") {
        if (value < 2 || value > 64) return gsx::fail(c, GSX_E_INVALID, "set_option: render_phase_ratio must be in [2,64]");
        c->ropt.phase_ratio = (int)value;
    }
    else if (k == "render_multi_pre") c->ropt.multi_pre = value != 0;
    else if (k == "render_bin32") c->ropt.bin32 = value != 0;
    else if (k == "render_compact") c->ropt.compact = value != 0;
    else if (k == "render_wide_sort") c->ropt.wide_sort = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    else if (k == "render_share_stream") {
        if ((value != 0) != (c->ropt.share_stream != 0)) gsx::render_release_twin(c);  // the extra frames' streams are made anew
        c->ropt.share_stream = value != 0;
    }
    else if (k == "render_frames") {
        if (value < 1 || value > gsx::kMaxFrames) return gsx::fail(c, GSX_E_INVALID, "set_option: render_frames must be in [1,%d]", (int)gsx::kMaxFrames);
        c->ropt.frames = (int)value;
    }
    else if (k == "blend_pk2") c->ropt.blend_pk2 = value < 0 ? 0 : (value > 2 ? 2 : (int)value);
    else if (k == "exchange_slabs") {
        if (value < 1 || value > 64) return gsx::fail(c, GSX_E_INVALID, "set_option: exchange_slabs must be in [1,64]");
        c->vopt.slabs = (int)value;
    } else if (k == "exchange_local") c->vopt.local_codes = value != 0;
    else if (k == "flat_project") c->vopt.flat_project = value != 0;
    else if (k == "seg_coarse") c->vopt.seg_coarse = value != 0;
    else if (k == "batched_counts") c->vopt.batched_counts = value != 0;
    else if (k == "wave_cull") c->vopt.wave_cull = value != 0;
    else if (k == "filter_project") c->vopt.filter_project = value != 0;
    else if (k == "host_pack") c->vopt.host_pack = value != 0;
    else if (k == "labels_u8") c->vopt.labels_u8 = value != 0;
    else if (k == "host_compact") c->vopt.host_compact = value != 0;
    else if (k == "early_vote") {
        if (value < 0 || value > 2) return gsx::fail(c, GSX_E_INVALID, "set_option: early_vote must be 0, 1 or 2");
        c->vopt.early_vote = (int)value;
    } else if (k == "early_replay") c->vopt.early_replay = value != 0;
    else if (k == "early_vote_at") {
        if (value < 0 || value > 1000) return gsx::fail(c, GSX_E_INVALID, "set_option: early_vote_at must be in [0,1000] (permille of the announced views; 0 = from the hand-over rate)");
        c->vopt.early_at = (int)value;
    }
    else if (k == "host_prefetch") gsx::set_host_prefetch((int)value);
    else if (k == "host_prefetch_burst") gsx::set_host_prefetch_burst(value != 0);
#ifdef GSX_EXPERIMENTS
    else if (k == "ablate") c->vopt.ablate = (int)value;
#endif
    else if (k == "host_threads") {
        if (value < 0 || value > 256) return gsx::fail(c, GSX_E_INVALID, "set_option: host_threads must be in [0,256]");
        if ((int)value != c->vopt.host_threads) c->ho.workers.reset();  // re-created with the new size at the next host-side hand-over
        c->vopt.host_threads = (int)value;
    }
    else if (k == "vote_unroll") {
        if (value != 2 && value != 4 && value != 8)
            return gsx::fail(c, GSX_E_INVALID, "set_option: vote_unroll must be 2, 4 or 8");
        c->vopt.vote_unroll = (int)value;
    } else
        return gsx::fail(c, GSX_E_INVALID, "set_option: unknown option '%s'", name);
    return GSX_OK;
}

int gsx_get_option(gsx_ctx* ctx, const char* name, int64_t* value) {
    CTX_OR_FAIL(ctx);
    if (!name || !value) return gsx::fail(c, GSX_E_INVALID, "get_option: NULL argument");
    const std::string k(name);
    if (k == "early_vote") *value = c->vopt.early_vote;
    else if (k == "early_vote_at") *value = c->vopt.early_at;
    else if (k == "early_replay") *value = c->vopt.early_replay ? 1 : 0;
    else if (k == "seg_tiled") *value = c->vopt.seg_tiled ? 1 : 0;
    else if (k == "seg_coarse") *value = c->vopt.seg_coarse ? 1 : 0;
    else
        return gsx::fail(c, GSX_E_INVALID, "get_option: option '%s' cannot be read back", name);
    return GSX_OK;
}

int gsx_synchronize(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    GSX_HIP(c, hipSetDevice(c->device));
    {
        const int rc = gsx::vote_flush_pending(c);
        if (rc) return rc;
    }
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

// ---- scene ---------------------------------------------------------------------------------------
static int alloc_positions(Ctx* c, int64_t n) {
    GSX_HIP(c, hipSetDevice(c->device));
    const size_t bytes = sizeof(float) * (size_t)(n > 0 ? n : 1);
    GSX_HIP(c, c->x.ensure(bytes));
    GSX_HIP(c, c->y.ensure(bytes));
    GSX_HIP(c, c->z.ensure(bytes));
    c->n = n;
    c->run.n_pad = (n + 255) / 256 * 256;
    c->run.begun = false;  // planes are sized by n: a new scene needs a new vote_begin
    c->run.labels_valid = false;
    gsx::assoc_end(c);  // an association run's ids belong to the Gaussians that go away here
    return GSX_OK;
}

int gsx_upload_positions(gsx_ctx* ctx, int64_t n, const float* x, const float* y, const float* z) {
    CTX_OR_FAIL(ctx);
    if (n < 0 || (n > 0 && (!x || !y || !z))) return gsx::fail(c, GSX_E_INVALID, "upload_positions: bad arguments");
    if (n > (int64_t)1 << 31) return gsx::fail(c, GSX_E_UNSUPPORTED, "upload_positions: n > 2^31");
    int rc = alloc_positions(c, n);
    if (rc) return rc;
    if (n == 0) return GSX_OK;
    GSX_HIP(c, hipMemcpyAsync(c->x.p, x, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(c->y.p, y, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(c->z.p, z, sizeof(float) * n, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    c->sorted = false;
    if (c->vopt.spatial_sort) return gsx::spatial_sort_positions(c);
    return GSX_OK;
}

int gsx_upload_positions_strided(gsx_ctx* ctx, int64_t n, const void* base, int64_t stride_bytes, int64_t off_x,
                                 int64_t off_y, int64_t off_z) {
    CTX_OR_FAIL(ctx);
    if (n < 0 || (n > 0 && !base) || stride_bytes < 4 || off_x < 0 || off_y < 0 || off_z < 0)
        return gsx::fail(c, GSX_E_INVALID, "upload_positions_strided: bad arguments");
    if (n > (int64_t)1 << 31) return gsx::fail(c, GSX_E_UNSUPPORTED, "upload_positions_strided: n > 2^31");
    return gsx::guard(c, __func__, [&] {
        // AoS -> SoA transpose on the host (rows are 248+ bytes in a 3DGS PLY; only 12 are wanted)
        std::vector<float> sx((size_t)n), sy((size_t)n), sz((size_t)n);
        const char* b = static_cast<const char*>(base);
        for (int64_t i = 0; i < n; ++i) {
            const char* row = b + i * stride_bytes;
            std::memcpy(&sx[i], row + off_x, 4);
            std::memcpy(&sy[i], row + off_y, 4);
            std::memcpy(&sz[i], row + off_z, 4);
        }
        return gsx_upload_positions(ctx, n, sx.data(), sy.data(), sz.data());
    });
}

int64_t gsx_num_gaussians(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? c->n : 0;
}

// ---- projection probe ----------------------------------------------------------------------------
int gsx_project_one(gsx_ctx* ctx, const float pos[3], const gsx_camera* cam, int32_t* x, int32_t* y,
                    int32_t* visible) {
    CTX_OR_FAIL(ctx);
    if (!pos || !cam || !x || !y || !visible) return gsx::fail(c, GSX_E_INVALID, "project_one: NULL argument");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf tmp;
    GSX_HIP(c, tmp.ensure(3 * sizeof(float)));
    hipError_t e = hipMemcpy(tmp.p, pos, 3 * sizeof(float), hipMemcpyHostToDevice);
    int rc = GSX_OK;
    if (e != hipSuccess) rc = gsx::fail(c, GSX_E_HIP, "project_one: H2D failed: %s", hipGetErrorString(e));
    if (!rc) rc = gsx::project_all(c, cam, tmp.as<float>(), tmp.as<float>() + 1, tmp.as<float>() + 2, 1, x, y, nullptr);
    if (!rc) *visible = (*x >= 0) ? 1 : 0;
    return rc;
}

int gsx_project_all(gsx_ctx* ctx, const gsx_camera* cam, int32_t* x, int32_t* y) {
    CTX_OR_FAIL(ctx);
    if (!cam || !x || !y) return gsx::fail(c, GSX_E_INVALID, "project_all: NULL argument");
    return gsx::guard(c, __func__, [&] { return gsx::project_all(c, cam, c->x.as<float>(), c->y.as<float>(), c->z.as<float>(), c->n, x, y,
                            c->sorted ? c->perm.as<uint32_t>() : nullptr); });
}

// ---- vote ----------------------------------------------------------------------------------------
int gsx_vote_begin(gsx_ctx* ctx, int32_t n_classes, int32_t first_view, int32_t total_views) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_begin(c, n_classes, first_view, total_views); });
}
int gsx_vote_view(gsx_ctx* ctx, const gsx_camera* cam, const void* seg, int32_t seg_dtype, int32_t seg_w,
                  int32_t seg_h, int32_t img_w, int32_t img_h) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_view(c, cam, seg, seg_dtype, seg_w, seg_h, img_w, img_h); });
}
int gsx_vote_view_device(gsx_ctx* ctx, const gsx_camera* cam, const void* seg_dev, int32_t seg_dtype, int32_t seg_w,
                         int32_t seg_h, int32_t img_w, int32_t img_h) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_views_device(c, 1, cam, &seg_dev, seg_dtype, seg_w, seg_h, img_w, img_h); });
}
int gsx_vote_views_device(gsx_ctx* ctx, int32_t n, const gsx_camera* cams, const void* const* segs_dev, int32_t seg_dtype,
                          int32_t seg_w, int32_t seg_h, int32_t img_w, int32_t img_h) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_views_device(c, n, cams, segs_dev, seg_dtype, seg_w, seg_h, img_w, img_h); });
}
int64_t gsx_debug_workers_stress(int32_t threads, int32_t runs, int32_t max_parts) {
    try {
        return gsx::workers_stress(threads, runs, max_parts);
    } catch (...) {
        return -1;
    }
}
int gsx_debug_widen_labels(int32_t threads, const uint8_t* bins, int64_t n, int32_t* labels_out) {
    if (n < 0 || (n > 0 && (!bins || !labels_out))) return GSX_E_INVALID;
    try {
        if (threads > 1) {
            gsx::Workers pool(threads);
            gsx::host_widen_labels(&pool, labels_out, bins, (size_t)n);
        } else {
            gsx::host_widen_labels(nullptr, labels_out, bins, (size_t)n);
        }
        return GSX_OK;
    } catch (...) {
        return GSX_E_HIP;  /* the pool could not be created (thread / memory exhaustion) */
    }
}
int gsx_debug_host_pack_compact(const void* seg, int32_t seg_dtype, int32_t w, int32_t h, int32_t n_classes, int32_t threads, uint8_t* out,
                                int64_t out_cap, int64_t* bytes, int64_t* table_bytes, int64_t* stream_off, int32_t* bad) {
    try {
        return gsx::debug_host_pack_compact(seg, seg_dtype, w, h, n_classes, threads, out, out_cap, bytes, table_bytes, stream_off, bad);
    } catch (...) {
        return GSX_E_HIP;
    }
}
int gsx_debug_host_pack(const void* seg, int32_t seg_dtype, int32_t w, int32_t h, int32_t n_classes, int32_t tiled,
                        int32_t coarse, int32_t threads, uint8_t* out, int64_t out_cap, int64_t* bytes, int64_t* coarse_off,
                        int32_t* bad) {
    return gsx::guard(nullptr, __func__, [&] { return gsx::debug_host_pack(seg, seg_dtype, w, h, n_classes, tiled, coarse, threads, out, out_cap, bytes, coarse_off, bad); });
}
int32_t gsx_vote_num_views(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? (int32_t)c->run.views.size() : 0;
}
int gsx_vote_rewind(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_rewind(c); });
}
int gsx_vote_finalize(gsx_ctx* ctx, int32_t* labels_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_finalize(c, labels_out); });
}
void* gsx_vote_labels_device(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return (c && c->run.labels_valid) ? c->planes.labels.p : nullptr;
}
int gsx_vote_flush(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    return gsx::vote_flush(c);
}
void* gsx_vote_counts_device(gsx_ctx* ctx, int64_t* n_int32_words) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !c->run.begun) return nullptr;
    if (n_int32_words) *n_int32_words = (int64_t)c->run.bins * c->run.n_pad * (c->run.wide ? 2 : 1) / 4;
    return c->planes.cnt.p;
}
int gsx_vote_tiebreak_keys(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    return gsx::vote_tiebreak_keys(c);
}
void* gsx_vote_keys_device(gsx_ctx* ctx, int64_t* n_int32_words) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !c->run.begun) return nullptr;
    if (n_int32_words) *n_int32_words = c->run.n_pad;
    return c->planes.keys.p;
}
int gsx_vote_labels_from_keys(gsx_ctx* ctx, int32_t* labels_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_labels_from_keys(c, labels_out); });
}
void* gsx_vote_first_device(gsx_ctx* ctx, int64_t* n_int32_words) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !c->run.begun) return nullptr;
    if (n_int32_words) *n_int32_words = (int64_t)c->run.bins * c->run.n_pad * (c->run.wide ? 2 : 1) / 4;
    return c->planes.fv.p;
}
int64_t gsx_vote_slab_size(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return (c && c->run.begun) ? c->run.sn : 0;
}
int gsx_vote_slab_reduce(gsx_ctx* ctx, const void* recv_counts_dev, const void* recv_first_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_slab_reduce(c, recv_counts_dev, recv_first_dev); });
}
int gsx_vote_flush_counts(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    return gsx::vote_flush_counts(c);
}
int gsx_vote_slab_totals(gsx_ctx* ctx, const void* recv_counts_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_slab_totals(c, recv_counts_dev); });
}
void* gsx_vote_cand_device(gsx_ctx* ctx, int64_t* n_int32_words) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !c->run.begun) return nullptr;
    if (n_int32_words) *n_int32_words = 8 * c->run.sn;
    return c->planes.cand.p;
}
int gsx_vote_tie_codes(gsx_ctx* ctx, const void* cand_all_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_tie_codes(c, cand_all_dev); });
}
void* gsx_vote_codes_device(gsx_ctx* ctx, int64_t* n_int32_words) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || !c->run.begun) return nullptr;
    if (n_int32_words) *n_int32_words = c->run.n_pad / 2;
    return c->planes.codes.p;
}
int gsx_vote_tie_resolve(gsx_ctx* ctx, const void* recv_codes_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_tie_resolve(c, recv_codes_dev); });
}
int gsx_vote_labels_from_sorted(gsx_ctx* ctx, const void* sorted_labels_dev, int32_t* labels_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_labels_from_sorted(c, sorted_labels_dev, labels_out); });
}
int gsx_vote_export(gsx_ctx* ctx, int64_t reserve_bytes, void* blobs_out, void** pool_dev, int64_t* pool_bytes) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_export(c, reserve_bytes, blobs_out, pool_dev, pool_bytes); });
}
int64_t gsx_vote_pool_bytes(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return (c && c->run.begun && !c->run.pool_base) ? (int64_t)((c->run.seg_used + 255) / 256 * 256) : 0;
}
int64_t gsx_vote_link_bytes(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return (c && c->run.begun) ? (int64_t)c->ho.compact_bytes : 0;
}
int64_t gsx_vote_early_views(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c && (c->early.phase == gsx::EarlyPhase::Started || c->early.batches > 0) ? c->early.done : 0;
}
int gsx_vote_import(gsx_ctx* ctx, int32_t n_parts, const int32_t* part_views, const int64_t* part_offsets, const void* blobs,
                    const void* pool_all_dev, int64_t pool_all_bytes) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_import(c, n_parts, part_views, part_offsets, blobs, pool_all_dev, pool_all_bytes); });
}
int gsx_vote_import_uniform(gsx_ctx* ctx, int32_t n_parts, const int32_t* part_views, const int64_t* part_offsets, const gsx_camera* cams,
                            int32_t seg_w, int32_t seg_h, int32_t img_w, int32_t img_h, const void* pool_all_dev, int64_t pool_all_bytes) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_import_uniform(c, n_parts, part_views, part_offsets, cams, seg_w, seg_h, img_w, img_h, pool_all_dev, pool_all_bytes); });
}
int gsx_vote_import_undo(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_import_undo(c); });
}
int gsx_vote_map_stride(gsx_ctx* ctx, int32_t seg_w, int32_t seg_h, int64_t* stride) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_map_stride(c, seg_w, seg_h, stride); });
}
int gsx_vote_views_match_uniform(gsx_ctx* ctx, int32_t n, const gsx_camera* cams, int32_t seg_w, int32_t seg_h, int32_t img_w, int32_t img_h,
                                 int32_t* match) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_views_match_uniform(c, n, cams, seg_w, seg_h, img_w, img_h, match); });
}
int gsx_vote_slab_labels(gsx_ctx* ctx, int32_t slab, int32_t slabs, int64_t* slab_size) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_slab_labels(c, slab, slabs, slab_size); });
}
int gsx_host_threads(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c) return 0;
    try {
        return gsx::host_threads(c);  // may create the worker pool
    } catch (...) {
        return 1;  // no pool: maps are packed on the calling thread
    }
}
int gsx_default_host_threads(void) { return gsx::default_host_threads(); }
int gsx_vote_debug_planes(gsx_ctx* ctx, uint16_t* counts_out, uint16_t* first_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::vote_debug_planes(c, counts_out, first_out); });
}

// ---- rasterizer -----------------------------------------------------------------------------------
int gsx_upload_splats(gsx_ctx* ctx, int64_t n, const float* xyz, const float* scale, const float* rot,
                      const float* opacity, const float* f_dc, const int32_t* labels) {
    CTX_OR_FAIL(ctx);
    gsx::lift_end(c);  // a lift run's table belongs to the splats that go away here
    gsx::label_new_upload(c, labels != nullptr);  // ... and so do the checked one-byte labels of the label frames
    gsx::depth_new_upload(c);                     // ... and the last depth view
    return gsx::guard(c, __func__, [&] { return gsx::upload_splats(c, n, xyz, scale, rot, opacity, f_dc, labels); });
}
int gsx_upload_sh(gsx_ctx* ctx, const float* f_rest, int32_t sh_degree) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::upload_sh(c, f_rest, sh_degree); });
}
int gsx_render_set_edits(gsx_ctx* ctx, const gsx_render_edits* edits) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::render_set_edits(c, edits); });
}
int64_t gsx_render_num_hidden(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? c->scene.edit_hidden_n : 0;
}
int64_t gsx_num_splats(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? c->scene.rn : 0;
}
int gsx_render_view(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, float* rgba_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::render_view(c, cam, width, height, rgba_out); });
}
int gsx_render_views(gsx_ctx* ctx, int32_t n, const gsx_camera* cams, int32_t width, int32_t height, float* const* rgba_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::render_views(c, n, cams, width, height, rgba_out); });
}
void* gsx_render_image_device(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return c ? c->frame.image.p : nullptr;
}
int64_t gsx_render_num_pairs(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? (int64_t)c->frame.P : 0;
}
int64_t gsx_render_num_pairs_consumed(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? (int64_t)c->frame.consumed : 0;
}
int gsx_hit_test(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, double x, double y,
                 int32_t* label_out, int64_t* index_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::hit_test(c, cam, width, height, x, y, label_out, index_out); });
}
int gsx_render_debug(gsx_ctx* ctx, uint8_t* buffer_out, uint32_t* order_out, uint32_t* texdata_out,
                     uint32_t* bucket_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::render_debug(c, buffer_out, order_out, texdata_out, bucket_out); });
}
int gsx_debug_render_scene(gsx_ctx* ctx, int32_t* labels_out, float* sh_out, int32_t* sh_degree_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::debug_render_scene(c, labels_out, sh_out, sh_degree_out); });
}
int gsx_debug_render_pre(gsx_ctx* ctx, int32_t num_views, const gsx_camera* cams, int32_t width, int32_t height, int32_t multi,
                         int32_t compact, const gsx_debug_pre_view* out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::debug_render_pre(c, num_views, cams, width, height, multi, compact, out); });
}

int gsx_kmeans(gsx_ctx* ctx, int64_t n, const float* points, const float* colors, int32_t k, const int64_t* init_index,
               int32_t max_iter, double tol, int32_t* labels_out, float* centroids_out, int32_t* iterations_out,
               int32_t* converged_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::kmeans(c, n, points, colors, k, init_index, max_iter, tol, labels_out, centroids_out, iterations_out,
                       converged_out); });
}

int gsx_normals(gsx_ctx* ctx, int64_t n, const float* points, int64_t k, double* normals_out, double* residuals_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::normals(c, n, points, k, normals_out, residuals_out); });
}
int gsx_debug_normals_moments(gsx_ctx* ctx, int64_t n, const float* points, int64_t k, double* moments_out) {
    CTX_OR_FAIL(ctx);
    if (!moments_out) return gsx::fail(c, GSX_E_INVALID, "debug_normals_moments: moments_out is NULL");
    return gsx::guard(c, __func__, [&] { return gsx::normals(c, n, points, k, nullptr, nullptr, moments_out); });
}
int gsx_debug_nn_grid(int64_t n, const float* points, int64_t k, int brute, double origin_out[3], double* h_out, int32_t dims_out[3],
                      uint32_t* cell_start_out, int32_t* order_out) {
    return gsx::guard(nullptr, __func__, [&] { return gsx::debug_nn_grid(n, points, k, brute, origin_out, h_out, dims_out, cell_start_out, order_out); });
}
int gsx_knn(gsx_ctx* ctx, int64_t n, const float* points, int32_t k, int32_t* index_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::knn(c, n, points, k, index_out); });
}
void* gsx_knn_device(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return c && c->nn_index_rows ? c->nn_index.p : nullptr;
}
int gsx_region_growing(gsx_ctx* ctx, int64_t n, const float* points, int64_t k_normals, int32_t k, double residual_threshold,
                       double angle_threshold, int32_t* labels_out, double* normals_out, double* residuals_out, int32_t* n_regions_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::region_growing(c, n, points, k_normals, k, residual_threshold, angle_threshold, labels_out,
                               normals_out, residuals_out, n_regions_out); });
}

int gsx_smooth_labels(gsx_ctx* ctx, int64_t n, const float* points, const int32_t* labels, int64_t k, int32_t rounds, int32_t min_votes,
                      int32_t ignore_label, int32_t flags, int32_t* labels_out, int32_t* support_out, int64_t* changed_out,
                      int32_t* rounds_done_out) {
    CTX_OR_FAIL(ctx);
    const gsx::SmoothArgs a{rounds, min_votes, ignore_label, flags, labels_out, support_out, changed_out, rounds_done_out};
    return gsx::guard(c, __func__, [&] { return gsx::smooth_labels(c, n, points, labels, k, a); });
}
int gsx_smooth_labels_lists(gsx_ctx* ctx, int64_t n, int32_t k, const int32_t* knn, const int32_t* labels, int32_t rounds, int32_t min_votes,
                            int32_t ignore_label, int32_t flags, int32_t* labels_out, int32_t* support_out, int64_t* changed_out,
                            int32_t* rounds_done_out) {
    CTX_OR_FAIL(ctx);
    const gsx::SmoothArgs a{rounds, min_votes, ignore_label, flags, labels_out, support_out, changed_out, rounds_done_out};
    return gsx::guard(c, __func__, [&] { return gsx::smooth_labels_lists(c, n, k, knn, labels, a); });
}
int gsx_debug_smooth_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_smooth_constants: NULL argument");
    gsx::smooth_constants(out);
    return GSX_OK;
}

int gsx_split_labels(gsx_ctx* ctx, int64_t n, const float* points, const int32_t* labels, int32_t k, double max_dist, int64_t min_size,
                     int32_t max_instances, int32_t ignore_label, int32_t flags, int32_t* labels_out, int32_t* component_out,
                     int32_t* instance_label_out, int64_t* instance_size_out, int32_t* instance_rep_out, int32_t* n_instances_out,
                     int64_t* n_components_out) {
    CTX_OR_FAIL(ctx);
    const gsx::SplitArgs a{max_dist, min_size, max_instances, ignore_label, flags, labels_out, component_out, instance_label_out,
                           instance_size_out, instance_rep_out, n_instances_out, n_components_out};
    return gsx::guard(c, __func__, [&] { return gsx::split_labels(c, n, points, labels, k, a); });
}
int gsx_split_labels_lists(gsx_ctx* ctx, int64_t n, int32_t k, const int32_t* knn, const float* points, const int32_t* labels, double max_dist,
                           int64_t min_size, int32_t max_instances, int32_t ignore_label, int32_t flags, int32_t* labels_out,
                           int32_t* component_out, int32_t* instance_label_out, int64_t* instance_size_out, int32_t* instance_rep_out,
                           int32_t* n_instances_out, int64_t* n_components_out) {
    CTX_OR_FAIL(ctx);
    const gsx::SplitArgs a{max_dist, min_size, max_instances, ignore_label, flags, labels_out, component_out, instance_label_out,
                           instance_size_out, instance_rep_out, n_instances_out, n_components_out};
    return gsx::guard(c, __func__, [&] { return gsx::split_labels_lists(c, n, k, knn, points, labels, a); });
}

int gsx_iou_masks(gsx_ctx* ctx, int32_t n_masks, const void* const* masks, int32_t mask_dtype, int32_t n_gt, const void* const* gts,
                  int32_t gt_dtype, int32_t h, int32_t w, int64_t* inter_out, int64_t* area_masks_out, int64_t* area_gt_out, double* iou_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::iou_masks(c, false, n_masks, masks, mask_dtype, n_gt, gts, gt_dtype, h, w, inter_out,
                                                               area_masks_out, area_gt_out, iou_out); });
}
int gsx_iou_masks_device(gsx_ctx* ctx, int32_t n_masks, const void* const* masks_dev, int32_t mask_dtype, int32_t n_gt,
                         const void* const* gts_dev, int32_t gt_dtype, int32_t h, int32_t w, int64_t* inter_out, int64_t* area_masks_out,
                         int64_t* area_gt_out, double* iou_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::iou_masks(c, true, n_masks, masks_dev, mask_dtype, n_gt, gts_dev, gt_dtype, h, w, inter_out,
                                                               area_masks_out, area_gt_out, iou_out); });
}
int gsx_iou_label_maps(gsx_ctx* ctx, int32_t n_pairs, const void* const* pred, int32_t pred_dtype, int32_t n_pred_classes,
                       const void* const* gt, int32_t gt_dtype, int32_t n_gt_classes, int32_t h, int32_t w, int64_t* table_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::iou_label_maps(c, false, n_pairs, pred, pred_dtype, n_pred_classes, gt, gt_dtype,
                                                                    n_gt_classes, h, w, table_out); });
}
int gsx_iou_label_maps_device(gsx_ctx* ctx, int32_t n_pairs, const void* const* pred_dev, int32_t pred_dtype, int32_t n_pred_classes,
                              const void* const* gt_dev, int32_t gt_dtype, int32_t n_gt_classes, int32_t h, int32_t w, int64_t* table_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::iou_label_maps(c, true, n_pairs, pred_dev, pred_dtype, n_pred_classes, gt_dev, gt_dtype,
                                                                    n_gt_classes, h, w, table_out); });
}
int gsx_masks_top_index(gsx_ctx* ctx, int32_t n_masks, const void* const* masks, int32_t mask_dtype, int32_t h, int32_t w,
                        int32_t* index_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::masks_top_index(c, n_masks, masks, mask_dtype, h, w, index_out); });
}
int gsx_debug_iou_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_iou_constants: NULL argument");
    gsx::iou_constants(out);
    return GSX_OK;
}

int gsx_segmap_from_logits(gsx_ctx* ctx, const void* logits_dev, int32_t dtype, int32_t n, int32_t C, int32_t h, int32_t w, int32_t out_w,
                           int32_t out_h, int32_t* maps_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::segmap_from_logits(c, logits_dev, dtype, n, C, h, w, out_w, out_h, maps_dev); });
}
int gsx_segmap_from_masks(gsx_ctx* ctx, const void* masks_dev, int32_t dtype, int32_t K, int32_t mh, int32_t mw, const float* cls_dev,
                          const float* conf_dev, int32_t out_w, int32_t out_h, int32_t* map_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::segmap_from_masks(c, masks_dev, dtype, K, mh, mw, cls_dev, conf_dev, out_w, out_h, map_dev); });
}
int gsx_debug_segmap_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_segmap_constants: NULL argument");
    gsx::segmap_constants(out);
    return GSX_OK;
}
int gsx_segmap_from_queries(gsx_ctx* ctx, const void* masks_dev, int32_t dtype, int32_t Q, int32_t h, int32_t w, int32_t K,
                            const int32_t* slot_query_dev, const float* slot_score_dev, const int32_t* slot_label_dev, int32_t mid_w,
                            int32_t mid_h, double threshold, int32_t mode, int32_t out_w, int32_t out_h, int32_t* map_dev,
                            int32_t* slot_segment_dev, float* slot_pred_score_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] {
        return gsx::segmap_from_queries(c, masks_dev, dtype, Q, h, w, K, slot_query_dev, slot_score_dev, slot_label_dev, mid_w, mid_h, threshold,
                                        mode, out_w, out_h, map_dev, slot_segment_dev, slot_pred_score_dev);
    });
}
int gsx_debug_queries_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_queries_constants: NULL argument");
    gsx::queries_constants(out);
    return GSX_OK;
}
int gsx_lift_begin(gsx_ctx* ctx, int32_t n_classes) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::lift_begin(c, n_classes); });
}
int gsx_lift_view(gsx_ctx* ctx, const gsx_camera* cam, const void* seg, int32_t seg_dtype, int32_t width, int32_t height) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::lift_view(c, cam, seg, seg_dtype, width, height, false); });
}
int gsx_lift_view_device(gsx_ctx* ctx, const gsx_camera* cam, const void* seg_dev, int32_t seg_dtype, int32_t width, int32_t height) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::lift_view(c, cam, seg_dev, seg_dtype, width, height, true); });
}
int32_t gsx_lift_num_views(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c && c->lift.begun ? c->lift.views : 0;
}
int64_t gsx_lift_num_atomics(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? (int64_t)c->lift.atomics : 0;
}
int gsx_lift_finalize(gsx_ctx* ctx, double min_weight, int32_t* labels_out, double* share_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::lift_finalize(c, min_weight, labels_out, share_out); });
}
int gsx_lift_table(gsx_ctx* ctx, uint64_t* table_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::lift_table(c, table_out); });
}
// ---- label frames (labelmap.hip) --------------------------------------------------------------------
int gsx_label_view(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, int32_t n_classes, double min_weight,
                   int32_t n_planes, const int32_t* plane_labels, int32_t* label_out, uint32_t* weight_out, uint32_t* total_out,
                   uint32_t* planes_out) {
    CTX_OR_FAIL(ctx);
    const gsx::LabelViewArgs a{n_classes, min_weight, n_planes, plane_labels, label_out, weight_out, total_out, planes_out};
    return gsx::guard(c, __func__, [&] { return gsx::label_view(c, cam, width, height, a); });
}
void* gsx_label_map_device(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return c ? c->labelmap.map.p : nullptr;
}
int64_t gsx_label_num_passes(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? (int64_t)c->labelmap.passes : 0;
}
int64_t gsx_label_num_single_tiles(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c ? (int64_t)c->labelmap.single : 0;
}
int gsx_debug_labelmap_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_labelmap_constants: NULL argument");
    gsx::labelmap_constants(out);
    return GSX_OK;
}
// ---- depth frames (depthmap.hip) --------------------------------------------------------------------
int gsx_depth_view(gsx_ctx* ctx, const gsx_camera* cam, int32_t width, int32_t height, double quantile, uint32_t* total_out,
                   int64_t* moment_out, int32_t* surface_key_out, int32_t* surface_index_out) {
    CTX_OR_FAIL(ctx);
    const gsx::DepthViewArgs a{quantile, total_out, moment_out, surface_key_out, surface_index_out};
    return gsx::guard(c, __func__, [&] { return gsx::depth_view(c, cam, width, height, a); });
}
void* gsx_depth_surface_index_device(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return c && c->depthmap.valid ? c->depthmap.index.p : nullptr;
}
void* gsx_depth_surface_key_device(gsx_ctx* ctx) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    return c && c->depthmap.valid ? c->depthmap.key.p : nullptr;
}
int64_t gsx_depth_num_surface(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c && c->depthmap.valid ? (int64_t)c->depthmap.surfaces : 0;
}
int gsx_depth_key_to_z(const gsx_camera* cam, int32_t width, int32_t height, double* scale, double* offset) {
    return gsx::guard(nullptr, __func__, [&] { return gsx::depth_key_to_z(cam, width, height, scale, offset); });
}
int gsx_depth_pick(gsx_ctx* ctx, double x, double y, int32_t* label_out, int64_t* index_out, double* z_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::depth_pick(c, x, y, label_out, index_out, z_out); });
}
int gsx_debug_depth_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_depth_constants: NULL argument");
    gsx::depth_constants(out);
    return GSX_OK;
}
// ---- instance association (assoc.hip) --------------------------------------------------------------
int gsx_assoc_begin(gsx_ctx* ctx, int32_t max_segments, int32_t max_instances, double min_overlap, int32_t min_size) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::assoc_begin(c, max_segments, max_instances, min_overlap, min_size); });
}
int gsx_assoc_view(gsx_ctx* ctx, const gsx_camera* cam, const void* seg, int32_t seg_dtype, int32_t seg_w, int32_t seg_h, int32_t img_w,
                   int32_t img_h, int32_t* remap_out, void* map_out_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__,
                      [&] { return gsx::assoc_view(c, cam, seg, seg_dtype, seg_w, seg_h, img_w, img_h, remap_out, map_out_dev, false); });
}
int gsx_assoc_view_device(gsx_ctx* ctx, const gsx_camera* cam, const void* seg_dev, int32_t seg_dtype, int32_t seg_w, int32_t seg_h,
                          int32_t img_w, int32_t img_h, int32_t* remap_out, void* map_out_dev) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__,
                      [&] { return gsx::assoc_view(c, cam, seg_dev, seg_dtype, seg_w, seg_h, img_w, img_h, remap_out, map_out_dev, true); });
}
int32_t gsx_assoc_num_views(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c && c->assoc.begun ? c->assoc.views : 0;
}
int32_t gsx_assoc_num_instances(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c && c->assoc.begun ? c->assoc.instances : 0;
}
int64_t gsx_assoc_num_dropped(const gsx_ctx* ctx) {
    const Ctx* c = reinterpret_cast<const Ctx*>(ctx);
    return c && c->assoc.begun ? (int64_t)c->assoc.dropped : 0;
}
int gsx_assoc_ids(gsx_ctx* ctx, int32_t* gid_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::assoc_ids(c, gid_out); });
}
int gsx_assoc_table(gsx_ctx* ctx, uint32_t* table_out) {
    CTX_OR_FAIL(ctx);
    return gsx::guard(c, __func__, [&] { return gsx::assoc_table(c, table_out); });
}
int gsx_debug_assoc_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_assoc_constants: NULL argument");
    gsx::assoc_constants(out);
    return GSX_OK;
}
int gsx_debug_lift_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_lift_constants: NULL argument");
    gsx::lift_constants(out);
    return GSX_OK;
}
int gsx_debug_segpack_constants(int32_t* out) {
    if (!out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_segpack_constants: NULL argument");
    gsx::segpack_constants(out);
    return GSX_OK;
}

int gsx_vote_culled(gsx_ctx* ctx, int64_t* wave_views, int32_t reset) {
    CTX_OR_FAIL(ctx);
    if (!wave_views) return gsx::fail(c, GSX_E_INVALID, "vote_culled: NULL argument");
    return gsx::guard(c, __func__, [&] { return gsx::vote_culled(c, wave_views, reset != 0); });
}

int gsx_debug_filter_check(gsx_ctx* ctx, double* out) {
    CTX_OR_FAIL(ctx);
    if (!out) return gsx::fail(c, GSX_E_INVALID, "debug_filter_check: NULL argument");
    return gsx::guard(c, __func__, [&] { return gsx::filter_check(c, out); });
}

int gsx_debug_cull_planes(const gsx_camera* cam, double* out) {
    if (!cam || !out) return gsx::fail(nullptr, GSX_E_INVALID, "debug_cull_planes: NULL argument");
    gsx::debug_cull_planes(cam, out);
    return GSX_OK;
}

int gsx_debug_sort_pairs(gsx_ctx* ctx, uint32_t* keys, uint32_t* values, int64_t n, int32_t bits) {
    CTX_OR_FAIL(ctx);
    if (n < 0 || bits < 0 || bits > 32 || (n > 0 && (!keys || !values)))
        return gsx::fail(c, GSX_E_INVALID, "debug_sort_pairs: bad arguments");
    if (n == 0) return GSX_OK;
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf k0, v0, k1, v1;
    const size_t nb = sizeof(uint32_t) * (size_t)n;
    GSX_HIP(c, k0.ensure(nb));
    GSX_HIP(c, v0.ensure(nb));
    GSX_HIP(c, k1.ensure(nb));
    GSX_HIP(c, v1.ensure(nb));
    GSX_HIP(c, hipMemcpyAsync(k0.p, keys, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(v0.p, values, nb, hipMemcpyHostToDevice, c->stream));
    int where = 0;
    int rc = gsx::radix_sort_pairs(c, k0.as<uint32_t>(), v0.as<uint32_t>(), k1.as<uint32_t>(), v1.as<uint32_t>(), n, bits,
                                   &where);
    if (rc) return rc;
    GSX_HIP(c, hipMemcpyAsync(keys, where ? k1.p : k0.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(values, where ? v1.p : v0.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

int gsx_debug_sort_pairs_drop(gsx_ctx* ctx, uint32_t* keys, uint32_t* values, int64_t n, int32_t bits, int64_t* kept_out) {
    CTX_OR_FAIL(ctx);
    if (n < 1 || bits < 1 || bits > 32 || !keys || !values || !kept_out)
        return gsx::fail(c, GSX_E_INVALID, "debug_sort_pairs_drop: bad arguments");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf k0, v0, k1, v1, cnt;
    const size_t nb = sizeof(uint32_t) * (size_t)n;
    GSX_HIP(c, k0.ensure(nb));
    GSX_HIP(c, v0.ensure(nb));
    GSX_HIP(c, k1.ensure(nb));
    GSX_HIP(c, v1.ensure(nb));
    GSX_HIP(c, cnt.ensure(8));
    GSX_HIP(c, hipMemcpyAsync(k0.p, keys, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(v0.p, values, nb, hipMemcpyHostToDevice, c->stream));
    // (the result's slots behind the kept elements are not written: let them read as 0xff bytes, never as stale memory)
    GSX_HIP(c, hipMemsetAsync(k1.p, 0xff, nb, c->stream));
    GSX_HIP(c, hipMemsetAsync(v1.p, 0xff, nb, c->stream));
    int where = 0;
    int rc = gsx::radix_sort_pairs_drop(c, k0.as<uint32_t>(), v0.as<uint32_t>(), k1.as<uint32_t>(), v1.as<uint32_t>(), n, nullptr,
                                        bits, &where, cnt.as<unsigned long long>());
    if (rc) return rc;
    unsigned long long kept = 0;
    GSX_HIP(c, hipMemcpyAsync(&kept, cnt.p, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(keys, where ? k1.p : k0.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(values, where ? v1.p : v0.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    *kept_out = (int64_t)kept;
    return GSX_OK;
}

// The count lives on the device, the launch is sized for the capacity (what every frame of the rasterizer does): the whole
// result buffer comes back, with the slots the sort must not have touched.
int gsx_debug_sort_pairs_dev(gsx_ctx* ctx, uint32_t* keys, uint32_t* values, int64_t capacity, int64_t count, int32_t bits,
                             int32_t* where_out) {
    CTX_OR_FAIL(ctx);
    if (capacity < 1 || count < 0 || bits < 1 || bits > 32 || !keys || !values || !where_out)
        return gsx::fail(c, GSX_E_INVALID, "debug_sort_pairs_dev: bad arguments");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf k0, v0, k1, v1, cnt;
    const size_t nb = sizeof(uint32_t) * (size_t)capacity;
    GSX_HIP(c, k0.ensure(nb));
    GSX_HIP(c, v0.ensure(nb));
    GSX_HIP(c, k1.ensure(nb));
    GSX_HIP(c, v1.ensure(nb));
    GSX_HIP(c, cnt.ensure(8));
    const unsigned long long count_host = (unsigned long long)count;
    GSX_HIP(c, hipMemcpyAsync(cnt.p, &count_host, 8, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(k0.p, keys, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(v0.p, values, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemsetAsync(k1.p, 0xff, nb, c->stream));
    GSX_HIP(c, hipMemsetAsync(v1.p, 0xff, nb, c->stream));
    int where = 0;
    int rc = gsx::radix_sort_pairs_dev(c, k0.as<uint32_t>(), v0.as<uint32_t>(), k1.as<uint32_t>(), v1.as<uint32_t>(), capacity,
                                       cnt.as<unsigned long long>(), bits, &where);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);  // count_host and the buffers go away
        return rc;
    }
    GSX_HIP(c, hipMemcpyAsync(keys, where ? k1.p : k0.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(values, where ? v1.p : v0.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    *where_out = where;
    return GSX_OK;
}

int gsx_debug_sort_values_wide(gsx_ctx* ctx, const uint32_t* keys, const uint32_t* values, int64_t capacity, int64_t count,
                               int32_t bits, int32_t nranges, uint32_t* values_out, int32_t* ranges_out) {
    CTX_OR_FAIL(ctx);
    if (capacity < 1 || count < 0 || bits < 1 || bits > 11 || nranges < 1 || nranges > 2048 || !keys || !values || !values_out ||
        !ranges_out)
        return gsx::fail(c, GSX_E_INVALID, "debug_sort_values_wide: bad arguments");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf k0, v0, v1, rg, cnt;
    const size_t nb = sizeof(uint32_t) * (size_t)capacity, rb = sizeof(int2) * (size_t)nranges;
    GSX_HIP(c, k0.ensure(nb));
    GSX_HIP(c, v0.ensure(nb));
    GSX_HIP(c, v1.ensure(nb));
    GSX_HIP(c, rg.ensure(rb));
    GSX_HIP(c, cnt.ensure(8));
    const unsigned long long count_host = (unsigned long long)count;
    GSX_HIP(c, hipMemcpyAsync(cnt.p, &count_host, 8, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(k0.p, keys, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(v0.p, values, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemsetAsync(v1.p, 0xff, nb, c->stream));
    GSX_HIP(c, hipMemsetAsync(rg.p, 0xa5, rb, c->stream));  // (a range the sort does not write must not read as (0, 0))
    int rc = gsx::radix_sort_values_wide(c, k0.as<uint32_t>(), v0.as<uint32_t>(), v1.as<uint32_t>(), capacity,
                                         cnt.as<unsigned long long>(), bits, rg.as<int2>(), nranges);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    GSX_HIP(c, hipMemcpyAsync(values_out, v1.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(ranges_out, rg.p, rb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

int gsx_debug_exclusive_scan(gsx_ctx* ctx, const uint32_t* in, int64_t n, uint32_t* out, uint64_t* grand_out) {
    CTX_OR_FAIL(ctx);
    if (n < 1 || n > ((int64_t)1 << 31) || !in || !out || !grand_out)
        return gsx::fail(c, GSX_E_INVALID, "debug_exclusive_scan: bad arguments");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf din, dout, grand;
    const size_t nb = sizeof(uint32_t) * (size_t)n;
    GSX_HIP(c, din.ensure(nb));
    GSX_HIP(c, dout.ensure(nb));
    GSX_HIP(c, grand.ensure(8));
    GSX_HIP(c, hipMemcpyAsync(din.p, in, nb, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemsetAsync(dout.p, 0xff, nb, c->stream));
    GSX_HIP(c, hipMemsetAsync(grand.p, 0xff, 8, c->stream));
    int rc = gsx::debug_exclusive_scan(c, din.as<uint32_t>(), dout.as<uint32_t>(), n, grand.as<unsigned long long>());
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    unsigned long long g = 0;
    GSX_HIP(c, hipMemcpyAsync(out, dout.p, nb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(&g, grand.p, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    *grand_out = (uint64_t)g;
    return GSX_OK;
}

int gsx_debug_ranges(gsx_ctx* ctx, const uint32_t* sorted_keys, int64_t capacity, int64_t total, int32_t nlists, int32_t* ranges_out) {
    CTX_OR_FAIL(ctx);
    if (capacity < 1 || capacity > 0x7fffffff || total < 0 || nlists < 1 || !sorted_keys || !ranges_out)
        return gsx::fail(c, GSX_E_INVALID, "debug_ranges: bad arguments");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::DevBuf dk, rg, tot;
    const size_t nb = sizeof(uint32_t) * (size_t)capacity, rb = sizeof(int2) * (size_t)nlists;
    GSX_HIP(c, dk.ensure(nb));
    GSX_HIP(c, rg.ensure(rb));
    GSX_HIP(c, tot.ensure(8));
    const unsigned long long total_host = (unsigned long long)total;
    GSX_HIP(c, hipMemcpyAsync(tot.p, &total_host, 8, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemcpyAsync(dk.p, sorted_keys, nb, hipMemcpyHostToDevice, c->stream));
    int rc = gsx::debug_ranges(c, dk.as<uint32_t>(), tot.as<unsigned long long>(), capacity, nlists, rg.as<int2>());
    if (rc) {
        (void)hipStreamSynchronize(c->stream);
        return rc;
    }
    GSX_HIP(c, hipMemcpyAsync(ranges_out, rg.p, rb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

// Everything comes from the caller and is checked here, on the host, before a kernel sees it: the kernels trust the pre pass and
// the level-1 sort for in-range indices and rectangles, a test's arrays get no such trust.
int gsx_debug_bin(gsx_ctx* ctx, int64_t n, const uint32_t* tile_rect, const float* rec, const uint32_t* by_depth, int64_t len,
                  int64_t nvis, int64_t div0, int64_t div1, int64_t m_cap, int32_t height, int32_t tiles_x, int32_t tiles_y,
                  int32_t bin32, int32_t exact, const uint8_t* sat, int64_t pair_cap, uint32_t* count_out, uint64_t* total_out,
                  uint32_t* keys_out, uint32_t* vals_out) {
    CTX_OR_FAIL(ctx);
    if (n < 1 || n > ((int64_t)1 << 28) || !tile_rect || !by_depth || len < 0 || len > ((int64_t)1 << 31) || nvis < 0 || nvis > len ||
        !count_out || !total_out || !keys_out || !vals_out)
        return gsx::fail(c, GSX_E_INVALID, "debug_bin: bad arguments (n, len, nvis <= len, NULL array)");
    if (tiles_x < 1 || tiles_x > 256 || tiles_y < 1 || tiles_y > 256 || height < 1)
        return gsx::fail(c, GSX_E_INVALID, "debug_bin: %d x %d tiles, height %d: 1..256 tiles per side", tiles_x, tiles_y, height);
    if (div0 < 0 || div1 < 1) return gsx::fail(c, GSX_E_INVALID, "debug_bin: div0 %lld < 0 or div1 %lld < 1", (long long)div0, (long long)div1);
    const int64_t phase_len = nvis / div1 - (div0 ? nvis / div0 : 0);
    if (m_cap < 1 || m_cap > ((int64_t)1 << 31) || m_cap < phase_len)
        return gsx::fail(c, GSX_E_INVALID, "debug_bin: m_cap %lld does not cover the phase's %lld splats", (long long)m_cap, (long long)phase_len);
    if (pair_cap < 1 || pair_cap > 0x7fffffff) return gsx::fail(c, GSX_E_INVALID, "debug_bin: pair_cap %lld outside [1, 2^31 - 1]", (long long)pair_cap);
    if (bin32 && exact) return gsx::fail(c, GSX_E_INVALID, "debug_bin: bin32 with exact is never launched");
    if (exact && !rec) return gsx::fail(c, GSX_E_INVALID, "debug_bin: exact needs rec");
    for (int64_t j = 0; j < nvis; ++j)
        if ((int64_t)by_depth[j] >= n) return gsx::fail(c, GSX_E_INVALID, "debug_bin: by_depth[%lld] = %u >= n", (long long)j, by_depth[j]);
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t r = tile_rect[i], tx0 = r & 255u, tx1 = (r >> 8) & 255u, ty0 = (r >> 16) & 255u, ty1 = r >> 24;
        if (tx1 >= tx0 && ty1 >= ty0 && ((int)tx1 >= tiles_x || (int)ty1 >= tiles_y))
            return gsx::fail(c, GSX_E_INVALID, "debug_bin: rectangle %lld (%u..%u, %u..%u) outside the frame's tiles", (long long)i, tx0, tx1, ty0, ty1);
    }
    GSX_HIP(c, hipSetDevice(c->device));
    const int lists = bin32 ? ((tiles_x + 1) / 2) * ((tiles_y + 1) / 2) : tiles_x * tiles_y;
    const size_t sat_bytes = bin32 ? 4 * (size_t)lists : (size_t)lists;
    const size_t nb = sizeof(uint32_t) * (size_t)n, lb = sizeof(uint32_t) * (size_t)(len > 0 ? len : 1);
    const size_t mb = sizeof(uint32_t) * (size_t)m_cap, pb = sizeof(uint32_t) * (size_t)pair_cap;
    gsx::DevBuf drect, drec, dorder, dsat, dcount, doffset, dseq, dkeys, dvals, dsmall;
    GSX_HIP(c, drect.ensure(nb));
    if (rec) GSX_HIP(c, drec.ensure(12 * sizeof(float) * (size_t)n));
    GSX_HIP(c, dorder.ensure(lb));
    if (sat) GSX_HIP(c, dsat.ensure(sat_bytes));
    GSX_HIP(c, dcount.ensure(mb));
    GSX_HIP(c, doffset.ensure(mb));
    GSX_HIP(c, dseq.ensure(mb));
    GSX_HIP(c, dkeys.ensure(pb));
    GSX_HIP(c, dvals.ensure(pb));
    GSX_HIP(c, dsmall.ensure(16));  // u64 nvis, u64 pair total
    const unsigned long long nvis_host = (unsigned long long)nvis;
    GSX_HIP(c, hipMemcpyAsync(drect.p, tile_rect, nb, hipMemcpyHostToDevice, c->stream));
    if (rec) GSX_HIP(c, hipMemcpyAsync(drec.p, rec, 12 * sizeof(float) * (size_t)n, hipMemcpyHostToDevice, c->stream));
    if (len > 0) GSX_HIP(c, hipMemcpyAsync(dorder.p, by_depth, sizeof(uint32_t) * (size_t)len, hipMemcpyHostToDevice, c->stream));
    if (sat) GSX_HIP(c, hipMemcpyAsync(dsat.p, sat, sat_bytes, hipMemcpyHostToDevice, c->stream));
    GSX_HIP(c, hipMemsetAsync(dcount.p, 0xff, mb, c->stream));
    GSX_HIP(c, hipMemsetAsync(doffset.p, 0xff, mb, c->stream));
    GSX_HIP(c, hipMemsetAsync(dseq.p, 0xff, mb, c->stream));
    GSX_HIP(c, hipMemsetAsync(dkeys.p, 0xff, pb, c->stream));
    GSX_HIP(c, hipMemsetAsync(dvals.p, 0xff, pb, c->stream));
    GSX_HIP(c, hipMemsetAsync(dsmall.p, 0xff, 16, c->stream));
    GSX_HIP(c, hipMemcpyAsync(dsmall.p, &nvis_host, 8, hipMemcpyHostToDevice, c->stream));
    gsx::BinPhaseArgs a;
    a.nvis_dev = dsmall.as<unsigned long long>();
    a.div0 = div0;
    a.div1 = div1;
    a.m_cap = m_cap;
    a.by_depth = dorder.as<uint32_t>();
    a.tile_rect = drect.as<uint32_t>();
    a.rec = rec ? drec.as<float4>() : nullptr;
    a.H = height;
    a.tiles_x = tiles_x;
    a.bin32 = bin32 ? 1 : 0;
    a.exact = exact ? 1 : 0;
    a.sat = sat ? dsat.as<uint8_t>() : nullptr;
    a.count = dcount.as<uint32_t>();
    a.offset = doffset.as<uint32_t>();
    a.rect_seq = dseq.as<uint32_t>();
    a.keys = dkeys.as<uint32_t>();
    a.vals = dvals.as<uint32_t>();
    a.total_dev = dsmall.as<unsigned long long>() + 1;
    a.pair_cap = (unsigned long long)pair_cap;
    int rc = gsx::debug_bin(c, a);
    if (rc) {
        (void)hipStreamSynchronize(c->stream);  // nvis_host and the buffers go away
        return rc;
    }
    unsigned long long total = 0;
    GSX_HIP(c, hipMemcpyAsync(count_out, dcount.p, mb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(&total, a.total_dev, 8, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(keys_out, dkeys.p, pb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipMemcpyAsync(vals_out, dvals.p, pb, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    *total_out = (uint64_t)total;
    return GSX_OK;
}

int gsx_debug_spatial_order(gsx_ctx* ctx, uint32_t* perm_out) {
    CTX_OR_FAIL(ctx);
    if (!perm_out) return gsx::fail(c, GSX_E_INVALID, "debug_spatial_order: perm_out is NULL");
    if (!c->sorted || c->n < 2)
        return gsx::fail(c, GSX_E_INVALID, "debug_spatial_order: the context holds no sorted order (fewer than two positions, or the option "
                                           "\"spatial_sort\" was off at the upload)");
    GSX_HIP(c, hipSetDevice(c->device));
    GSX_HIP(c, hipMemcpyAsync(perm_out, c->perm.p, sizeof(uint32_t) * (size_t)c->n, hipMemcpyDeviceToHost, c->stream));
    GSX_HIP(c, hipStreamSynchronize(c->stream));
    return GSX_OK;
}

// ---- profiling -----------------------------------------------------------------------------------
int gsx_profile_enable(gsx_ctx* ctx, int on) {
    CTX_OR_FAIL(ctx);
    c->prof_on = on != 0;
    return GSX_OK;
}
int gsx_profile_reset(gsx_ctx* ctx) {
    CTX_OR_FAIL(ctx);
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::prof_drain(c);
    c->prof_acc.clear();
    return GSX_OK;
}
const char* gsx_profile_name(gsx_ctx* ctx, int32_t index) {
    Ctx* c = reinterpret_cast<Ctx*>(ctx);
    if (!c || index < 0 || (size_t)index >= c->prof_names.size()) return nullptr;
    return c->prof_names[(size_t)index].c_str();
}
int gsx_profile_get(gsx_ctx* ctx, const char* name, int64_t* launches, double* total_ms) {
    CTX_OR_FAIL(ctx);
    if (!name) return gsx::fail(c, GSX_E_INVALID, "profile_get: name is NULL");
    GSX_HIP(c, hipSetDevice(c->device));
    gsx::prof_drain(c);
    auto it = c->prof_acc.find(name);
    if (launches) *launches = it == c->prof_acc.end() ? 0 : it->second.first;
    if (total_ms) *total_ms = it == c->prof_acc.end() ? 0.0 : it->second.second;
    return GSX_OK;
}

}  // extern "C"
