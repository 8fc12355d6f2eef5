// nerf_api.hip -- the C ABI of libnerf_mi355.so (include/nerf_mi355.h): context, weight upload,
// scratch arena and the orchestration of the render path (field queries: field_api.hip; isosurface, radiance volume: beside their kernels)
//   NeRF.render        src/NeRF.py:109-134
//   NeRF.render_image  src/NeRF.py:190-246
//   render_rays        src/UtilsNeuralRadianceField.py:181-211
// on one HIP stream.  No CPU compute path exists here: without a gfx950 device every call fails.
#include "../../include/nerf_mi355.h"

#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "nerf_ctx.h"

using namespace nerf;

thread_local std::string g_err;

namespace nerf {

int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

int ensure(nerf_ctx* c, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return 0;
    // a grow may free memory a still-running kernel uses: drain the stream first
    HIP_OK(hipStreamSynchronize(c->stream));
    if (b.p) HIP_OK(hipFree(b.p));
    b.p = nullptr; b.cap = 0;
    size_t want = bytes + bytes / 8;
    HIP_OK(hipMalloc(&b.p, want));
    b.cap = want;
    return 0;
}

int h2d(nerf_ctx* c, DevBuf& b, const void* src, size_t bytes) {
    if (int r = ensure(c, b, bytes)) return r;
    HIP_OK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, c->stream));
    return 0;
}

int copy_to_caller(nerf_ctx* c, void* dst, const void* src_dev, size_t bytes, int mem) {
    HIP_OK(hipMemcpyAsync(dst, src_dev, bytes, mem == NERF_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

int copy_from_caller(nerf_ctx* c, void* dst_dev, const void* src, size_t bytes, int mem) {
    HIP_OK(hipMemcpyAsync(dst_dev, src, bytes, mem == NERF_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
    return 0;
}

Staging::Staging(nerf_ctx* c, int mem) : c(c), host(mem == NERF_MEM_HOST) {}

void* Staging::stage(DevBuf& b, void* caller, size_t bytes, bool upload) {
    if (!caller || err) return nullptr;
    if (!host) return caller;
    if (upload) {
        err = h2d(c, b, caller, bytes);
    } else if (n_back == (int)(sizeof back / sizeof back[0])) {
        err = fail("internal: more than %d staged outputs in one call", n_back);
    } else if (!(err = ensure(c, b, bytes))) {
        back[n_back].dst = caller; back[n_back].src = b.p; back[n_back].bytes = bytes;
        ++n_back;
    }
    return err ? nullptr : b.p;
}

int Staging::finish() {
    if (!host) return 0;
    for (int i = 0; i < n_back; ++i) HIP_OK(hipMemcpyAsync(back[i].dst, back[i].src, back[i].bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int enter(nerf_ctx* c) {
    if (!c) return fail("ctx is NULL");
    HIP_OK(hipSetDevice(c->cfg.device));
    return 0;
}

int sampling_ok(const nerf_ctx* c) {
    // 1/near: checked where depths are drawn as well as in the setter, since nerf_ctx_set_bounds may come after it
    if (c->sampling == NERF_SAMPLING_LINDISP && !(c->cfg.near_boundary > 0.f)) return fail("lindisp needs near_boundary > 0");
    return 0;
}

int draw_z_values(nerf_ctx* c, const float* o, const float* d, long long N, int S, const float* u, uint64_t seed,
                  long long ray_base, float* z) {
    const float* bounds = nullptr;
    const int* state = nullptr;
    if (c->box_on && c->grid_R > 0 && o && d && N > 0) {
        // the walk through the grid is made once per ray, into the ctx's own scratch; the depth kernel reads the result
        if (int r = ensure(c, c->b_gbounds, (size_t)N * 8)) return r;
        if (int r = ensure(c, c->b_gstate, (size_t)N * 4)) return r;
        launch_ray_grid_bounds(c->box, c->cfg.near_boundary, c->cfg.far_boundary, (const uint32_t*)c->b_grid[c->grid_cur].p,
                               c->grid_R, o, d, N, (float*)c->b_gbounds.p, (int*)c->b_gstate.p, c->stream);
        bounds = (const float*)c->b_gbounds.p;
        state = (const int*)c->b_gstate.p;
    }
    launch_z_values(c->cfg.near_boundary, c->cfg.far_boundary, c->sampling == NERF_SAMPLING_LINDISP, N, S, u, seed, ray_base,
                    z, c->stream, o, d, c->box_on ? &c->box : nullptr, bounds, state);
    return 0;
}

// with timing on: the next event of the culled render passes' pool (six per pass, read by nerf_ctx_read_culling_timing)
static int cull_stamp(nerf_ctx* c, bool stamp = true) {
    if (!stamp || !c->timing) return 0;
    if (c->cull_ev_used == c->cull_ev.size()) {
        hipEvent_t e;
        HIP_OK(hipEventCreate(&e));
        c->cull_ev.push_back(e);
    }
    HIP_OK(hipEventRecord(c->cull_ev[c->cull_ev_used++], c->stream));
    return 0;
}

// Verdict bits -> scan -> the row count M, read by the host because every kernel downstream takes it by value -> the kept
// samples' points and directions as compact rows.  Four stage events: before the verdicts, after the scan, after the read and
// the growth of the compact buffers, after the gather.
int compact_samples(nerf_ctx* c, SampleCompaction& rec, const float* o, const float* d, const float* z, long long N, int S,
                    bool stamp) {
    const long long total = N * S;
    if (total > (long long)INT32_MAX) return fail("sample culling: %lld samples in one pass do not fit int32", total);
    const long long words = (total + 63) / 64, mask_bytes = words * 8;
    const size_t tiles = scan_sums_words(mask_bytes);
    if (int r = ensure(c, rec.mask, (size_t)mask_bytes)) return r;
    if (int r = ensure(c, rec.first, (size_t)mask_bytes * 4)) return r;
    if (int r = ensure(c, c->b_csums, (tiles + 1) * 4)) return r;
    if (!c->cull_rows) HIP_OK(hipHostMalloc((void**)&c->cull_rows, sizeof(uint32_t), hipHostMallocDefault));
    const uint8_t* mask = (const uint8_t*)rec.mask.p;
    uint32_t *first = (uint32_t*)rec.first.p, *sums = (uint32_t*)c->b_csums.p;
    if (int r = cull_stamp(c, stamp)) return r;
    launch_sample_keep(c->box, (const uint32_t*)c->b_grid[c->grid_cur].p, c->grid_R, o, d, z, N, S, (uint64_t*)rec.mask.p,
                       nullptr, c->stream);
    launch_scan_popc(mask, mask_bytes, sums, first, sums + tiles, c->stream);
    HIP_OK(hipGetLastError());
    if (int r = cull_stamp(c, stamp)) return r;
    HIP_OK(hipMemcpyAsync(c->cull_rows, sums + tiles, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    const long long M = *c->cull_rows;
    if (M > total) return fail("internal: sample culling kept %lld of %lld samples", M, total);
    rec.rows = M;
    c->cull_samples += total;
    c->cull_kept += M;
    const bool with_dirs = c->cfg.n_angles != 0;
    if (M > 0) {      // the compact buffers follow M, not N * S
        if (int r = ensure(c, c->b_cxyz, (size_t)M * 12)) return r;
        if (with_dirs) if (int r = ensure(c, c->b_cdirs, (size_t)M * 12)) return r;
    }
    if (int r = cull_stamp(c, stamp)) return r;
    if (M > 0)
        launch_sample_gather(o, d, z, N, S, mask, first, (float*)c->b_cxyz.p, with_dirs ? (float*)c->b_cdirs.p : nullptr, c->stream);
    HIP_OK(hipGetLastError());
    return cull_stamp(c, stamp);
}

int ensure_render_tables(nerf_ctx* c) {
    if (c->rt_built) return 0;
    StreamTables t;
    build_stream_tables(c->cfg.n_pos_enc_xyz, c->cfg.n_pos_enc_dir, c->cfg.n_angles, t);
    auto up = [&](const std::vector<int32_t>& v, int32_t** dst) -> int {      // (blocking: the host table dies with this call)
        if (v.empty()) return 0;
        if (!*dst) HIP_OK(hipMalloc((void**)dst, v.size() * sizeof(int32_t)));
        HIP_OK(hipMemcpy(*dst, v.data(), v.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        return 0;
    };
    for (int k = 0; k < kStreamKinds; ++k) if (int r = up(t.stream[k], &c->rt[k])) return r;
    for (int b = 0; b < kConstBlocks; ++b) if (int r = up(t.cst[b], &c->rt_cst[b])) return r;
    c->rt_built = true;
    return 0;
}

int repack_render_streams(nerf_ctx* c, int which, const float* dev_blob) {
    if (int r = ensure_render_tables(c)) return r;
    NetWeights& n = c->net[which];
    {   // new weights: what the rgb-skipping kernel's gate knew is about the old ones (a copy still in flight included)
        RgbSkipGate& g = c->skip_gate[which];
        g.full_left = g.since_copy = 0;
        g.known = false;
        g.discard = g.pending;
    }
    StreamDesc d[kStreamKinds];
    render_streams(c->cfg.n_pos_enc_xyz, c->cfg.n_angles, which, d);
    for (int k = 0; k < kStreamKinds; ++k) {
        if (!d[k].bytes) continue;
        const int32_t *tab = c->rt[d[k].table], *ctab = c->rt_cst[d[k].cst];
        if (!tab || !ctab) return fail("internal: no gather table for stream kind %d of network %d", k, which);
        if (!n.stream[k]) HIP_OK(hipMalloc(&n.stream[k], d[k].bytes));
        if (!n.cst[d[k].cst]) HIP_OK(hipMalloc((void**)&n.cst[d[k].cst], kConstBytes));
        // (every kind of a block writes the block's constants: the same values, in stream order)
        launch_repack(d[k].elem, dev_blob, window_scale(c), tab, n.stream[k], d[k].bytes / (d[k].elem == kElemF32 ? 4 : 2), ctab,
                      n.cst[d[k].cst], c->stream);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace nerf

namespace {

// The kernel that renders a network of `cfg` in `precision`: its operand stream, its constant block and its launcher.
// want_sigma asks for the sigma-only kernel (f16x3 / bf16x3, the kLx build, n_angles 1 or 2; the coarse network alone keeps its
// stream); sigma_only says whether that is what came back: raw then receives sigma alone, (M,) floats.
// rgb_unread says that nothing reads the rgb of a sample whose weight is exactly 0 (the composite's pixel sum is the only
// reader: no rgb_samples): f16x3, the kLx build and n_angles 1 or 2 then render with the rgb-skipping kernel (mlp_f16x3.hip),
// either network; same raw layout, same pixels.
struct RenderKernel {
    StreamKind stream;
    ConstBlock cst;
    void (*launch)(const MlpArgs& a, int num_cus, hipStream_t s, bool xyz_only, unsigned long long* skip_count);   // (the last: rgb-skipping kernel only)
    bool sigma_only;
};
// -> 0; 1: the config has no kernel of that precision; 2: no such precision (nerf_last_error() says which, either way)
int pick_render_kernel(const nerf_config& cfg, int precision, bool want_sigma, RenderKernel* k, bool rgb_unread = false) {
    const bool wide_pe = cfg.n_pos_enc_xyz > kLx, sig = want_sigma && !wide_pe && cfg.n_angles != 0;
    const bool skip = rgb_unread && !wide_pe && cfg.n_angles != 0;
    switch (precision) {
    case NERF_PRECISION_FP32:
        if (wide_pe)
            return fail("n_pos_enc_dim_xyz %d (> %d) renders with the 16-bit-core kernels only: precision f16x3, bf16x3 or f16, not fp32",
                        cfg.n_pos_enc_xyz, kLx);
        *k = {kFp32, kConstFp32, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { launch_mlp_fp32(a, n, s, x); }, false};
        return 0;
    case NERF_PRECISION_F16X3:
        if (sig) *k = {kF16x3Sig, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool, unsigned long long*) { launch_mlp_f16x3_sig(a, n, s); }, true};
        else if (skip) *k = {kF16x3Skip, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool, unsigned long long* sc) { launch_mlp_f16x3_rgbskip(a, n, s, sc); }, false};
        else if (wide_pe) *k = {kF16x3, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { wide::launch_mlp_f16x3(a, n, s, false, x); }, false};
        else *k = {kF16x3, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { launch_mlp_f16x3(a, n, s, false, x); }, false};
        return 0;
    case NERF_PRECISION_F16: {
        // two sample tiles per wave (half the weight stream per row) unless NERF_F16_TILES=1 asks for the one-tile kernel;
        // the xyz-only network and the wide-PE build have the one-tile variant only
        static const bool one_tile = [] { const char* e = getenv("NERF_F16_TILES"); return e && e[0] == '1'; }();
        if (wide_pe) *k = {kF16Hi, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { wide::launch_mlp_f16x3(a, n, s, true, x); }, false};
        else if (cfg.n_angles != 0 && !one_tile) *k = {kF16Hi, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool, unsigned long long*) { launch_mlp_f16_2t(a, n, s); }, false};
        else *k = {kF16Hi, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { launch_mlp_f16x3(a, n, s, true, x); }, false};
        return 0;
    }
    case NERF_PRECISION_BF16X3:
        if (sig) *k = {kBf16x3Sig, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool, unsigned long long*) { bf16::launch_mlp_bf16x3_sig(a, n, s); }, true};
        else if (wide_pe) *k = {kBf16x3, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { bf16::wide::launch_mlp_bf16x3(a, n, s, x); }, false};
        else *k = {kBf16x3, kConst16, [](const MlpArgs& a, int n, hipStream_t s, bool x, unsigned long long*) { bf16::launch_mlp_bf16x3(a, n, s, x); }, false};
        return 0;
    }
    fail("unknown precision %d", precision);
    return 2;
}

int check_cfg(const nerf_config* cfg) {
    if (!cfg) return fail("nerf_config is NULL");
    if (cfg->n_angles != 2 && cfg->n_angles != 1 && cfg->n_angles != 0)
        return fail("n_angles_for_model should be 1 or 2.");   // message of src/UtilsCV.py:138 (0 = xyz-only network)
    if (cfg->n_pos_enc_xyz < 1 || cfg->n_pos_enc_xyz > kLxWide || cfg->n_pos_enc_dir < 1 || cfg->n_pos_enc_dir > kLd ||
        cfg->hidden_dim != kHidden || cfg->last_hidden_dim != kLast)
        return fail("supported networks: n_pos_enc_dim_xyz 1..%d, n_pos_enc_view_dir 1..%d, hidden %d, last hidden %d "
                    "(got %d %d %d %d)", kLxWide, kLd, kHidden, kLast, cfg->n_pos_enc_xyz, cfg->n_pos_enc_dir, cfg->hidden_dim,
                    cfg->last_hidden_dim);
    RenderKernel k;      // a precision this config has no kernel for is nerf_ctx_create's to refuse: a blob still has a size
    if (pick_render_kernel(*cfg, cfg->precision, false, &k) == 2)
        return fail("unknown precision %d (NERF_PRECISION_FP32 = 0, NERF_PRECISION_F16X3 = 1, NERF_PRECISION_F16 = 2, "
                    "NERF_PRECISION_BF16X3 = 3)", cfg->precision);
    return 0;
}

// record the MLP launch between two events when timing is on
int run_mlp(nerf_ctx* c, int which, const RenderKernel& k, const float* in_a, const float* in_b, const float* z, float* raw,
            long long M, int S, int mode) {
    if (!c->net[which].loaded) return fail("network %d has no weights loaded", which);
    if (int r = train_flush_weights(c, which)) return r;   // re-pack the operand streams after optimizer steps
    MlpArgs a{};
    a.wstream = (const float*)c->net[which].stream[k.stream];
    a.wconst = c->net[which].cst[k.cst];
    if (!a.wstream || !a.wconst) return fail("internal: network %d keeps no stream of kind %d", which, (int)k.stream);
    a.in_a = in_a; a.in_b = in_b; a.z = z; a.raw = raw; a.M = M; a.S = S; a.mode = mode;
    a.nonfinite = c->nonfinite;
    a.alpha = c->cfg.leaky_relu_alpha;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing) {
        if (c->ev_used == c->ev_pool.size()) {
            hipEvent_t x, y;
            HIP_OK(hipEventCreate(&x));
            HIP_OK(hipEventCreate(&y));
            c->ev_pool.emplace_back(x, y);
        }
        e0 = c->ev_pool[c->ev_used].first; e1 = c->ev_pool[c->ev_used].second;
        c->ev_used++;
        c->timed_rows += M;
        HIP_OK(hipEventRecord(e0, c->stream));
    }
    k.launch(a, c->num_cus, c->stream, c->cfg.n_angles == 0, k.stream == kF16x3Skip ? c->skip_gate[which].dev : nullptr);
    if (c->timing) HIP_OK(hipEventRecord(e1, c->stream));
    HIP_OK(hipGetLastError());
    return 0;
}

struct OutSizes { size_t per_ray[7]; };
OutSizes out_sizes(int S) {
    OutSizes o;
    o.per_ray[0] = 3; o.per_ray[1] = S; o.per_ray[2] = S; o.per_ray[3] = S; o.per_ray[4] = 3 * (size_t)S;
    o.per_ray[5] = S; o.per_ray[6] = 1;
    return o;
}
float** out_ptrs(nerf_outputs& o, int i) {
    switch (i) {
        case 0: return &o.rgb; case 1: return &o.weights; case 2: return &o.cumprod; case 3: return &o.alpha;
        case 4: return &o.rgb_samples; case 5: return &o.z; default: return &o.depth;
    }
}

// The device pointers of the requested outputs: member i of a host caller's nerf_outputs is staged on b_out[i].
nerf_outputs stage_outputs(nerf_ctx* c, Staging& st, const nerf_outputs& outs, long long N, int S) {
    const OutSizes sz = out_sizes(S);
    nerf_outputs dev = outs;
    for (int i = 0; i < 7; ++i) {
        float** p = out_ptrs(dev, i);
        *p = st.out(c->b_out[i], *p, sz.per_ray[i] * N * sizeof(float));
    }
    return dev;
}

// Host-memory render_image: the rows [off, off + n) of every requested output leave for the host on the ctx's COPY stream
// as soon as the batch that produced them is done (event), while the next batch computes on the ctx stream.  With
// page-locked destinations (nerf_host_alloc) the copies are DMA transfers that run beside the kernels; pageable
// destinations work too (the runtime stages them) but serialise.
int copy_back_batch(nerf_ctx* c, const nerf_outputs* host, const nerf_outputs* dev, long long off, long long n, int S,
                    size_t batch_index) {
    if (!c->copy_stream) HIP_OK(hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    constexpr size_t kRing = 64;
    if (c->copy_ev.size() < kRing) {
        hipEvent_t e;
        HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        c->copy_ev.push_back(e);
    }
    hipEvent_t ev = c->copy_ev[batch_index % c->copy_ev.size()];
    HIP_OK(hipEventRecord(ev, c->stream));
    HIP_OK(hipStreamWaitEvent(c->copy_stream, ev, 0));
    const OutSizes sz = out_sizes(S);
    nerf_outputs h = host ? *host : nerf_outputs{};
    nerf_outputs d = *dev;
    for (int i = 0; i < 7; ++i) {
        float* hp = *out_ptrs(h, i);
        if (!hp) continue;
        HIP_OK(hipMemcpyAsync(hp + sz.per_ray[i] * off, *out_ptrs(d, i) + sz.per_ray[i] * off,
                              sz.per_ray[i] * n * sizeof(float), hipMemcpyDeviceToHost, c->copy_stream));
    }
    return 0;
}

// network_pass under sample culling (cull_kernels.hip): compact_samples -> the kept samples' points as M mode-1 rows of the same
// kernel pick_render_kernel gives the unculled pass -> the full raw (or sigma) buffer with zeros for the culled samples.
int culled_mlp(nerf_ctx* c, int which, const RenderKernel& k, const float* o, const float* d, const float* z, long long N, int S,
               float* raw) {
    if (!c->net[which].loaded) return fail("network %d has no weights loaded", which);      // run_mlp's, also when M == 0
    if (int r = compact_samples(c, c->cull, o, d, z, N, S, true)) return r;
    const long long M = c->cull.rows;
    if (M > 0) {
        if (int r = ensure(c, c->b_craw, (size_t)M * (k.sigma_only ? 4 : 16))) return r;
        const float* view = c->cfg.n_angles != 0 ? (const float*)c->b_cdirs.p : nullptr;
        if (int r = run_mlp(c, which, k, (const float*)c->b_cxyz.p, view, nullptr, (float*)c->b_craw.p, M, 1, 1)) return r;
    }
    if (int r = cull_stamp(c)) return r;
    launch_raw_expand((const float*)c->b_craw.p, N * S, k.sigma_only, (const uint8_t*)c->cull.mask.p,
                      (const uint32_t*)c->cull.first.p, raw, c->stream);
    return cull_stamp(c);
}

// The network pass of dev_render_rays: raw (N*S, 4) -- sigma_only: (N*S,) -- of every sample.  Under sample culling (on, and
// the ctx holds a grid) it is culled_mlp's; otherwise the one mode-0 launch it always was.
int network_pass(nerf_ctx* c, int which, const RenderKernel& k, const float* o, const float* d, const float* z, long long N, int S,
                 float* raw) {
    if (!(culling_acts(c, c->cull_on) && N > 0)) return run_mlp(c, which, k, o, d, z, raw, N * S, S, 0);
    const size_t ev0 = c->cull_ev_used;
    const int r = culled_mlp(c, which, k, o, d, z, N, S, raw);
    if (r) c->cull_ev_used = ev0;                                  // the stage events count whole passes only
    return r;
}

// The per-launch gate of the rgb-skipping kernel (nerf_ctx.h: RgbSkipGate).  rgb_skip_wanted, before a launch that may use it:
// takes in a counter copy whose event has completed, and says whether this launch runs that kernel (*want) or, the network's
// skipped share having stayed under 1 / kMinShareDen, the full one.  rgb_skip_launched, behind a launch that used it: sends
// the counters to the host unless a copy is in flight or a share is known and fewer than kCopyEvery launches have passed.
// Neither waits for the device.
int rgb_skip_wanted(nerf_ctx* c, int which, bool* want) {
    RgbSkipGate& g = c->skip_gate[which];
    if (!g.dev) {
        HIP_OK(hipMalloc((void**)&g.dev, 2 * sizeof(unsigned long long)));
        HIP_OK(hipMemset(g.dev, 0, 2 * sizeof(unsigned long long)));
        HIP_OK(hipHostMalloc((void**)&g.host, 2 * sizeof(unsigned long long), hipHostMallocDefault));
        HIP_OK(hipEventCreateWithFlags(&g.ev, hipEventDisableTiming));
    }
    if (g.pending) {
        const hipError_t e = hipEventQuery(g.ev);
        if (e == hipErrorNotReady) (void)hipGetLastError();      // still on its way: not an error to keep
        else if (e != hipSuccess) HIP_OK(e);
        else {
            g.pending = false;
            const unsigned long long tiles = g.host[0] - g.seen[0], skipped = g.host[1] - g.seen[1];
            g.seen[0] = g.host[0]; g.seen[1] = g.host[1];
            if (tiles > 0 && !g.discard) {
                g.known = true;
                if (skipped * RgbSkipGate::kMinShareDen < tiles) {
                    g.full_left = RgbSkipGate::kFullRun;
                    g.known = false;                             // the probe behind the full run reports at once
                }
            }
            g.discard = false;
        }
    }
    *want = g.full_left == 0;
    if (g.full_left > 0) --g.full_left;
    return 0;
}
int rgb_skip_launched(nerf_ctx* c, int which) {
    RgbSkipGate& g = c->skip_gate[which];
    if (g.pending || (g.known && ++g.since_copy < RgbSkipGate::kCopyEvery)) return 0;
    g.since_copy = 0;
    HIP_OK(hipMemcpyAsync(g.host, g.dev, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipEventRecord(g.ev, c->stream));
    g.pending = true;
    return 0;
}

// render_rays on device pointers
// A coarse pass whose only output is the weights (the coarse pass of NeRF.render) runs the sigma-only network and the
// weights-only composite where pick_render_kernel has one: the weights depend on sigma alone and come out bit-identical.
int dev_render_rays(nerf_ctx* c, int which, const float* o, const float* d, const float* z, long long N, int S,
                    const nerf_outputs& outs) {
    const bool weights_only = outs.weights && !outs.rgb && !outs.cumprod && !outs.alpha && !outs.rgb_samples && !outs.z &&
                              !outs.depth;
    RenderKernel k;
    if (pick_render_kernel(c->cfg, c->cfg.precision, which == NERF_NET_COARSE && weights_only, &k, outs.rgb && !outs.rgb_samples)) return 1;
    if (k.stream == kF16x3Skip) {      // the gate: a network that skips next to nothing runs the full kernel, same bits
        bool want = true;
        if (int r = rgb_skip_wanted(c, which, &want)) return r;
        if (!want && pick_render_kernel(c->cfg, c->cfg.precision, false, &k)) return 1;
    }
    if (k.sigma_only) {
        if (int r = ensure(c, c->b_raw, (size_t)N * S * sizeof(float))) return r;
        float* sigma = (float*)c->b_raw.p;
        if (int r = network_pass(c, which, k, o, d, z, N, S, sigma)) return r;
        launch_composite_weights(sigma, z, N, S, outs.weights, c->stream);
        HIP_OK(hipGetLastError());
        return 0;
    }
    if (int r = ensure(c, c->b_raw, (size_t)N * S * 4 * sizeof(float))) return r;
    float* raw = (float*)c->b_raw.p;
    if (int r = network_pass(c, which, k, o, d, z, N, S, raw)) return r;
    if (k.stream == kF16x3Skip) if (int r = rgb_skip_launched(c, which)) return r;
    launch_composite(raw, z, N, S, outs.rgb, outs.weights, outs.cumprod, outs.alpha, outs.rgb_samples, outs.depth,
                     c->stream);
    if (outs.z && outs.z != z)
        HIP_OK(hipMemcpyAsync(outs.z, z, (size_t)N * S * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIP_OK(hipGetLastError());
    return 0;
}

// NeRF.render on device pointers (u_* may be NULL -> Philox)
int dev_render(nerf_ctx* c, const float* o, const float* d, long long N, int Sc, int Sf, const float* u_c,
               const float* u_f, uint64_t seed, long long ray_base, const nerf_outputs& outs) {
    const bool fine = Sf > 0 && c->net[NERF_NET_FINE].loaded;
    if (int r = sampling_ok(c)) return r;
    if (int r = ensure(c, c->b_zc, (size_t)N * Sc * sizeof(float))) return r;
    float* zc = (float*)c->b_zc.p;
    if (int r = draw_z_values(c, o, d, N, Sc, u_c, seed, ray_base, zc)) return r;
    if (!fine) return dev_render_rays(c, NERF_NET_COARSE, o, d, zc, N, Sc, outs);
    if (Sc < 2) return fail("hierarchical sampling needs at least 2 coarse samples (got %d)", Sc);
    if (int r = ensure(c, c->b_wc, (size_t)N * Sc * sizeof(float))) return r;
    nerf_outputs co{};
    co.weights = (float*)c->b_wc.p;
    if (int r = dev_render_rays(c, NERF_NET_COARSE, o, d, zc, N, Sc, co)) return r;   // weights only: the sigma-only path
    const int St = Sc + Sf;
    if (int r = ensure(c, c->b_zf, (size_t)N * St * sizeof(float))) return r;
    float* zf = (float*)c->b_zf.p;
    launch_sample_pdf(co.weights, zc, N, Sc, Sf, u_f, seed, ray_base, nullptr, zf, c->stream);
    return dev_render_rays(c, NERF_NET_FINE, o, d, zf, N, St, outs);
}

}  // namespace

// the one way out of this file to run_mlp (nerf_ctx.h): model_predict's kernel on M device-resident rows
int nerf::eval_points(nerf_ctx* c, int which, const float* xyz, const float* view, long long M, float* raw) {
    RenderKernel k;
    if (pick_render_kernel(c->cfg, c->cfg.precision, false, &k)) return 1;
    return run_mlp(c, which, k, xyz, view, nullptr, raw, M, 1, 1);
}

extern "C" {

int nerf_abi_version(void) { return NERF_ABI_VERSION; }
const char* nerf_last_error(void) { return g_err.c_str(); }

size_t nerf_blob_size(const nerf_config* cfg) {
    if (check_cfg(cfg)) return 0;
    return blob_floats(cfg->n_pos_enc_xyz, cfg->n_pos_enc_dir, cfg->n_angles);
}

int nerf_ctx_create(const nerf_config* cfg, nerf_ctx** out) {
    if (!out) return fail("out is NULL");
    *out = nullptr;
    if (int r = check_cfg(cfg)) return r;
    RenderKernel k;
    if (pick_render_kernel(*cfg, cfg->precision, false, &k)) return 1;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail("no HIP device available (%s): libnerf_mi355 has no CPU path", hipGetErrorString(e));
    if (cfg->device < 0 || cfg->device >= ndev) return fail("device %d out of range (%d devices)", cfg->device, ndev);
    HIP_OK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIP_OK(hipGetDeviceProperties(&prop, cfg->device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail("device %d is %s; this library is built for gfx950 (MI355X) only", cfg->device, prop.gcnArchName);
    nerf_ctx* c = new nerf_ctx();
    c->cfg = *cfg;
    c->num_cus = prop.multiProcessorCount;
    if (hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return fail("hipStreamCreate failed");
    }
    c->stream = c->own_stream;
    if (hipMalloc((void**)&c->nonfinite, sizeof(unsigned long long)) != hipSuccess ||
        hipMemset(c->nonfinite, 0, sizeof(unsigned long long)) != hipSuccess) {
        delete c;
        return fail("hipMalloc of the status counter failed");
    }
    mlp_fp32_set_attributes();
    mlp_f16x3_set_attributes();
    wide::mlp_f16x3_set_attributes();
    bf16::mlp_bf16x3_set_attributes();
    bf16::wide::mlp_bf16x3_set_attributes();
    mlp_bwd_f16x3_set_attributes();
    mlp_f16_2t_set_attributes();
    *out = c;
    return 0;
}

void nerf_ctx_destroy(nerf_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    (void)hipStreamSynchronize(c->stream);
    DevBuf* bufs[] = {&c->b_orig, &c->b_dirs, &c->b_zc, &c->b_zf, &c->b_raw, &c->b_wc, &c->b_u0, &c->b_u1,
                      &c->b_in0, &c->b_in1, &c->b_in2, &c->b_grid[0], &c->b_grid[1], &c->b_gbounds, &c->b_gstate,
                      &c->b_mesh_v, &c->b_mesh_n, &c->b_mesh_t, &c->b_mesh_sigma, &c->b_mesh_mask, &c->b_mesh_first,
                      &c->b_mesh_count, &c->b_mesh_tfirst, &c->b_mesh_sums, &c->b_lattice, &c->b_sh_table, &c->cull.mask, &c->cull.first,
                      &c->b_csums, &c->b_cxyz, &c->b_cdirs, &c->b_craw};
    for (DevBuf* b : bufs) if (b->p) (void)hipFree(b->p);
    for (auto& b : c->b_out) if (b.p) (void)hipFree(b.p);
    for (auto& n : c->net) {
        for (void* p : n.stream) if (p) (void)hipFree(p);
        for (float* p : n.cst) if (p) (void)hipFree(p);
        if (n.dev_blob) (void)hipFree(n.dev_blob);
    }
    for (int32_t* p : c->rt) if (p) (void)hipFree(p);
    for (int32_t* p : c->rt_cst) if (p) (void)hipFree(p);
    if (c->win_scale) (void)hipFree(c->win_scale);
    for (auto& ev : c->ev_pool) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    if (c->copy_stream) { (void)hipStreamSynchronize(c->copy_stream); (void)hipStreamDestroy(c->copy_stream); }
    for (hipEvent_t e : c->copy_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->cull_ev) (void)hipEventDestroy(e);
    if (c->cull_rows) (void)hipHostFree(c->cull_rows);
    for (RgbSkipGate& g : c->skip_gate) {
        if (g.pending) (void)hipEventSynchronize(g.ev);
        if (g.ev) (void)hipEventDestroy(g.ev);
        if (g.host) (void)hipHostFree(g.host);
        if (g.dev) (void)hipFree(g.dev);
    }
    comm_free(c);
    train_free(c);
    if (c->nonfinite) (void)hipFree(c->nonfinite);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

// Debug entry (not part of include/nerf_mi355.h): the rgb-skipping kernel's counters of network `which` after the ctx stream has
// drained -- out[0] the 128-row tiles it ran, out[1] those it skipped, both cumulative -- and out[2], the launches the gate
// still sends to the full kernel.  What tests/test_gpu_rgb_skip.py reads to see which kernel a render ran.
extern "C" int nerf_debug_rgb_skip_counts(nerf_ctx* c, int which, unsigned long long* out) {
    ENTER(c);
    if ((which != 0 && which != 1) || !out) return fail("nerf_debug_rgb_skip_counts: bad argument");
    const RgbSkipGate& g = c->skip_gate[which];
    out[0] = out[1] = 0;
    out[2] = (unsigned long long)g.full_left;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (g.dev) HIP_OK(hipMemcpy(out, g.dev, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return 0;
}

int nerf_ctx_synchronize(nerf_ctx* c) {
    if (!c) return fail("ctx is NULL");
    HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int nerf_ctx_set_stream(nerf_ctx* c, void* s) {
    if (!c) return fail("ctx is NULL");
    HIP_OK(hipStreamSynchronize(c->stream));
    c->stream = (s == NERF_STREAM_OWN) ? c->own_stream : (hipStream_t)s;
    return 0;
}

int nerf_ctx_set_bounds(nerf_ctx* c, float near_b, float far_b) {
    if (!c) return fail("ctx is NULL");
    c->cfg.near_boundary = near_b; c->cfg.far_boundary = far_b;
    return 0;
}

int nerf_ctx_set_sampling(nerf_ctx* c, int mode) {
    if (!c) return fail("ctx is NULL");
    if (mode != NERF_SAMPLING_LINEAR && mode != NERF_SAMPLING_LINDISP)
        return fail("unknown sampling mode %d (NERF_SAMPLING_LINEAR = 0, NERF_SAMPLING_LINDISP = 1)", mode);
    if (mode == NERF_SAMPLING_LINDISP && !(c->cfg.near_boundary > 0.f)) return fail("lindisp needs near_boundary > 0");
    c->sampling = mode;
    return 0;
}

int nerf_ctx_set_ray_space(nerf_ctx* c, int space, float ndc_near_plane) {
    if (!c) return fail("ctx is NULL");
    if (space != NERF_RAYS_WORLD && space != NERF_RAYS_NDC)
        return fail("unknown ray space %d (NERF_RAYS_WORLD = 0, NERF_RAYS_NDC = 1)", space);
    if (space == NERF_RAYS_NDC && !(ndc_near_plane > 0.f)) return fail("ndc_near_plane must be > 0 (got %g)", ndc_near_plane);
    c->ray_space = space;
    if (space == NERF_RAYS_NDC) c->ndc_near_plane = ndc_near_plane;
    return 0;
}

int nerf_ctx_set_scene_box(nerf_ctx* c, const float* lo3, const float* hi3) {
    if (!c) return fail("ctx is NULL");
    if (!lo3 && !hi3) { c->box_on = false; c->grid_R = 0; return 0; }   // the grid lives on the box: it goes with it
    if (!lo3 || !hi3) return fail("scene box: lo and hi are both given, or both NULL (box off)");
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo3[a]) || !std::isfinite(hi3[a]) || !(lo3[a] < hi3[a]))
            return fail("scene box needs finite lo < hi on every axis (axis %d: lo %g, hi %g)", a, lo3[a], hi3[a]);
    for (int a = 0; a < 3; ++a) { c->box.lo[a] = lo3[a]; c->box.hi[a] = hi3[a]; }
    c->box_on = true;
    c->grid_R = 0;
    return 0;
}

int nerf_ctx_set_precision(nerf_ctx* c, int precision) {
    if (!c) return fail("ctx is NULL");
    RenderKernel k;
    if (pick_render_kernel(c->cfg, precision, false, &k)) return 1;
    HIP_OK(hipStreamSynchronize(c->stream));
    c->cfg.precision = precision;
    return 0;
}

int nerf_load_weights(nerf_ctx* c, int which, const float* blob, size_t n_floats) {
    if (!c || !blob) return fail("ctx/blob is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail("which must be 0 (coarse) or 1 (fine)");
    const size_t want = nerf_blob_size(&c->cfg);
    if (n_floats != want) return fail("weight blob has %zu floats, expected %zu", n_floats, want);
    HIP_OK(hipSetDevice(c->cfg.device));
    // The blob goes to the device and every stream is re-packed from it there, all enqueued on the ctx stream: work already on
    // that stream still reads the old weights, work enqueued later the new ones.  No other stream reads a render stream (the
    // copy stream moves finished outputs, the trainer's side stream works on the trainer's own buffers), so nothing waits.
    // host_blob is pageable: a copy from it has left the host when hipMemcpyAsync returns, and the next load may overwrite it.
    NetWeights& n = c->net[which];
    n.host_blob.assign(blob, blob + want);
    if (!n.dev_blob) HIP_OK(hipMalloc((void**)&n.dev_blob, want * sizeof(float)));
    HIP_OK(hipMemcpyAsync(n.dev_blob, n.host_blob.data(), want * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int r = repack_render_streams(c, which, n.dev_blob)) return r;
    n.loaded = true;
    return train_on_load(c, which);      // a running trainer restarts from the new weights
}

// ---- encoding window ----
// The window is a scale table over the blob (weight_tables.hip::build_scale_table) that every re-pack multiplies by and every
// gradient reduction scales its contribution with; no MLP kernel knows of it.  Setting it uploads the table and re-packs
// whatever exists, all on the ctx stream: work already enqueued reads the old streams, work enqueued later the new ones.
int nerf_ctx_set_encoding_window(nerf_ctx* c, const float* w_xyz, const float* w_dir) {
    ENTER(c);
    const int lx = c->cfg.n_pos_enc_xyz, ld = c->cfg.n_pos_enc_dir;
    auto check = [](const char* name, const float* w, int n) -> int {
        for (int k = 0; w && k < n; ++k)
            if (!std::isfinite(w[k]) || w[k] < 0.f || w[k] > 1.f)
                return fail("encoding window: every weight is finite and in [0, 1] (%s[%d] = %g)", name, k, w[k]);
        return 0;
    };
    if (int r = check("w_xyz", w_xyz, lx)) return r;
    if (int r = check("w_dir", w_dir, ld)) return r;
    if (c->cfg.n_angles == 0) w_dir = nullptr;      // the xyz-only network has no direction encoding: accepted, no effect
    bool on = false;
    for (int k = 0; w_xyz && k < lx; ++k) on |= w_xyz[k] != 1.f;
    for (int k = 0; w_dir && k < ld; ++k) on |= w_dir[k] != 1.f;
    if (!on && !c->win_on) return 0;                // off stays off: nothing to launch
    if (int r = train_window_guard(c)) return r;
    for (int k = 0; k < 10; ++k) c->win_xyz[k] = on && w_xyz && k < lx ? w_xyz[k] : 1.f;
    for (int k = 0; k < 4; ++k) c->win_dir[k] = on && w_dir && k < ld ? w_dir[k] : 1.f;
    if (on) {
        build_scale_table(lx, ld, c->cfg.n_angles, c->win_xyz, c->win_dir, c->win_host);
        const size_t bytes = c->win_host.size() * sizeof(float);
        if (!c->win_scale) HIP_OK(hipMalloc((void**)&c->win_scale, bytes));
        // (win_host is pageable: the copy has left the host when hipMemcpyAsync returns, as nerf_load_weights relies on)
        HIP_OK(hipMemcpyAsync(c->win_scale, c->win_host.data(), bytes, hipMemcpyHostToDevice, c->stream));
    }
    c->win_on = on;
    // the render streams: from the trainer's master blob where one trains the network (train_flush_weights re-packs after
    // optimizer steps and keeps its own books), else from the loaded blob
    for (int w = 0; w < 2; ++w) {
        if (!c->net[w].loaded) continue;
        const float* src = train_master_blob(c, w);
        if (int r = repack_render_streams(c, w, src ? src : c->net[w].dev_blob)) return r;
    }
    return train_on_window(c);
}

int nerf_ctx_get_encoding_window(nerf_ctx* c, float* w_xyz, float* w_dir, int32_t* active) {
    if (!c) return fail("ctx is NULL");
    for (int k = 0; w_xyz && k < c->cfg.n_pos_enc_xyz; ++k) w_xyz[k] = c->win_xyz[k];
    for (int k = 0; w_dir && k < c->cfg.n_pos_enc_dir; ++k) w_dir[k] = c->win_dir[k];
    if (active) *active = c->win_on ? 1 : 0;
    return 0;
}

int nerf_get_rays_directions(nerf_ctx* c, const float* c2w, float fov, int32_t H, int32_t W, float* dirs, int mem) {
    ENTER(c);
    if (!c || !c2w || !dirs) return fail("NULL argument");
    if (H <= 0 || W <= 0) return fail("bad image size %dx%d", H, W);
    const long long N = (long long)H * W;
    Staging st(c, mem);
    float* d = st.out(c->b_dirs, dirs, N * 16);
    if (st.err) return st.err;
    launch_raygen(c2w, fov, H, W, 0, N, nullptr, d, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_rays_to_ndc(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, int64_t N, float fov, float ndc_near_plane,
                     float* out_orig, float* out_dirs, int mem) {
    ENTER(c);
    if (!rays_orig || !rays_dirs || !out_orig || !out_dirs) return fail("NULL argument");
    if (N < 0) return fail("bad shape N=%lld", (long long)N);
    if (!(ndc_near_plane > 0.f)) return fail("ndc_near_plane must be > 0 (got %g)", ndc_near_plane);
    if ((out_orig == rays_orig) != (out_dirs == rays_dirs) || out_orig == rays_dirs || out_dirs == rays_orig || out_orig == out_dirs)
        return fail("nerf_rays_to_ndc works in place only as out_orig == rays_orig AND out_dirs == rays_dirs");
    if (N == 0) return 0;
    Staging st(c, mem);
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    float* oo = st.out(c->b_orig, out_orig, (size_t)N * 16);      // (a host caller's rays are converted in their staging buffers)
    float* od = st.out(c->b_dirs, out_dirs, (size_t)N * 16);
    if (st.err) return st.err;
    launch_rays_to_ndc(o, d, N, fov, ndc_near_plane, oo, od, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_get_z_values(nerf_ctx* c, int64_t N, int32_t S, const float* u, uint64_t seed, int64_t ray_base, float* z,
                      int mem) {
    ENTER(c);
    if (!c || !z) return fail("NULL argument");
    if (N < 0 || S <= 0) return fail("bad shape N=%lld S=%d", (long long)N, S);
    if (int r = sampling_ok(c)) return r;
    Staging st(c, mem);
    const float* du = st.in(c->b_u0, u, (size_t)N * S * 4);
    float* dz = st.out(c->b_zc, z, (size_t)N * S * 4);
    if (st.err) return st.err;
    launch_z_values(c->cfg.near_boundary, c->cfg.far_boundary, c->sampling == NERF_SAMPLING_LINDISP, N, S, du, seed, ray_base,
                    dz, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_get_z_values_rays(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, int64_t N, int32_t S, const float* u,
                           uint64_t seed, int64_t ray_base, float* z, int mem) {
    ENTER(c);
    if (!rays_orig || !rays_dirs || !z) return fail("NULL argument");
    if (N < 0 || S <= 0) return fail("bad shape N=%lld S=%d", (long long)N, S);
    if (int r = sampling_ok(c)) return r;
    Staging st(c, mem);
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    const float* du = st.in(c->b_u0, u, (size_t)N * S * 4);
    float* dz = st.out(c->b_zc, z, (size_t)N * S * 4);
    if (st.err) return st.err;
    if (int r = draw_z_values(c, o, d, N, S, du, seed, ray_base, dz)) return r;
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_ray_box_bounds(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, int64_t N, float* bounds, int32_t* narrowed,
                        int mem) {
    ENTER(c);
    if (!rays_orig || !rays_dirs || !bounds) return fail("NULL argument");
    if (N < 0) return fail("bad shape N=%lld", (long long)N);
    if (!c->box_on) return fail("no scene box is set (nerf_ctx_set_scene_box)");
    Staging st(c, mem);
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    float* db = st.out(c->b_in0, bounds, (size_t)N * 8);
    int32_t* dn = st.out(c->b_in1, narrowed, (size_t)N * 4);
    if (st.err) return st.err;
    launch_ray_box_bounds(c->box, c->cfg.near_boundary, c->cfg.far_boundary, o, d, N, db, dn, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_ray_occupancy_bounds(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, int64_t N, float* bounds,
                              int32_t* state, int mem) {
    ENTER(c);
    if (!rays_orig || !rays_dirs || !bounds) return fail("NULL argument");
    if (N < 0) return fail("bad shape N=%lld", (long long)N);
    if (!c->box_on || c->grid_R == 0) return fail("no occupancy grid is set (nerf_ctx_set_occupancy_grid, nerf_occupancy_bake)");
    Staging st(c, mem);
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    float* db = st.out(c->b_in0, bounds, (size_t)N * 8);
    int32_t* ds = st.out(c->b_in1, state, (size_t)N * 4);
    if (st.err) return st.err;
    launch_ray_grid_bounds(c->box, c->cfg.near_boundary, c->cfg.far_boundary, (const uint32_t*)c->b_grid[c->grid_cur].p, c->grid_R,
                           o, d, N, db, ds, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

// ---- sample culling (cull_kernels.hip) ----
int nerf_ctx_set_sample_culling(nerf_ctx* c, int on) {
    if (!c) return fail("ctx is NULL");
    c->cull_on = on != 0;
    return 0;
}

int nerf_ctx_set_train_sample_culling(nerf_ctx* c, int on) {      // the trainer's switch: train_api.hip (forward_pass)
    if (!c) return fail("ctx is NULL");
    c->train_cull_on = on != 0;
    return 0;
}

int nerf_sample_occupancy(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, const float* z, int64_t N, int32_t S,
                          int32_t* keep, int mem) {
    ENTER(c);
    if (!rays_orig || !rays_dirs || !z || !keep) return fail("NULL argument");
    if (N < 0 || S <= 0) return fail("bad shape N=%lld S=%d", (long long)N, S);
    if (!c->box_on || c->grid_R == 0) return fail("no occupancy grid is set (nerf_ctx_set_occupancy_grid, nerf_occupancy_bake)");
    if (N == 0) return 0;
    Staging st(c, mem);
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    const float* dz = st.in(c->b_zc, z, (size_t)N * S * 4);
    int32_t* dk = st.out(c->b_in0, keep, (size_t)N * S * 4);
    if (st.err) return st.err;
    launch_sample_keep(c->box, (const uint32_t*)c->b_grid[c->grid_cur].p, c->grid_R, o, d, dz, N, S, nullptr, dk, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_ctx_read_culling(nerf_ctx* c, int64_t* samples, int64_t* kept) {
    if (!c) return fail("ctx is NULL");
    if (samples) *samples = c->cull_samples;
    if (kept) *kept = c->cull_kept;
    c->cull_samples = c->cull_kept = 0;
    return 0;
}

int nerf_ctx_read_culling_timing(nerf_ctx* c, double* ms4, int64_t* n_passes) {
    if (!c) return fail("ctx is NULL");
    HIP_OK(hipStreamSynchronize(c->stream));
    double tot[4] = {0, 0, 0, 0};
    const size_t passes = c->cull_ev_used / 6;
    for (size_t p = 0; p < passes; ++p) {
        const hipEvent_t* e = &c->cull_ev[6 * p];
        const int pair[4][2] = {{0, 1}, {1, 2}, {2, 3}, {4, 5}};
        for (int i = 0; i < 4; ++i) {
            float ms = 0;
            HIP_OK(hipEventElapsedTime(&ms, e[pair[i][0]], e[pair[i][1]]));
            tot[i] += ms;
        }
    }
    if (ms4) for (int i = 0; i < 4; ++i) ms4[i] = tot[i];
    if (n_passes) *n_passes = (int64_t)passes;
    c->cull_ev_used = 0;
    return 0;
}

int nerf_sample_pdf(nerf_ctx* c, const float* weights, const float* z, int64_t N, int32_t S, int32_t Sf,
                    const float* u, uint64_t seed, int64_t ray_base, float* z_new, float* z_merged, int mem) {
    ENTER(c);
    if (!c || !weights || !z) return fail("NULL argument");
    if (N < 0 || S < 2 || Sf <= 0) return fail("bad shape N=%lld S=%d Sf=%d (need S>=2, Sf>=1)", (long long)N, S, Sf);
    if (sample_pdf_lds_bytes(S, Sf) > 64 * 1024) return fail("S=%d Sf=%d exceeds the sampler's LDS budget", S, Sf);
    Staging st(c, mem);
    const float* dw = st.in(c->b_in0, weights, (size_t)N * S * 4);
    const float* dz = st.in(c->b_in1, z, (size_t)N * S * 4);
    const float* du = st.in(c->b_u1, u, (size_t)N * Sf * 4);
    float* dn = st.out(c->b_in2, z_new, (size_t)N * Sf * 4);
    float* dm = st.out(c->b_zf, z_merged, (size_t)N * (S + Sf) * 4);
    if (st.err) return st.err;
    launch_sample_pdf(dw, dz, N, S, Sf, du, seed, ray_base, dn, dm, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_positional_encoding(nerf_ctx* c, const float* x, int64_t M, int32_t n_enc, int32_t passthrough, float* out,
                             int mem) {
    ENTER(c);
    if (!c || !x || !out) return fail("NULL argument");
    if (M < 0 || n_enc < 0 || n_enc > 16) return fail("bad shape M=%lld n_enc=%d", (long long)M, n_enc);
    const size_t per = 3 * ((passthrough ? 1 : 0) + 2 * (size_t)n_enc);
    Staging st(c, mem);
    const float* dx = st.in(c->b_in0, x, (size_t)M * 12);
    float* dout = st.out(c->b_in1, out, (size_t)M * per * 4);
    if (st.err) return st.err;
    launch_posenc(dx, M, n_enc, passthrough, dout, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_model_predict(nerf_ctx* c, int which, const float* xyz, const float* view_dirs, int64_t M, float* raw,
                       int mem) {
    ENTER(c);
    // view_dirs may be NULL for the xyz-only network (model_predict(..., view_dirs=None), UtilsNRF.py:229-234)
    if (!c || !xyz || !raw || (!view_dirs && c->cfg.n_angles != 0)) return fail("NULL argument");
    if (which != 0 && which != 1) return fail("which must be 0 (coarse) or 1 (fine)");
    if (M < 0) return fail("bad M");
    Staging st(c, mem);
    const float* dx = st.in(c->b_in0, xyz, (size_t)M * 12);
    const float* dv = st.in(c->b_in1, view_dirs, (size_t)M * 12);
    float* dr = st.out(c->b_raw, raw, (size_t)M * 16);
    if (st.err) return st.err;
    if (int r = eval_points(c, which, dx, dv, M, dr)) return r;
    return st.finish();
}

int nerf_ray_marching(nerf_ctx* c, const float* raw, const float* z, int64_t N, int32_t S, const nerf_outputs* outs,
                      int mem) {
    ENTER(c);
    if (!c || !raw || !z || !outs) return fail("NULL argument");
    if (N < 0 || S <= 0) return fail("bad shape");
    Staging st(c, mem);
    const float* dr = st.in(c->b_raw, raw, (size_t)N * S * 16);
    const float* dz = st.in(c->b_zc, z, (size_t)N * S * 4);
    const nerf_outputs dev = stage_outputs(c, st, *outs, N, S);
    if (st.err) return st.err;
    launch_composite(dr, dz, N, S, dev.rgb, dev.weights, dev.cumprod, dev.alpha, dev.rgb_samples, dev.depth, c->stream);
    if (dev.z && dev.z != dz) HIP_OK(hipMemcpyAsync(dev.z, dz, (size_t)N * S * 4, hipMemcpyDeviceToDevice, c->stream));
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_render_rays(nerf_ctx* c, int which, const float* o, const float* d, const float* z, int64_t N, int32_t S,
                     const nerf_outputs* outs, int mem) {
    ENTER(c);
    if (!c || !o || !d || !z || !outs) return fail("NULL argument");
    if (which != 0 && which != 1) return fail("which must be 0 (coarse) or 1 (fine)");
    if (N < 0 || S <= 0) return fail("bad shape");
    Staging st(c, mem);
    const float* so = st.in(c->b_orig, o, (size_t)N * 16);
    const float* sd = st.in(c->b_dirs, d, (size_t)N * 16);
    const float* sz = st.in(c->b_zc, z, (size_t)N * S * 4);
    const nerf_outputs dev = stage_outputs(c, st, *outs, N, S);
    if (st.err) return st.err;
    if (int r = dev_render_rays(c, which, so, sd, sz, N, S, dev)) return r;
    return st.finish();
}

int nerf_render(nerf_ctx* c, const float* o, const float* d, int64_t N, int32_t Sc, int32_t Sf, const float* u_c,
                const float* u_f, uint64_t seed, int64_t ray_base, const nerf_outputs* outs, int mem) {
    ENTER(c);
    if (!c || !o || !d || !outs) return fail("NULL argument");
    if (N < 0 || Sc <= 0 || Sf < 0) return fail("bad shape N=%lld Sc=%d Sf=%d", (long long)N, Sc, Sf);
    const bool fine = Sf > 0 && c->net[NERF_NET_FINE].loaded;
    const int S = fine ? Sc + Sf : Sc;
    if (fine && sample_pdf_lds_bytes(Sc, Sf) > 64 * 1024) return fail("Sc=%d Sf=%d exceeds the sampler's LDS budget", Sc, Sf);
    Staging st(c, mem);
    const float* so = st.in(c->b_orig, o, (size_t)N * 16);
    const float* sd = st.in(c->b_dirs, d, (size_t)N * 16);
    const float* duc = st.in(c->b_u0, u_c, (size_t)N * Sc * 4);
    const float* duf = st.in(c->b_u1, fine ? u_f : nullptr, (size_t)N * Sf * 4);      // (without a fine pass nothing reads u_f)
    const nerf_outputs dev = stage_outputs(c, st, *outs, N, S);
    if (st.err) return st.err;
    if (int r = dev_render(c, so, sd, N, Sc, Sf, duc, duf, seed, ray_base, dev)) return r;
    return st.finish();
}

int nerf_render_image(nerf_ctx* c, const float* c2w, float fov, int32_t H, int32_t W, int64_t ray_begin,
                      int64_t ray_count, int64_t batch, int32_t Sc, int32_t Sf, const float* u_c, const float* u_f,
                      uint64_t seed, const nerf_outputs* outs, int mem) {
    ENTER(c);
    if (!c || !c2w || !outs) return fail("NULL argument");
    if (H <= 0 || W <= 0 || Sc <= 0 || Sf < 0) return fail("bad shape");
    const long long total = (long long)H * W;
    if (ray_count <= 0) { ray_begin = 0; ray_count = total; }
    if (ray_begin < 0 || ray_begin + ray_count > total) return fail("ray slab [%lld,+%lld) outside %lld rays",
                                                                    (long long)ray_begin, (long long)ray_count, total);
    if (batch < 0) return fail("batch_size must be > 0");   // assert of src/UtilsNRF.py:25
    const bool fine = Sf > 0 && c->net[NERF_NET_FINE].loaded;
    const int S = fine ? Sc + Sf : Sc;
    if (fine && sample_pdf_lds_bytes(Sc, Sf) > 64 * 1024) return fail("Sc=%d Sf=%d exceeds the sampler's LDS budget", Sc, Sf);
    const long long N = ray_count;
    if (int r = sampling_ok(c)) return r;
    if (batch == 0) {
        batch = 1 << 18;
        // host destinations with per-sample outputs (up to 5.4 KB per ray): four batches per slab so that the device-to-host
        // copies of one batch run under the next batch's kernels (results do not depend on the batch)
        const bool per_sample = outs->weights || outs->cumprod || outs->alpha || outs->rgb_samples || outs->z;
        if (mem == NERF_MEM_HOST && per_sample && N >= 32768) batch = ((N + 3) / 4 + 127) / 128 * 128;
    }
    // rays of the slab (origins are the broadcast translation column, src/NeRF.py:209)
    if (int r = ensure(c, c->b_orig, (size_t)N * 16)) return r;
    if (int r = ensure(c, c->b_dirs, (size_t)N * 16)) return r;
    launch_raygen(c2w, fov, H, W, ray_begin, N, (float*)c->b_orig.p, (float*)c->b_dirs.p, c->stream);
    if (c->ray_space == NERF_RAYS_NDC)   // in place: what nerf_rays_to_ndc makes of these rays, bit for bit
        launch_rays_to_ndc((const float*)c->b_orig.p, (const float*)c->b_dirs.p, N, fov, c->ndc_near_plane, (float*)c->b_orig.p,
                           (float*)c->b_dirs.p, c->stream);
    const float *duc = u_c, *duf = u_f;
    nerf_outputs dev = *outs;
    if (mem == NERF_MEM_HOST) {
        if (u_c) { if (int r = h2d(c, c->b_u0, u_c + ray_begin * Sc, (size_t)N * Sc * 4)) return r; duc = (const float*)c->b_u0.p; }
        if (u_f && fine) { if (int r = h2d(c, c->b_u1, u_f + ray_begin * Sf, (size_t)N * Sf * 4)) return r; duf = (const float*)c->b_u1.p; }
        Staging st(c, mem);      // never finished: the outputs leave batch by batch on the copy stream (copy_back_batch)
        dev = stage_outputs(c, st, *outs, N, S);
        if (st.err) return st.err;
    } else {
        if (u_c) duc = u_c + ray_begin * Sc;
        if (u_f) duf = u_f + ray_begin * Sf;
    }
    const OutSizes sz = out_sizes(S);
    size_t k = 0;
    for (long long off = 0; off < N; off += batch, ++k) {
        const long long n = std::min<long long>(batch, N - off);
        nerf_outputs part = dev;
        for (int i = 0; i < 7; ++i) {
            float** p = out_ptrs(part, i);
            if (*p) *p += sz.per_ray[i] * off;
        }
        if (int r = dev_render(c, (const float*)c->b_orig.p + off * 4, (const float*)c->b_dirs.p + off * 4, n, Sc, Sf,
                               duc ? duc + off * Sc : nullptr, (duf && fine) ? duf + off * Sf : nullptr, seed,
                               ray_begin + off, part)) {
            if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
            return r;
        }
        if (mem == NERF_MEM_HOST)
            if (int r = copy_back_batch(c, outs, &dev, off, n, S, k)) { (void)hipStreamSynchronize(c->copy_stream); return r; }
    }
    // the last copy waits for the last batch: an idle copy stream means the whole call is done
    if (mem == NERF_MEM_HOST && c->copy_stream) HIP_OK(hipStreamSynchronize(c->copy_stream));
    return 0;
}

// Page-locked host memory: destinations the device writes by DMA at link speed, beside running kernels.
int nerf_host_alloc(size_t bytes, void** out) {
    if (!out) return fail("out is NULL");
    *out = nullptr;
    if (bytes == 0) return fail("nerf_host_alloc of 0 bytes");
    HIP_OK(hipHostMalloc(out, bytes, hipHostMallocPortable));
    return 0;
}

int nerf_host_free(void* p) {
    if (!p) return 0;
    HIP_OK(hipHostFree(p));
    return 0;
}

int nerf_ctx_read_nonfinite(nerf_ctx* c, int64_t* rows) {
    if (!c || !rows) return fail("NULL argument");
    ENTER(c);
    HIP_OK(hipStreamSynchronize(c->stream));
    unsigned long long v = 0;
    HIP_OK(hipMemcpy(&v, c->nonfinite, sizeof v, hipMemcpyDeviceToHost));
    HIP_OK(hipMemset(c->nonfinite, 0, sizeof v));
    *rows = (int64_t)v;
    return 0;
}

int nerf_ctx_enable_timing(nerf_ctx* c, int on) {
    if (!c) return fail("ctx is NULL");
    HIP_OK(hipStreamSynchronize(c->stream));
    c->timing = on != 0;
    c->ev_used = 0;
    c->cull_ev_used = 0;
    c->timed_rows = 0;
    return 0;
}

int nerf_ctx_read_timing(nerf_ctx* c, double* mlp_ms, int64_t* n_launches, int64_t* n_rows) {
    if (!c) return fail("ctx is NULL");
    HIP_OK(hipStreamSynchronize(c->stream));
    double tot = 0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second));
        tot += ms;
    }
    if (mlp_ms) *mlp_ms = tot;
    if (n_launches) *n_launches = (int64_t)c->ev_used;
    if (n_rows) *n_rows = c->timed_rows;
    c->ev_used = 0;
    c->timed_rows = 0;
    c->cull_ev_used = 0;      // the culled passes' stage events belong to the same span: nerf_ctx_read_culling_timing comes first
    return 0;
}

}  // extern "C"
