// train_api.hip -- C ABI of the training path (include/nerf_mi355.h, "training" section):
//   NeRF.train_step            src/NeRF.py:136-178   (loss, gradients of both networks, optimizer step, metrics)
//   Adam(optimizer_lr)         src/ExecutionRun.py:226 (Keras-2.7 defaults beta_1=.9 beta_2=.999 epsilon=1e-7)
// Orchestration only: every arithmetic step is a HIP kernel of train_kernels.hip / aux_kernels.hip / the fused MLP
// kernels on the context's stream.  Master weights, gradients and Adam moments live on the device as flat blobs in Keras
// get_weights() order; what the kernels read (the fused trainer's two operand streams, the reference trainer's padded
// [K x N] / [N x K] matrices) is rebuilt from the blob after every update.
// Two trainers (TrainState::reference): the fused one (default; stash forward, mlp_bwd_f16x3, batched weight gradients
// on fragment-major buffers) and the layer-wise exact-fp32 one (NERF_TRAIN_FORWARD=gemm), kept as an independent reference.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "nerf_ctx.h"
#include "train_kernels.h"

using namespace nerf;

namespace nerf {

struct TLayer {
    int K_real, N_real, Kp, Np, rowmap;
    size_t w_off, b_off;           // offsets into the blob
    float *W, *WT, *bias;          // padded copies (device; the reference trainer's, TNet::mats)
};

struct TNet {
    bool present = false;
    bool render_dirty = false;     // optimizer steps not yet packed into the render path's operand streams
    bool host_stale = false;       // ... and not yet copied to NetWeights::host_blob (the seed of the next trainer)
    float *blob = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr;
    float* mats = nullptr;         // reference trainer: W, WT and bias of every layer (TLayer)
    void* fstream = nullptr;       // fused forward (f16x3 stash kernel): operand stream + constants, re-packed on device
    float* fcst = nullptr;
    void* bstream = nullptr;       // fused backward (mlp_bwd_f16x3): transposed operand stream, re-packed on device
    bool bdx = false;              // ... built with the encoding tiles (the fine network under sampler_gradient; both under ray_grads)
    int n_layers = 11;             // 11: xyz + view-direction network; 12: xyz-only network (n_angles_for_model = 0)
    TLayer L[12];
};

struct TPass {                      // activations of one pass, kept from forward to backward
    DevBuf C4, C8, H1, H2, H3, H5, H6, H7, H8b, H9, raw, T, w, rgb, z;   // H8b: xyz-only network's extra layer
    // fused backward: LeakyReLU' bit records of layers 0..8 (32 B per row and layer, written by the stash forward),
    // the pre-activation gradients D[0..7] (Mp x 256) and G9 = D[8] (Mp x 128), the two encoding-gradient parts
    DevBuf masks, D[10], dxa, dxb;     // D[8], D[9]: see MlpBwdArgs::d_ptr (the xyz-only network has ten gradient buffers)
    DevBuf rs;                         // pair16 gradient buffers (fused trainer, float32 policy): 10 x Mp row factors (MlpBwdArgs::rs_ptr)
    // The record of a pass run under nerf_ctx_set_train_sample_culling (stash side: it travels with a RenderSlot, so a slot's
    // backward pass does not depend on what the ctx culled, or was told, after its forward pass)
    SampleCompaction cull;
};

// nerf_train_render_forward / _backward (ABI 5): the activations of one ray batch of NeRF.render(), kept from a forward to
// its backward while other batches run -- a whole source image of DietNeRF's consistency loss stays resident (150 x 150 rays x
// (55 + 110) rows: 38 GB under the float32 policy, 19 GB under mixed_float16 of this device's 288 GB) instead of being
// rendered once for the embedding network and a second time under the tape.  A slot owns the STASH side of two passes, its
// own copies of the rays and draws, and the new depths; the gradient side of a TPass (D, dxa, dxb, rs) is lent by
// TrainState::pass while the slot runs.
struct RenderSlot {
    TPass pass[2];
    DevBuf o, d, u_c, u_f, z_new;
    long long N = 0, ray_base = 0;
    int Sc = 0, Sf = 0;
    unsigned long long seed = 0;
    bool has_uc = false, has_uf = false, valid = false;
};
constexpr int kMaxRenderSlots = 4096;

struct TrainState {
    nerf_train_config cfg;
    // The layer-wise exact-fp32 trainer (NERF_TRAIN_FORWARD=gemm): gemm_abt forward and data gradients, gemm_atb weight
    // gradients, row-major fp32 buffers -- an independent reference for the tests.  Otherwise (default) the fused trainer:
    // the f16x3 stash forward, the mlp_bwd_f16x3 chain and the batched weight-gradient GEMMs on the fp16 matrix cores, all
    // on fragment-major buffers (frag_layout.h::frag_index) that hold fp32 activations and "pair16" gradients (fp16 (hi, lo)
    // pairs in the fp32 slots, MlpBwdArgs::rs_ptr) under the float32 policy, fp16 values under mixed_float16.
    bool reference = false;
    // device gather tables of the backward stream: [0] plain, [1] with encoding tiles (the stash forward's stream and
    // constants are re-packed through the ctx's tables of the render stream of the same kind: nerf_ctx::rt)
    int32_t* bidx[2] = {nullptr, nullptr};
    long long step = 0;
    size_t nblob = 0;
    TNet net[2];
    TPass pass[2];
    DevBuf Graw, partial, d_rgb, d_wext, d_zf, tgt, o, d, u_c, u_f, scal;
    DevBuf Ga, Gb, G9, dA0;         // reference trainer: ping-pong gradient buffers (Mp x 256), the rgb branch's (Mp x 128), dL/d(xyz_enc)
    DevBuf Gc;                      // a culled pass: the kept rows of Graw (padded rows x 4, padding rows zero)
    DevBuf gmax;                    // fused trainer: 2 passes x 16 x 64 max|D| slots (MlpBwdArgs::gmax -> GemmAtb::gmax)
    DevBuf dsig;                    // ... (Mp) column 3 of Graw as a vector, written by the backward chain (GemmAtb::sig_g)
    // The fine pass's batched weight-gradient launch on a second stream, beside the sampler / compositing backward and the coarse
    // pass's backward chain (default; NERF_TRAIN_OVERLAP=0 keeps one stream).  Its slab sums live in their own buffer, each pass
    // has its own max|D| slots, and the main stream joins before anything reads the fine network's gradient blob.  Both big
    // kernels want a whole CU per workgroup, so this is tail filling, not co-residency: -1.2 % on a mixed_float16 step, +-0
    // under the float32 policy; bit-identical results (tests/test_gpu_train.py::test_side_stream_...).
    bool overlap = false;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool side_pending = false;
    DevBuf partial_side;
    bool acc_grads = false;         // the running backward pass ADDS to the gradient blobs (nerf_train_render_gradients)
    // ray loss = loss_w[0] * MSE(coarse) + loss_w[1] * MSE(fine) (nerf_train_set_loss_weights): 1, 1 is NeRF.train_step
    // (src/NeRF.py:151,157); DietNeRF's ray loss counts the coarse term twice (src/DietNeRF.py:160-170)
    float loss_w[2] = {1.f, 1.f};
    // ... + dist_w[0] * L(coarse weights) + dist_w[1] * L(fine weights), L the batch mean of the distortion loss
    // (distortion_kernels.hip; nerf_train_set_distortion_weights).  0, 0: no kernel of it runs and none of its buffers exists.
    float dist_w[2] = {0.f, 0.f};
    DevBuf d_wdist;                 // the fine pass's dL/dw from the regulariser (N x Sf): that pass's d_w_ext
    DevBuf dist_ray;                // the per-ray losses of the pass at hand (N)
    DevBuf dacc;                    // running sums (3 doubles: L coarse, L fine, gradient computations under the regulariser)
    // mixed_float16 policy (src/ExecutionRun.py:220-221, src/NeRF.py:159-163): single-pass fp16 forward / data gradients
    // and the dynamic loss scale of Keras' LossScaleOptimizer
    bool mixed = false;
    DevBuf opt;                     // OptState (train_kernels.h): loss scale, verdicts, Adam iteration count -- on the device
    DevBuf z_new, d_zm, zero_rgb;   // backward through NeRF.render(): the Sf new depths, d/dz of the merged fine pass
    // nerf_train_render_forward_outputs / _backward_outputs: the last pass's depth output (N), the folded dL/dw of the depth /
    // weights / z cotangents (N x S: that pass's d_w_ext) and a host caller's staged cotangents.  None exists until asked for.
    DevBuf depth, g_wfold, in_dd, in_dw, in_dz;
    // nerf_train_set_ray_gradients: both networks' backward streams carry the encoding tiles, so every pass's chain leaves
    // the encoding gradient that nerf_train_render_backward_rays reduces per ray.  out_ro / out_rd: a host caller's (N, 4)
    // results before they leave; neither exists until asked for.
    bool ray_grads = false;
    DevBuf out_ro, out_rd;
    DevBuf macc;                    // running sums of the step metrics (4 doubles: loss, psnr_coarse, psnr_fine, steps)
    DevBuf gsave[2];                // ... under mixed_float16 with accumulate = 1: the (unscaled) gradients already there
    // A render between optimizer steps (DietNeRF's consistency render every 13th step, the epoch plots) needs the render
    // path's operand streams (nerf_kernels.h::render_streams) re-packed from the trained blob: train_flush_weights does what
    // nerf_load_weights does, from TNet::blob instead of the loaded blob's device copy (repack_render_streams: the ctx's
    // gather tables and one kernel per stream on the ctx stream, no synchronisation).
    std::vector<RenderSlot> slots;  // nerf_train_render_forward / _backward
};

}  // namespace nerf

namespace {

int layer_table(const nerf_config& cfg, TLayer L[12]) {
    const int xd = 3 + 6 * cfg.n_pos_enc_xyz;                    // xyz encoding: 33 at Lx 5
    int dims[12][2];                                             // {K_real, N_real}
    const int n = layer_dims(cfg.n_pos_enc_xyz, cfg.n_pos_enc_dir, cfg.n_angles, dims);
    // {Kp, Np, rowmap} of the reference trainer's padded matrices; rowmap = xd on layer 4 (train_kernels.h, ReduceArgs::rowmap)
    const int with_dirs[11][3] = {{kXyzPad, 256, 0}, {256, 256, 0}, {256, 256, 0}, {256, 256, 0}, {kLdC4, 256, xd}, {256, 256, 0},
                                  {256, 256, 0}, {256, 256, 0}, {kLdC8, 128, 0}, {128, 32, 0}, {kLdC8, 32, 0}};
    const int xyz_only[12][3] = {{kXyzPad, 256, 0}, {256, 256, 0}, {256, 256, 0}, {256, 256, 0}, {kLdC4, 256, xd}, {256, 256, 0},
                                 {256, 256, 0}, {256, 256, 0}, {256, 256, 0}, {256, 128, 0}, {128, 32, 0}, {256, 32, 0}};
    size_t off = 0;
    for (int l = 0; l < n; ++l) {
        const int* pad = cfg.n_angles == 0 ? xyz_only[l] : with_dirs[l];
        L[l].K_real = dims[l][0]; L[l].N_real = dims[l][1]; L[l].Kp = pad[0]; L[l].Np = pad[1]; L[l].rowmap = pad[2];
        L[l].w_off = off; off += (size_t)L[l].K_real * L[l].N_real;
        L[l].b_off = off; off += L[l].N_real;
        L[l].W = L[l].WT = L[l].bias = nullptr;
    }
    return n;
}

void free_buf(DevBuf& b) { if (b.p) (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }

void free_pass(TPass& p) {
    for (DevBuf* b : {&p.C4, &p.C8, &p.H1, &p.H2, &p.H3, &p.H5, &p.H6, &p.H7, &p.H8b, &p.H9, &p.raw, &p.T, &p.w, &p.rgb,
                      &p.z, &p.masks, &p.dxa, &p.dxb, &p.rs, &p.cull.mask, &p.cull.first})
        free_buf(*b);
    for (DevBuf& b : p.D) free_buf(b);
}

void free_slot(RenderSlot& s) {
    for (TPass& p : s.pass) free_pass(p);
    for (DevBuf* b : {&s.o, &s.d, &s.u_c, &s.u_f, &s.z_new}) free_buf(*b);
}

// The encoding window's scale table over layer l's weights (the layout of the blob, as TLayer::w_off), or null: window off, or
// a layer no encoding enters (scale 1 throughout).  What relayout and the gradient reductions of that layer multiply by.
const float* layer_scale(const nerf_ctx* c, const TNet& n, int l) {
    const bool enc = l == 0 || l == 4 || (n.n_layers == 11 && (l == 8 || l == 10));
    return window_scale(c) && enc ? window_scale(c) + n.L[l].w_off : nullptr;
}

int relayout_net(nerf_ctx* c, TNet& n) {
    const TrainState* t = c->train;
    if (!t->reference) {     // the fused kernels read their two re-packed streams and nothing else
        const StreamKind k = t->mixed ? kF16Hi : kF16x3;      // the stash forward reads the render stream of its arithmetic
        StreamDesc d[kStreamKinds];
        render_streams(c->cfg.n_pos_enc_xyz, c->cfg.n_angles, 1, d);
        const float* sc = window_scale(c);     // the encoding window: both streams are packed from the scaled weights
        launch_repack(kElemF16, n.blob, sc, c->rt[k], n.fstream, d[k].bytes / 2, c->rt_cst[kConst16], n.fcst, c->stream);
        launch_repack(kElemF16, n.blob, sc, t->bidx[n.bdx ? 1 : 0], n.bstream, kBwdStreamBytes / 2, nullptr, nullptr, c->stream);
        HIP_OK(hipGetLastError());
        return 0;
    }
    for (int l = 0; l < n.n_layers; ++l) {
        const TLayer& L = n.L[l];
        RelayoutArgs a;
        a.w = n.blob + L.w_off; a.b = n.blob + L.b_off;
        a.scale = layer_scale(c, n, l);
        a.K_real = L.K_real; a.N_real = L.N_real; a.Kp = L.Kp; a.Np = L.Np; a.rowmap = L.rowmap;
        a.W = L.W; a.WT = L.WT; a.bias = L.bias;
        launch_relayout(a, c->stream);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

int alloc_optimizer(nerf_ctx* c, TrainState* t, TNet& n) {
    const size_t nb = t->nblob * sizeof(float);
    if (!n.grad) HIP_OK(hipMalloc((void**)&n.grad, nb));
    if (!n.m) HIP_OK(hipMalloc((void**)&n.m, nb));
    if (!n.v) HIP_OK(hipMalloc((void**)&n.v, nb));
    HIP_OK(hipMemsetAsync(n.m, 0, nb, c->stream));
    HIP_OK(hipMemsetAsync(n.v, 0, nb, c->stream));
    HIP_OK(hipMemsetAsync(n.grad, 0, nb, c->stream));
    return 0;
}

// the fused trainer's operand streams of one network (and, once, the backward gather table they are re-packed with)
int ensure_fused(nerf_ctx* c, TrainState* t, TNet& n) {
    if (int r = ensure_render_tables(c)) return r;
    if (!n.fstream) HIP_OK(hipMalloc(&n.fstream, kStreamBytesF16Xyz));     // the largest of the four streams
    if (!n.fcst) HIP_OK(hipMalloc((void**)&n.fcst, kConstBytes));
    // the fine network's chain also produces the gradient w.r.t. the xyz encoding when the sampler is differentiated; both
    // networks' chains do while ray gradients are switched on
    n.bdx = t->ray_grads || ((&n == &t->net[1]) && t->cfg.sampler_gradient != 0);
    int32_t*& bi = t->bidx[n.bdx ? 1 : 0];
    if (!bi) {
        std::vector<int32_t> idx(kBwdStreamBytes / 2);
        build_bwd_gather(c->cfg.n_angles, n.bdx, t->mixed, idx.data(), pe_layout_lx(c->cfg.n_pos_enc_xyz));
        aim_gather(c->cfg.n_pos_enc_xyz, c->cfg.n_pos_enc_dir, c->cfg.n_angles, idx.data(), idx.size(), true);
        HIP_OK(hipMalloc((void**)&bi, idx.size() * sizeof(int32_t)));
        HIP_OK(hipMemcpy(bi, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    if (!n.bstream) HIP_OK(hipMalloc(&n.bstream, kBwdStreamBytes));
    return 0;
}

int init_net(nerf_ctx* c, TrainState* t, int which) {
    TNet& n = t->net[which];
    n.n_layers = layer_table(c->cfg, n.L);
    const size_t nb = t->nblob * sizeof(float);
    HIP_OK(hipMalloc((void**)&n.blob, nb));
    if (int r = alloc_optimizer(c, t, n)) return r;
    HIP_OK(hipMemcpyAsync(n.blob, c->net[which].host_blob.data(), nb, hipMemcpyHostToDevice, c->stream));
    n.present = true;
    n.render_dirty = n.host_stale = false;
    if (!t->reference) {
        if (int r = ensure_fused(c, t, n)) return r;
    } else {
        size_t mats = 0;
        for (int l = 0; l < n.n_layers; ++l) mats += 2 * (size_t)n.L[l].Kp * n.L[l].Np + n.L[l].Np;   // W, WT, bias
        HIP_OK(hipMalloc((void**)&n.mats, mats * sizeof(float)));
        float* p = n.mats;
        for (int l = 0; l < n.n_layers; ++l) {
            TLayer& L = n.L[l];
            L.W = p; p += (size_t)L.Kp * L.Np;
            L.WT = p; p += (size_t)L.Kp * L.Np;
            L.bias = p; p += L.Np;
        }
    }
    return relayout_net(c, n);
}

// ---- one pass: forward ---------------------------------------------------------------------------
struct PassDims { long long N; int S; long long M, Mp; };

long long padded_rows(long long M) { return (M + 127) / 128 * 128; }      // the network kernels work on whole 128-row tiles
PassDims pass_dims(long long N, int S) { return {N, S, N * S, padded_rows(N * S)}; }

int ensure_pass(nerf_ctx* c, TPass& p, const PassDims& d) {
    const TrainState* t = c->train;
    const size_t f = sizeof(float);
    // the mixed_float16 policy keeps activations and pre-activation gradients in fp16 (same element pitches, half the
    // bytes); the buffers are grow-only and are released by train_free before a trainer of the other policy starts
    const size_t ea = t->mixed ? 2 : f;
    int r = 0;
    r |= ensure(c, p.C4, d.Mp * kLdC4 * ea);
    r |= ensure(c, p.C8, d.Mp * kLdC8 * ea);
    DevBuf* hs[] = {&p.H1, &p.H2, &p.H3, &p.H5, &p.H6, &p.H7};
    for (DevBuf* h : hs) r |= ensure(c, *h, d.Mp * 256 * ea);
    r |= ensure(c, p.H9, d.Mp * 128 * ea);
    const bool xyz = c->cfg.n_angles == 0;
    if (xyz) r |= ensure(c, p.H8b, d.Mp * 256 * f);      // (fp32-sized under either policy)
    r |= ensure(c, p.raw, d.Mp * 4 * f);
    r |= ensure(c, p.T, d.M * f);
    r |= ensure(c, p.w, d.M * f);
    r |= ensure(c, p.rgb, d.N * 3 * f);
    r |= ensure(c, p.z, d.M * f);
    if (t->reference) return r;
    // the fused backward chain's side: mask records, one gradient buffer per layer, the two encoding-gradient parts
    r |= ensure(c, p.masks, (size_t)(xyz ? 10 : 9) * d.Mp * 32);
    for (int l = 0; l < 8; ++l) r |= ensure(c, p.D[l], d.Mp * 256 * ea);
    r |= ensure(c, p.D[8], d.Mp * (xyz ? 256 : 128) * ea);
    if (xyz) r |= ensure(c, p.D[9], d.Mp * 128 * ea);
    r |= ensure(c, p.dxa, d.Mp * kBwdXyzLd * f);
    r |= ensure(c, p.dxb, d.Mp * kBwdXyzLd * f);
    if (!t->mixed) r |= ensure(c, p.rs, (size_t)10 * d.Mp * sizeof(uint16_t));
    return r;
}

void fwd_layer(nerf_ctx* c, const TLayer& L, const float* A, int lda, float* Out, int ldo, long long Mp,
               bool linear_head = false, int n_valid = -1) {
    GemmAbt g{};
    g.A = A; g.lda = lda; g.Bt = L.WT; g.ldb = L.Kp; g.Out = Out; g.ldo = ldo;
    g.M = Mp; g.N = L.Np; g.K = L.Kp; g.bias = L.bias; g.alpha = c->cfg.leaky_relu_alpha;
    g.n_valid = n_valid < 0 ? L.Np : n_valid;
    launch_gemm_abt(linear_head ? EPI_FWD_LINEAR : EPI_FWD_LEAKY, linear_head, g, c->stream);
}

// the reference trainer's Dense stack over Mp encoded rows (C4 / C8 hold the encodings) -> raw_out (Mp x 4)
void forward_layers(nerf_ctx* c, TNet& n, TPass& p, long long Mp, float* raw) {
    float *C4 = (float*)p.C4.p, *C8 = (float*)p.C8.p;
    float *H1 = (float*)p.H1.p, *H2 = (float*)p.H2.p, *H3 = (float*)p.H3.p, *H5 = (float*)p.H5.p,
          *H6 = (float*)p.H6.p, *H7 = (float*)p.H7.p, *H9 = (float*)p.H9.p;
    fwd_layer(c, n.L[0], C4 + 256, kLdC4, H1, 256, Mp);
    fwd_layer(c, n.L[1], H1, 256, H2, 256, Mp);
    fwd_layer(c, n.L[2], H2, 256, H3, 256, Mp);
    fwd_layer(c, n.L[3], H3, 256, C4, kLdC4, Mp);          // h4 lands next to xyz_enc: the skip concat
    fwd_layer(c, n.L[4], C4, kLdC4, H5, 256, Mp);
    fwd_layer(c, n.L[5], H5, 256, H6, 256, Mp);
    fwd_layer(c, n.L[6], H6, 256, H7, 256, Mp);
    fwd_layer(c, n.L[7], H7, 256, C8, kLdC8, Mp);          // h8 lands next to dir_enc
    if (n.n_layers == 11) {
        fwd_layer(c, n.L[8], C8, kLdC8, H9, 128, Mp);
        fwd_layer(c, n.L[9], H9, 128, raw, 4, Mp, true, 3);          // rgb head   -> raw[:, 0:3]
        fwd_layer(c, n.L[10], C8, kLdC8, raw + 3, 4, Mp, true, 1);   // sigma head -> raw[:, 3]
    } else {                                                // xyz-only: h8 -> 256 -> 128 -> rgb; sigma from h8
        float* H8b = (float*)p.H8b.p;
        fwd_layer(c, n.L[8], C8, kLdC8, H8b, 256, Mp);
        fwd_layer(c, n.L[9], H8b, 256, H9, 128, Mp);
        fwd_layer(c, n.L[10], H9, 128, raw, 4, Mp, true, 3);
        fwd_layer(c, n.L[11], C8, kLdC8, raw + 3, 4, Mp, true, 1);
    }
}

// the rows the network kernels of a pass run on: every sample, or the kept ones of a culled pass (TPass::cull)
long long net_rows_padded(const TPass& p, const PassDims& d) { return p.cull.rows < 0 ? d.Mp : padded_rows(p.cull.rows); }
// ... and the pass's record as launch_pe_bwd takes it: nulls for a pass that ran every sample
const uint8_t* cull_mask(const TPass& p) { return p.cull.rows < 0 ? nullptr : (const uint8_t*)p.cull.mask.p; }
const uint32_t* cull_first(const TPass& p) { return p.cull.rows < 0 ? nullptr : (const uint32_t*)p.cull.first.p; }

// depth: where the compositing kernel stores its depth sum (N), for the caller who asked for it
int forward_pass(nerf_ctx* c, TrainState* t, int which, const PassDims& d, const float* o, const float* dirs,
                 float* depth = nullptr) {
    TNet& n = t->net[which];
    TPass& p = t->pass[which];
    float *raw = (float*)p.raw.p, *z = (float*)p.z.p;
    // what the network runs on: the pass's rays and depths (mode 0), or ...
    struct { const float *in_a, *in_b, *z; int S, mode; long long M, Mp; float* raw; } in = {o, dirs, z, d.S, 0, d.M, d.Mp, raw};
    p.cull.rows = -1;
    if (culling_acts(c, c->train_cull_on)) {
        // ... a culled pass: point mode on the compact rows, their raw rows to c->b_craw; with no row kept it does not run at all
        if (int r = compact_samples(c, p.cull, o, dirs, z, d.N, d.S, false)) return r;
        const long long M = p.cull.rows, Mp = padded_rows(M);
        if (int r = ensure(c, c->b_craw, (size_t)Mp * 16)) return r;
        in = {(const float*)c->b_cxyz.p, c->cfg.n_angles != 0 ? (const float*)c->b_cdirs.p : nullptr, nullptr, 1, 1, M, Mp,
              (float*)c->b_craw.p};
    }
    const long long Mp = in.Mp;
    if (in.M > 0)
        launch_train_encode(in.in_a, in.in_b, in.z, 0, in.M, in.S, Mp, c->cfg.n_angles, c->cfg.n_pos_enc_xyz, c->cfg.n_pos_enc_dir,
                            in.mode, (float*)p.C4.p, (float*)p.C8.p, c->stream, t->mixed, !t->reference);
    if (in.M == 0) {
    } else if (t->reference) {
        forward_layers(c, n, p, Mp, in.raw);
    } else {
        if (!n.fstream) return fail("internal: fused training forward without its weight stream");
        // the render path's fused PE + MLP kernel (3-pass split fp16, fp32-class results; one pass under mixed_float16) with
        // every activation also written to the buffers the weight-gradient GEMMs read, and the LeakyReLU' bit records the
        // backward chain reads: 4x the rate of the layer-wise forward
        MlpArgs a{};
        a.wstream = (const float*)n.fstream; a.wconst = n.fcst;
        a.in_a = in.in_a; a.in_b = in.in_b; a.z = in.z; a.raw = in.raw; a.nonfinite = c->nonfinite;
        a.M = in.M; a.S = in.S; a.mode = in.mode; a.alpha = c->cfg.leaky_relu_alpha;
        const bool xyz = c->cfg.n_angles == 0;
        float* dst[10] = {(float*)p.H1.p, (float*)p.H2.p, (float*)p.H3.p, (float*)p.C4.p, (float*)p.H5.p,
                          (float*)p.H6.p, (float*)p.H7.p, (float*)p.C8.p, xyz ? (float*)p.H8b.p : (float*)p.H9.p,
                          xyz ? (float*)p.H9.p : nullptr};
        const int ld[10] = {256, 256, 256, kLdC4, 256, 256, 256, kLdC8, xyz ? 256 : 128, 128};
        for (int i = 0; i < (xyz ? 10 : 9); ++i) {
            a.st_ptr[i] = dst[i]; a.st_ld[i] = ld[i];
            a.mask_ptr[i] = p.masks.p ? (uint32_t*)p.masks.p + (size_t)i * Mp * 8 : nullptr;
        }
#ifdef NERF_DIAG_STASH_WRAP   // diagnostic BUILD only (make EXTRA=-DNERF_DIAG_STASH_WRAP): timing without HBM stores, wrong results
        a.diag_wrap = Mp >= 8192;
#endif
        if (c->cfg.n_pos_enc_xyz > kLx) wide::launch_mlp_f16x3_stash(a, c->num_cus, c->stream, t->mixed, xyz);
        else launch_mlp_f16x3_stash(a, c->num_cus, c->stream, t->mixed, xyz);
    }
    if (p.cull.rows >= 0)     // the full raw buffer, zeros for the culled samples: the compositing runs on all N S samples
        launch_raw_expand(in.raw, d.M, false, cull_mask(p), cull_first(p), raw, c->stream);
    launch_composite(raw, z, d.N, d.S, (float*)p.rgb.p, (float*)p.w.p, (float*)p.T.p, nullptr, nullptr, depth,
                     c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- one pass: backward --------------------------------------------------------------------------
// The 256-wide layers' weight gradients of a pass (fused backward: every D_l exists before the first of them starts) are
// queued and leave as ONE GEMM launch + ONE reduction launch: two rounds of workgroups over the chip with ~56 row slabs per
// layer instead of 256 (a quarter of the partial-sum bytes: 2.1 GB -> 0.45 GB per step), 2 kernel boundaries instead of 16.
struct WgradQueue {
    GemmAtbBatch gemm{};
    ReduceBatch red{};
};

// floats of partial sums a batched launch needs: the layout loop of wgrad_flush, for the slab count it would choose
size_t wgrad_batch_floats(const WgradQueue& q, int splits) {
    size_t off = 0;
    for (int e = 0; e < q.gemm.n; ++e) off += (size_t)splits * (q.gemm.e[e].Kp + 1) * q.gemm.e[e].Nw;
    return off;
}

int join_side(nerf_ctx* c, TrainState* t) {       // the main stream waits for the side stream's weight gradients
    if (t->side_pending) {
        HIP_OK(hipStreamWaitEvent(c->stream, t->ev_join, 0));
        t->side_pending = false;
    }
    return 0;
}

int wgrad_flush(nerf_ctx* c, TrainState* t, WgradQueue& q, long long Mp, bool on_side = false) {
    if (q.gemm.n == 0) return 0;
    hipStream_t st = c->stream;
    DevBuf* pb = &t->partial;
    if (on_side) {
        if (!t->side) {
            HIP_OK(hipStreamCreateWithFlags(&t->side, hipStreamNonBlocking));
            HIP_OK(hipEventCreateWithFlags(&t->ev_fork, hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&t->ev_join, hipEventDisableTiming));
        }
        if (int r = join_side(c, t)) return r;         // (one launch in flight on the side stream at a time)
        HIP_OK(hipEventRecord(t->ev_fork, c->stream));  // everything the GEMM reads has been enqueued on the main stream
        HIP_OK(hipStreamWaitEvent(t->side, t->ev_fork, 0));
        st = t->side;
        pb = &t->partial_side;
    }
    int units = 0;
    for (int e = 0; e < q.gemm.n; ++e) units += (q.gemm.e[e].Kp + 255) / 256 * ((q.gemm.e[e].Nw + 255) / 256);
    // one 512-thread workgroup per CU, workgroups dealt round-robin to the 8 XCDs: a multiple of 8 slabs per layer such
    // that no XCD gets more than two rounds of its 32 CUs (10 units x 51 slabs put 70 workgroups on three of the XCDs:
    // a third round, +47 % on the launch)
    const int per_xcd = std::max(1, 2 * (c->num_cus / 8) / units);
    const int want_splits = 8 * per_xcd;
    long long rps = (Mp + want_splits - 1) / want_splits;
    rps = (rps + 31) / 32 * 32;
    const int splits = (int)((Mp + rps - 1) / rps);
    // the slab count follows the device's CU count: grow the partial-sum buffer to what THIS launch lays out (a device with
    // more CUs, a larger batch of layers) instead of trusting the size the per-layer launches were given
    if (int r = ensure(c, *pb, wgrad_batch_floats(q, splits) * sizeof(float))) { q.gemm.n = q.red.n = 0; return r; }
    size_t off = 0;
    for (int e = 0; e < q.gemm.n; ++e) {
        GemmAtb& g = q.gemm.e[e];
        g.rows_per_split = (int)rps;
        g.partial = (float*)pb->p + off;
        q.red.e[e].partial = g.partial;
        q.red.e[e].splits = splits;
        off += (size_t)splits * (g.Kp + 1) * g.Nw;
    }
    if (t->mixed) launch_gemm_atb_f16_batch(q.gemm, st);
    else launch_gemm_atb_p_batch(q.gemm, st);
    launch_reduce_grad_batch(q.red, st);
    q.gemm.n = q.red.n = 0;
    if (on_side) {
        HIP_OK(hipEventRecord(t->ev_join, t->side));
        t->side_pending = true;
    }
    return 0;
}

// One weight-gradient launch of layer l and its reduction into the gradient blob: the GEMM's operands, the row slabs (about
// `want_splits` of them, whole multiples of `row_quantum` rows), the slab sums' destination
struct Wgrad { GemmAtb g; ReduceArgs r; int splits; };

Wgrad wgrad_args(const nerf_ctx* c, TrainState* t, TNet& n, int l, const float* A, int lda, const float* G, int ldg, int Ncols,
                 int n_src_off, long long Mp, int want_splits, int row_quantum) {
    const TLayer& L = n.L[l];
    Wgrad w{};
    GemmAtb& g = w.g;
    g.A = A; g.lda = lda; g.K = L.Kp; g.G = G; g.ldg = ldg; g.N = Ncols;
    g.partial = (float*)t->partial.p; g.Kp = L.Kp; g.Nw = Ncols; g.M = Mp;
    g.a_f16 = t->mixed ? 1 : 0;
    long long rps = (Mp + want_splits - 1) / want_splits;
    rps = (rps + row_quantum - 1) / row_quantum * row_quantum;
    g.rows_per_split = (int)rps;
    w.splits = (int)((Mp + rps - 1) / rps);
    ReduceArgs& r = w.r;
    r.partial = g.partial; r.Kp = L.Kp; r.Nw = Ncols; r.splits = w.splits;
    r.grad_w = n.grad + L.w_off; r.grad_b = n.grad + L.b_off;
    r.K_real = L.K_real; r.N_real = L.N_real; r.n_src_off = n_src_off; r.rowmap = L.rowmap;
    r.accumulate = t->acc_grads ? 1 : 0;
    r.scale_w = layer_scale(c, n, l);
    return w;
}

// The reference trainer: exact fp32 MFMA (the heads: the VALU kernel) over row-major operands, 16-row slab quantum
void wgrad_reference(nerf_ctx* c, TrainState* t, TNet& n, int l, const float* A, int lda, const float* G, int ldg, int Ncols,
                     int n_src_off, long long Mp) {
    // the heads' (K x 4) results come from a VALU kernel that wants many small slabs; their inputs are H9 (128 wide) and
    // C8 (kLdC8 wide, its first 256 columns for the xyz-only network's sigma head): whole, 16-byte-aligned column quads,
    // at most 256 of them, as head_wgrad_rows_kernel requires
    static_assert(kLdC8 % 4 == 0 && kLdC8 <= 1024, "head_wgrad_rows_kernel: Kp % 4 == 0, Kp <= 1024, lda % 4 == 0");
    const Wgrad w = wgrad_args(c, t, n, l, A, lda, G, ldg, Ncols, n_src_off, Mp, Ncols == 4 ? 1024 : kTrainSplits, 16);
    if (Ncols == 4) launch_head_wgrad(w.g, false, c->stream);
    else launch_gemm_atb(w.g, c->stream);
    launch_reduce_grad(w.r, c->stream);
}

// The fused trainer's three forms (fragment-major operands: slabs of whole 32-row blocks).  D: layer l's pre-activation
// gradient from the backward chain, rs / gmax: its row factors (pair16, float32 policy; else null) and max|D| slots.
// A 256-wide layer joins the pass's batched launch.  wgrad_flush owns the slab layout of a queued entry: it sets
// rows_per_split, partial and splits of both halves for the batch as a whole, whatever wgrad_args put there.
int wgrad_queue(const nerf_ctx* c, TrainState* t, TNet& n, int l, const float* A, int lda, const float* D, const uint16_t* rs,
                const unsigned* gmax, long long Mp, WgradQueue& q) {
    if (q.gemm.n >= kWgradBatchMax) return fail("internal: more 256-wide layers than a batched weight-gradient launch holds");
    Wgrad w = wgrad_args(c, t, n, l, A, lda, D, 256, 256, 0, Mp, kTrainSplitsWide, 32);
    w.g.g_rs = rs; w.g.gmax = gmax;
    q.gemm.e[q.gemm.n++] = w.g;
    q.red.e[q.red.n++] = w.r;
    return 0;
}

// The 128-wide layer (8; 9 in the xyz-only network) on the 128 tile.  sig_layer >= 0: the GEMM also produces the weight gradient
// of that head (the sigma head: its input is A = C8, its gradient t->dsig) -- it stages C8 anyway, no second pass over that buffer;
// the head's slab sums land behind this GEMM's.
void wgrad_tile128(nerf_ctx* c, TrainState* t, TNet& n, int l, const float* A, int lda, const float* D, const uint16_t* rs,
                   const unsigned* gmax, long long Mp, int sig_layer = -1) {
    Wgrad w = wgrad_args(c, t, n, l, A, lda, D, 128, 128, 0, Mp, kTrainSplits, 32);
    w.g.g_rs = rs; w.g.gmax = gmax;
    if (sig_layer >= 0) {
        w.g.sig_g = (const float*)t->dsig.p;
        w.g.sig_partial = w.g.partial + (size_t)w.splits * (w.g.Kp + 1) * w.g.Nw;
    }
    if (t->mixed) launch_gemm_atb_f16(w.g, c->stream);
    else launch_gemm_atb_p(w.g, c->stream);
    launch_reduce_grad(w.r, c->stream);
    if (sig_layer >= 0) {
        const TLayer& Ls = n.L[sig_layer];
        ReduceArgs sig_r{};
        sig_r.partial = w.g.sig_partial; sig_r.Kp = w.g.Kp; sig_r.Nw = 1; sig_r.splits = w.splits;
        sig_r.grad_w = n.grad + Ls.w_off; sig_r.grad_b = n.grad + Ls.b_off;
        sig_r.K_real = Ls.K_real; sig_r.N_real = 1; sig_r.n_src_off = 0; sig_r.rowmap = Ls.rowmap;
        sig_r.accumulate = t->acc_grads ? 1 : 0;
        sig_r.scale_w = layer_scale(c, n, sig_layer);
        launch_reduce_grad(sig_r, c->stream);
    }
}

// A head (4-wide G = column n_src_off.. of Graw, row-major) on the VALU kernel, which wants many small slabs
void wgrad_head(nerf_ctx* c, TrainState* t, TNet& n, int l, const float* A, int lda, const float* Graw, int n_src_off,
                long long Mp) {
    const Wgrad w = wgrad_args(c, t, n, l, A, lda, Graw, 4, 4, n_src_off, Mp, 1024, 32);
    launch_head_wgrad(w.g, true, c->stream);
    launch_reduce_grad(w.r, c->stream);
}

void dgrad(nerf_ctx* c, const float* G, int ldg, int Kg, const float* Wrows, int ldb, int Nout, const float* H, int ldh,
           float* Out, int ldo, long long Mp, const float* r1a = nullptr, const float* r1b = nullptr) {
    GemmAbt g{};
    g.A = G; g.lda = ldg; g.Bt = Wrows; g.ldb = ldb; g.Out = Out; g.ldo = ldo;
    g.M = Mp; g.N = Nout; g.K = Kg; g.H = H; g.ldh = ldh; g.r1a = r1a; g.r1a_ld = 4; g.r1b = r1b;
    g.n_valid = Nout; g.alpha = c->cfg.leaky_relu_alpha;
    launch_gemm_abt(EPI_BWD_MASK, false, g, c->stream);
}

void dgrad_xyz(nerf_ctx* c, const float* G, const float* Wrows, float* dA0, long long Mp, bool accumulate) {
    GemmAbt g{};
    g.A = G; g.lda = 256; g.Bt = Wrows; g.ldb = 256; g.Out = dA0; g.ldo = kXyzPad;
    g.M = Mp; g.N = kXyzPad; g.K = 256; g.n_valid = kXyzPad; g.accumulate = accumulate ? 1 : 0;
    launch_gemm_abt(EPI_BWD_PLAIN, true, g, c->stream);
}

// The two backward passes below: Graw (Mp x 4, padding rows zero) must be filled; they write n.grad; with d_z != NULL they
// add dL/dz through the sample positions (d_z must already hold the compositing part).  For a culled pass (TPass::cull.rows >= 0)
// Mp is the kept rows' padded count, Graw is TrainState::Gc and d_z gets its addition at the kept samples only.

// rays: where the pass adds its share of dL/d(rays_orig), dL/d(rays_dirs) ((N, 4) on the device, zeroed by the caller; either
// may be null) -- the fused trainer with encoding tiles only (nerf_train_set_ray_gradients refuses the reference trainer).
struct RayGrads {
    float *d_o = nullptr, *d_d = nullptr;
    bool any() const { return d_o || d_d; }
};

// The fused trainer: ONE kernel for the whole data-gradient chain (mlp_bwd_f16x3.hip: the gradient stays on the lane from
// layer to layer; every D_l is written once, with max|D_l| in the pass's gmax slots), then the weight gradients from the
// stashed activations and the D_l.
int backward_fused(nerf_ctx* c, TrainState* t, int which, const PassDims& d, const float* o, const float* dirs, float* d_z,
                   const RayGrads& rays = RayGrads()) {
    TNet& n = t->net[which];
    TPass& p = t->pass[which];
    const long long Mp = net_rows_padded(p, d);
    const float* Graw = (const float*)(p.cull.rows < 0 ? t->Graw.p : t->Gc.p);
    float *C4 = (float*)p.C4.p, *C8 = (float*)p.C8.p;
    float *H1 = (float*)p.H1.p, *H2 = (float*)p.H2.p, *H3 = (float*)p.H3.p, *H5 = (float*)p.H5.p,
          *H6 = (float*)p.H6.p, *H7 = (float*)p.H7.p, *H9 = (float*)p.H9.p;
    // gm + 64 k: bits of max|D| of the gradient buffer the chain produces k-th in this pass (scale of gemm_atb_p's operand;
    // gemm_atb_f16 reads none: no reset under mixed_float16)
    unsigned* gm = t->gmax.p ? (unsigned*)t->gmax.p + (size_t)which * 16 * 64 : nullptr;   // per pass
    if (!(n.bstream && n.fcst && p.masks.p && gm))
        return fail("internal: fused training backward without its stream / mask records");
    if (!t->mixed) HIP_OK(hipMemsetAsync(gm, 0, 16 * 64 * sizeof(unsigned), c->stream));
    MlpBwdArgs b{};
    b.wstream = n.bstream; b.wconst = n.fcst; b.graw = Graw; b.gmax = gm; b.Mp = Mp;
    b.alpha = c->cfg.leaky_relu_alpha;
    b.ld = 256; b.ld9 = 128;
    const bool xyz = n.n_layers == 12;
    const int nrec = xyz ? 10 : 9;                   // mask records / gradient buffers; gmax group k <-> d_ptr[nrec - 1 - k]
    for (int l = 0; l < nrec; ++l) {
        b.mask_ptr[l] = (const uint32_t*)p.masks.p + (size_t)l * Mp * 8;
        b.d_ptr[l] = (float*)p.D[l].p;
        b.rs_ptr[l] = t->mixed ? nullptr : (uint16_t*)p.rs.p + (size_t)l * Mp;     // row factors of d_ptr[l] (pair16)
    }
    b.dx_ptr[0] = (float*)p.dxa.p; b.dx_ptr[1] = (float*)p.dxb.p;
    b.dsig = xyz ? nullptr : (float*)t->dsig.p;
    launch_mlp_bwd_f16x3(b, n.bdx, t->mixed, c->num_cus, c->stream, xyz);
    WgradQueue wq;
    // layer l's gradient buffer is d_ptr[l], its gmax group nrec - 1 - l
    auto queue = [&](int l, const float* A, int lda) {
        return wgrad_queue(c, t, n, l, A, lda, b.d_ptr[l], b.rs_ptr[l], gm + 64 * (nrec - 1 - l), Mp, wq);
    };
    if (xyz) {
        // get_network_only_xyz (src/NeRF.py:248-288): 10 = the rgb head on h9, 11 = the sigma head on h8 (the first 256
        // columns of C8), 9 = 256 -> 128 on the extra layer's output, 8 = that extra 256 -> 256 layer on h8
        wgrad_head(c, t, n, 10, H9, 128, Graw, 0, Mp);
        wgrad_head(c, t, n, 11, C8, kLdC8, Graw, 3, Mp);
        wgrad_tile128(c, t, n, 9, (const float*)p.H8b.p, 256, b.d_ptr[9], b.rs_ptr[9], gm, Mp);
        if (int r = queue(8, C8, kLdC8)) return r;
    } else {
        wgrad_head(c, t, n, 9, H9, 128, Graw, 0, Mp);
        // the sigma head (layer 10: input C8 = [h8 | dir_enc], gradient column 3 of Graw) rides in layer 8's GEMM
        wgrad_tile128(c, t, n, 8, C8, kLdC8, b.d_ptr[8], b.rs_ptr[8], gm, Mp, 10);
    }
    // (the xyz encoding's columns 256.. of C4: in the fragment-major buffer a column offset c is 32 c ELEMENTS --
    // half the byte offset under the fp16 policy)
    const size_t xyz_off = (size_t)32 * 256;
    const float* c4_xyz = t->mixed ? reinterpret_cast<const float*>(reinterpret_cast<const uint16_t*>(C4) + xyz_off) : C4 + xyz_off;
    const float* in[8] = {c4_xyz, H1, H2, H3, C4, H5, H6, H7};       // input of layer l
    for (int l = 7; l >= 0; --l)
        if (int r = queue(l, in[l], l == 0 || l == 4 ? kLdC4 : 256)) return r;
    // the fine pass's batched launch can run beside the coarse pass's backward (which reads none of its operands)
    if (int r = wgrad_flush(c, t, wq, Mp, t->overlap && which == 1 && !t->acc_grads)) return r;
    if (d_z) {
        if (!n.bdx) return fail("internal: the sampler term needs the backward stream with encoding tiles");
        // the chain's encoding tiles are laid out for kLx (wide-PE: kLxWide) octaves; the ones the network lacks carry
        // zero gradient
        launch_pe_bwd(b.dx_ptr[0], b.dx_ptr[1], o, dirs, (const float*)p.z.p, d.N, d.S, pe_layout_lx(c->cfg.n_pos_enc_xyz),
                      cull_mask(p), cull_first(p), d_z, c->stream, true);
    }
    if (rays.any()) {
        if (!n.bdx) return fail("internal: ray gradients need the backward stream with encoding tiles");
        const OptState* st = t->mixed ? (const OptState*)t->opt.p : nullptr;      // the chain carried the loss scale
        launch_ray_position_grads(b.dx_ptr[0], b.dx_ptr[1], o, dirs, (const float*)p.z.p, d.N, d.S,
                                  pe_layout_lx(c->cfg.n_pos_enc_xyz), cull_mask(p), cull_first(p), st, rays.d_o, rays.d_d,
                                  c->stream, true);
        if (rays.d_d && !xyz) {
            // the direction encoding is rows 256.. of the inputs of layer 8 and of the sigma head (10): layer_table's K_real
            const TLayer &L8 = n.L[8], &L9 = n.L[9], &L10 = n.L[10];
            if (L8.K_real - 256 != 2 * c->cfg.n_pos_enc_dir * (c->cfg.n_angles + 1) || L10.K_real != L8.K_real || L8.N_real != 128)
                return fail("internal: the layer table does not match the view-direction encoding");
            launch_view_dir_grads(Graw, p.H9.p, t->mixed, n.blob + L9.w_off, n.blob + L8.w_off + (size_t)256 * L8.N_real,
                                  n.blob + L10.w_off + 256, dirs, d.N, d.S, c->cfg.n_angles, c->cfg.n_pos_enc_dir, cull_mask(p),
                                  cull_first(p), c->cfg.leaky_relu_alpha, st, rays.d_d, c->stream,
                                  // (this kernel reads the master blob, not a packed stream: it scales the two blocks itself)
                                  layer_scale(c, n, 8) ? layer_scale(c, n, 8) + (size_t)256 * L8.N_real : nullptr,
                                  layer_scale(c, n, 10) ? layer_scale(c, n, 10) + 256 : nullptr);
        }
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// The reference trainer: layer by layer, the data gradient (gemm_abt, LeakyReLU' mask from the stored activation) ping-pongs
// between Ga and Gb, each layer's weight gradient follows from its stored input
int backward_reference(nerf_ctx* c, TrainState* t, int which, const PassDims& d, const float* o, const float* dirs, float* d_z) {
    TNet& n = t->net[which];
    TPass& p = t->pass[which];
    const long long Mp = net_rows_padded(p, d);
    float *C4 = (float*)p.C4.p, *C8 = (float*)p.C8.p;
    float *H1 = (float*)p.H1.p, *H2 = (float*)p.H2.p, *H3 = (float*)p.H3.p, *H5 = (float*)p.H5.p,
          *H6 = (float*)p.H6.p, *H7 = (float*)p.H7.p, *H9 = (float*)p.H9.p;
    float *Ga = (float*)t->Ga.p, *Gb = (float*)t->Gb.p, *G9 = (float*)t->G9.p,
          *Graw = (float*)(p.cull.rows < 0 ? t->Graw.p : t->Gc.p), *dA0 = (float*)t->dA0.p;
    const bool dx = d_z != nullptr;
    auto wgrad = [&](int l, const float* A, int lda, const float* G, int ldg, int Ncols, int n_src_off = 0) {
        wgrad_reference(c, t, n, l, A, lda, G, ldg, Ncols, n_src_off, Mp);
    };
    if (n.n_layers == 11) {
        wgrad(9, H9, 128, Graw, 4, 4);
        wgrad(10, C8, kLdC8, Graw, 4, 4, 3);
        launch_head_bwd(Graw, n.L[9].W, H9, Mp, c->cfg.leaky_relu_alpha, G9, c->stream);
        wgrad(8, C8, kLdC8, G9, 128, 128);
        // dL/dh8 = G9 . W8[hidden rows]^T + Graw[:,3] * W10[hidden rows]   (WT10 row 0 = the sigma head's column)
        dgrad(c, G9, 128, 128, n.L[8].W, 128, 256, C8, kLdC8, Ga, 256, Mp, Graw + 3, n.L[10].WT);
    } else {
        float* H8b = (float*)p.H8b.p;
        wgrad(10, H9, 128, Graw, 4, 4);
        wgrad(11, C8, kLdC8, Graw, 4, 4, 3);
        launch_head_bwd(Graw, n.L[10].W, H9, Mp, c->cfg.leaky_relu_alpha, G9, c->stream);
        wgrad(9, H8b, 256, G9, 128, 128);
        dgrad(c, G9, 128, 128, n.L[9].W, 128, 256, H8b, 256, Gb, 256, Mp);    // -> pre-activation grad of h8b
        wgrad(8, C8, kLdC8, Gb, 256, 256);
        // dL/dh8 = Gb . W8^T + Graw[:,3] * W11   (WT11 row 0 = the sigma head's column)
        dgrad(c, Gb, 256, 256, n.L[8].W, 256, 256, C8, kLdC8, Ga, 256, Mp, Graw + 3, n.L[11].WT);
    }
    wgrad(7, H7, 256, Ga, 256, 256);
    dgrad(c, Ga, 256, 256, n.L[7].W, 256, 256, H7, 256, Gb, 256, Mp);
    wgrad(6, H6, 256, Gb, 256, 256);
    dgrad(c, Gb, 256, 256, n.L[6].W, 256, 256, H6, 256, Ga, 256, Mp);
    wgrad(5, H5, 256, Ga, 256, 256);
    dgrad(c, Ga, 256, 256, n.L[5].W, 256, 256, H5, 256, Gb, 256, Mp);
    wgrad(4, C4, kLdC4, Gb, 256, 256);
    dgrad(c, Gb, 256, 256, n.L[4].W, 256, 256, C4, kLdC4, Ga, 256, Mp);
    if (dx) dgrad_xyz(c, Gb, n.L[4].W + (size_t)256 * 256, dA0, Mp, false);     // skip connection's xyz rows
    wgrad(3, H3, 256, Ga, 256, 256);
    dgrad(c, Ga, 256, 256, n.L[3].W, 256, 256, H3, 256, Gb, 256, Mp);
    wgrad(2, H2, 256, Gb, 256, 256);
    dgrad(c, Gb, 256, 256, n.L[2].W, 256, 256, H2, 256, Ga, 256, Mp);
    wgrad(1, H1, 256, Ga, 256, 256);
    dgrad(c, Ga, 256, 256, n.L[1].W, 256, 256, H1, 256, Gb, 256, Mp);
    wgrad(0, C4 + 256, kLdC4, Gb, 256, 256);
    if (dx) {
        dgrad_xyz(c, Gb, n.L[0].W, dA0, Mp, true);
        launch_pe_bwd(dA0, nullptr, o, dirs, (const float*)p.z.p, d.N, d.S, c->cfg.n_pos_enc_xyz, cull_mask(p), cull_first(p),
                      d_z, c->stream);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// dL/d(rgb) of pass `which` [+ dL/d(weights) from the sampler, d_wext] -> Graw through the compositing -> the network's
// gradient blob [+ dL/dz into d_z]
int composite_backward_pass(nerf_ctx* c, TrainState* t, int which, const PassDims& pd, const float* o, const float* dirs,
                            const float* d_rgb, const float* d_wext, float* d_z, const RayGrads& rays = RayGrads()) {
    const TPass& p = t->pass[which];
    float* Graw = (float*)t->Graw.p;
    HIP_OK(hipMemsetAsync(Graw + pd.M * 4, 0, (pd.Mp - pd.M) * 4 * sizeof(float), c->stream));
    launch_composite_bwd((const float*)p.raw.p, (const float*)p.z.p, (const float*)p.T.p, pd.N, pd.S, d_rgb, d_wext, Graw,
                         d_z, c->stream);
    if (p.cull.rows == 0) {
        // a culled pass that kept no row: no network kernel ran forward, none runs backward; the pass contributes exact zeros
        // to the network's gradient (stored, or added: nothing to do) and nothing to d_z beyond the compositing's own terms
        if (!t->acc_grads) HIP_OK(hipMemsetAsync(t->net[which].grad, 0, t->nblob * sizeof(float), c->stream));
        return 0;
    }
    if (p.cull.rows > 0) {
        const long long Mp = padded_rows(p.cull.rows);
        if (int r = ensure(c, t->Gc, (size_t)Mp * 4 * sizeof(float))) return r;
        launch_graw_gather(Graw, pd.M, p.cull.rows, Mp, cull_mask(p), cull_first(p), (float*)t->Gc.p, c->stream);
    }
    return t->reference ? backward_reference(c, t, which, pd, o, dirs, d_z)
                        : backward_fused(c, t, which, pd, o, dirs, d_z, rays);
}

// the sample counts of a training call; *fine: whether the fine pass runs
int check_samples(const TrainState* t, long long N, int Sc, int Sf, bool* fine) {
    if (N <= 0) return fail("need at least one ray (got %lld)", N);
    if (Sc < 1 || Sc > 1024) return fail("bad coarse sample count %d", Sc);
    *fine = Sf > 0 && t->net[1].present;
    if (!*fine) return 0;
    if (Sc < 2) return fail("hierarchical sampling needs at least 2 coarse samples (got %d)", Sc);
    if (Sf > kTrainMaxFine) return fail("training supports at most %d fine samples per ray (got %d)", kTrainMaxFine, Sf);
    // same budget as the render path's sampler (nerf_api.hip): the backward sampler was validated up to 64 KiB of LDS
    if (sample_pdf_lds_bytes(Sc, Sf) > 64 * 1024 || sample_pdf_bwd_lds_bytes(Sc, Sf) > 64 * 1024)
        return fail("Sc=%d Sf=%d exceeds the sampler's LDS budget (forward %zu B, backward %zu B, limit 65536 B)", Sc, Sf,
                    sample_pdf_lds_bytes(Sc, Sf), sample_pdf_bwd_lds_bytes(Sc, Sf));
    return 0;
}

// the buffers every backward needs, for passes of up to Mmax (padded) rows and a coarse pass of Mc rows
int ensure_bwd_workspace(nerf_ctx* c, TrainState* t, long long Mmax, long long Mc) {
    const size_t f = sizeof(float);
    int r = ensure(c, t->Graw, Mmax * 4 * f);
    r |= ensure(c, t->partial, (size_t)2 * kTrainSplitsWide * (kLdC4 + 1) * 256 * f);   // also holds a pass's batched slabs
    r |= ensure(c, t->d_wext, Mc * f);
    if (t->reference) {     // the layer-wise data gradients' buffers (the fused chain keeps its own per pass: TPass::D, dxa, dxb)
        r |= ensure(c, t->Ga, Mmax * 256 * f);
        r |= ensure(c, t->Gb, Mmax * 256 * f);
        r |= ensure(c, t->G9, Mmax * 128 * f);
        r |= ensure(c, t->dA0, Mmax * kXyzPad * f);
    } else {
        r |= ensure(c, t->dsig, Mmax * f);
        r |= ensure(c, t->gmax, 2 * 16 * 64 * sizeof(unsigned));
    }
    return r;
}

int gradients_impl(nerf_ctx* c, const float* rays_o, const float* rays_d, const float* target, int64_t N, int Sc,
                   int Sf, const float* u_c, const float* u_f, uint64_t seed, int mem) {
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (!rays_o || !rays_d || !target) return fail("NULL argument");
    bool fine;
    if (int r = check_samples(t, N, Sc, Sf, &fine)) return r;
    if (int r = sampling_ok(c)) return r;
    const size_t f = sizeof(float);
    Staging st(c, mem);      // inputs only: the outputs are the trainer's own buffers, and leave through copy_out
    const float* o = st.in(t->o, rays_o, N * 4 * f);
    const float* d = st.in(t->d, rays_d, N * 4 * f);
    const float* tg = st.in(t->tgt, target, N * 3 * f);
    const float* uc = st.in(t->u_c, u_c, (size_t)N * Sc * f);
    const float* uf = st.in(t->u_f, fine ? u_f : nullptr, (size_t)N * (fine ? Sf : 0) * f);
    if (st.err) return st.err;

    const PassDims dc = pass_dims(N, Sc), df = pass_dims(N, Sf);     // the fine pass renders the Sf new samples only
    int r = ensure_pass(c, t->pass[0], dc);
    if (fine) r |= ensure_pass(c, t->pass[1], df);
    r |= ensure_bwd_workspace(c, t, fine && df.Mp > dc.Mp ? df.Mp : dc.Mp, dc.M);
    r |= ensure(c, t->d_rgb, N * 3 * f);
    r |= ensure(c, t->d_zf, (fine ? df.M : 1) * f);
    r |= ensure(c, t->scal, 4 * f);
    if (!t->macc.p) {                             // (cleared when it is created, whatever else failed to grow)
        const int rm = ensure(c, t->macc, 4 * sizeof(double));
        if (!rm) HIP_OK(hipMemsetAsync(t->macc.p, 0, 4 * sizeof(double), c->stream));
        r |= rm;
    }
    // the distortion regulariser of a pass (TrainState::dist_w): its buffers exist only once a weight is non-zero
    const bool dist_c = t->dist_w[0] > 0.f, dist_f = fine && t->dist_w[1] > 0.f;
    if (dist_c || dist_f) {
        if (!(c->cfg.far_boundary > c->cfg.near_boundary))
            return fail("the distortion loss needs far_boundary > near_boundary (got %g, %g)", c->cfg.near_boundary,
                        c->cfg.far_boundary);
        r |= ensure(c, t->dist_ray, N * f);
        if (dist_f) r |= ensure(c, t->d_wdist, df.M * f);
        if (!t->dacc.p) {
            const int rd = ensure(c, t->dacc, 3 * sizeof(double));
            if (!rd) HIP_OK(hipMemsetAsync(t->dacc.p, 0, 3 * sizeof(double), c->stream));
            r |= rd;
        }
    }
    if (r) return r;
    // factor * (st->scale) * dL/dw of pass `which` -> d_w (stored, or added to the sampler's), its mean loss -> the running sums
    auto distortion = [&](int which, const PassDims& pd, float* d_w, bool add_w, bool count_step) {
        const TPass& p = t->pass[which];
        launch_distortion((const float*)p.w.p, (const float*)p.z.p, pd.N, pd.S, c->cfg.near_boundary, c->cfg.far_boundary,
                          (const OptState*)t->opt.p, t->dist_w[which] / (float)pd.N, (float*)t->dist_ray.p, d_w, add_w, nullptr,
                          false, c->stream);
        launch_distortion_mean((const float*)t->dist_ray.p, pd.N, which, count_step, (double*)t->dacc.p, c->stream);
    };
    float* scal = (float*)t->scal.p;
    float* d_rgb = (float*)t->d_rgb.p;
    // the finiteness flag collects over ONE gradient computation: gradients that were computed and never applied
    // (nerf_train_gradients without nerf_train_apply) must not decide the next step's verdict
    if (t->mixed) launch_opt_begin((OptState*)t->opt.p, c->stream);
    if (!fine && t->net[1].present)   // a skipped fine pass must not move the fine network
        HIP_OK(hipMemsetAsync(t->net[1].grad, 0, t->nblob * f, c->stream));

    // coarse forward (src/NeRF.py:146-151)
    TPass& pc = t->pass[0];
    if (int q = draw_z_values(c, o, d, N, Sc, uc, seed, 0, (float*)pc.z.p)) return q;
    if (int q = forward_pass(c, t, 0, dc, o, d)) return q;
    const bool through_sampler = fine && t->cfg.sampler_gradient != 0;
    if (fine) {
        // fine forward on the Sf new samples only (src/NeRF.py:155-157)
        TPass& pf = t->pass[1];
        launch_sample_pdf((const float*)pc.w.p, (const float*)pc.z.p, N, Sc, Sf, uf, seed, 0, (float*)pf.z.p, nullptr,
                          c->stream);
        if (int q = forward_pass(c, t, 1, df, o, d)) return q;
        launch_mse((const float*)pf.rgb.p, tg, N, (const OptState*)t->opt.p, t->loss_w[1], d_rgb, scal + 1, c->stream);
        float* d_zf = through_sampler ? (float*)t->d_zf.p : nullptr;
        if (dist_f) distortion(1, df, (float*)t->d_wdist.p, false, true);
        if (int q = composite_backward_pass(c, t, 1, df, o, d, d_rgb, dist_f ? (const float*)t->d_wdist.p : nullptr, d_zf))
            return q;
        // the regulariser's own dL/dz joins the pass's d_z AFTER the compositing backward, which stores there (the fine depths
        // have a consumer only under sampler_gradient; the coarse depths are data)
        if (dist_f && d_zf)
            launch_distortion((const float*)pf.w.p, (const float*)pf.z.p, N, Sf, c->cfg.near_boundary, c->cfg.far_boundary,
                              (const OptState*)t->opt.p, t->dist_w[1] / (float)N, nullptr, nullptr, false, d_zf, true, c->stream);
        if (through_sampler)
            launch_sample_pdf_bwd((const float*)pc.w.p, (const float*)pc.z.p, N, Sc, Sf, uf, seed, 0, d_zf,
                                  (float*)t->d_wext.p, c->stream);
    }
    launch_mse((const float*)pc.rgb.p, tg, N, (const OptState*)t->opt.p, t->loss_w[0], d_rgb, scal + 0, c->stream);
    if (dist_c) distortion(0, dc, (float*)t->d_wext.p, through_sampler, !dist_f);
    if (int q = composite_backward_pass(c, t, 0, dc, o, d, d_rgb,
                                        through_sampler || dist_c ? (const float*)t->d_wext.p : nullptr, nullptr))
        return q;
    if (int q = join_side(c, t)) return q;
    if (t->mixed) {
        // LossScaleOptimizer: unscale, test for Inf/NaN; the verdict is taken on the device (opt_verdict_kernel) and gates
        // this step's Adam update.  (The per-sample scaling of the backward chain makes the products themselves
        // scale-invariant; the loss scale still guards the compositing / sampler backward and gives the reference's
        // skip-step behaviour.)
        launch_unscale_check(t->net[0].grad, fine ? t->net[1].grad : nullptr, t->nblob, (OptState*)t->opt.p, c->stream);
    }
    launch_metrics_accum(scal, fine, t->loss_w[0], t->loss_w[1], (double*)t->macc.p, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

// The verdict of the gradients just computed, on the device: loss-scale bookkeeping (mixed_float16 policy: Keras 2.7
// LossScaleOptimizer -- halve on a non-finite step, double after `growth` finite ones) and the flag that lets this step's
// Adam launches through.  No host round trip: nerf_train_step keeps enqueuing.
// The verdict is taken on the blobs that are about to be APPLIED -- after a gradient all-reduce (the library's own, or the
// caller's between nerf_train_gradients and nerf_train_apply) those are the reduced blobs, on which every rank reaches
// the same verdict by itself: a non-finite shard makes the sum non-finite everywhere.
void take_verdict(nerf_ctx* c, bool recheck) {
    TrainState* t = c->train;
    if (t->mixed && recheck)
        launch_unscale_check(t->net[0].grad, t->net[1].present ? t->net[1].grad : nullptr, t->nblob, (OptState*)t->opt.p,
                             c->stream, true);
    launch_opt_verdict((OptState*)t->opt.p, c->stream);
}

// Backward through NeRF.render() itself (src/NeRF.py:109-134), the graph DietNeRF's consistency loss differentiates
// (src/DietNeRF.py:204-222): coarse pass -> inverse-CDF samples -> fine pass on sort(concat(z_new, z_coarse)) -> rgb.
// Given d_rgb = dL/d(render()[0]) it leaves dL/d(weights) of both networks in (or adds it to) the gradient blobs:
// the fine network through its Sc+Sf merged samples, the coarse network only through the sampler (its own rgb is
// not an output of render() when a fine network exists).  nerf_train_render_gradients runs the two cores below back to back;
// nerf_train_render_forward / _backward run one each, with the activations kept in a RenderSlot in between.

// The forward half, on TrainState::pass / z_new: coarse pass -> z_new and the merged, sorted depths -> fine pass.
int render_forward_core(nerf_ctx* c, TrainState* t, const PassDims& dc, const PassDims& df, bool fine, const float* o,
                        const float* d, const float* uc, const float* uf, uint64_t seed, long long ray_base,
                        float* depth = nullptr) {              // depth: of the last pass, or null
    const long long N = dc.N;
    const int Sc = dc.S, Sf = df.S - dc.S;                           // the fine pass renders the Sc + Sf merged samples
    if (int q = sampling_ok(c)) return q;
    int r = ensure_pass(c, t->pass[0], dc);
    if (fine) r |= ensure_pass(c, t->pass[1], df);
    r |= ensure(c, t->z_new, (fine ? N * (long long)Sf : 1) * sizeof(float));
    if (r) return r;
    TPass& pc = t->pass[0];
    if (int q = draw_z_values(c, o, d, N, Sc, uc, seed, ray_base, (float*)pc.z.p)) return q;
    if (int q = forward_pass(c, t, 0, dc, o, d, fine ? nullptr : depth)) return q;
    if (!fine) return 0;
    launch_sample_pdf((const float*)pc.w.p, (const float*)pc.z.p, N, Sc, Sf, uf, seed, ray_base, (float*)t->z_new.p,
                      (float*)t->pass[1].z.p, c->stream);
    return forward_pass(c, t, 1, df, o, d, depth);
}

// the cotangents of render()'s outputs beside rgb (nerf_render_grads), on the device; null = zero
struct OutputGrads {
    const float *d_depth = nullptr, *d_weights = nullptr, *d_z = nullptr;
};

// The backward half's buffers: the common workspace, dL/dz of the new and of the merged depths, the sampler-only coarse
// pass's zero d_rgb and, under mixed_float16, the scaled d_rgb and the gradients an accumulating call adds to.
int ensure_render_bwd(nerf_ctx* c, TrainState* t, const PassDims& dc, const PassDims& df, bool fine, bool accumulate,
                      bool fold_w = false) {      // fold_w: a depth or weights cotangent needs the last pass's folded dL/dw
    const size_t f = sizeof(float);
    const long long N = dc.N;
    int r = ensure_bwd_workspace(c, t, fine ? df.Mp : dc.Mp, dc.M);
    if (fold_w) r |= ensure(c, t->g_wfold, (fine ? df.M : dc.M) * f);
    r |= ensure(c, t->d_zf, (fine ? N * (long long)(df.S - dc.S) : 1) * f);
    r |= ensure(c, t->d_zm, (fine ? df.M : 1) * f);
    r |= ensure(c, t->zero_rgb, N * 3 * f);
    if (t->mixed) {
        r |= ensure(c, t->d_rgb, N * 3 * f);
        if (accumulate)
            for (int w = 0; w < 2; ++w)
                if (t->net[w].present) r |= ensure(c, t->gsave[w], t->nblob * f);
    }
    return r;
}

// The backward half, on what render_forward_core left in TrainState::pass / z_new; dr: the caller's d_rgb on the device
// (null: zero); x: the cotangents of the last pass's other outputs (nerf_train_render_backward_outputs), all null otherwise.
// Runs under a SlotLease (which clears acc_grads on the way out).
int render_backward_core(nerf_ctx* c, TrainState* t, const PassDims& dc, const PassDims& df, bool fine, const float* o,
                         const float* d, const float* uf, uint64_t seed, long long ray_base, const float* dr,
                         bool accumulate, const OutputGrads& x = OutputGrads(), const RayGrads& rays = RayGrads()) {
    const size_t f = sizeof(float);
    const long long N = dc.N;
    const int Sc = dc.S, Sf = df.S - dc.S;
    const bool through_sampler = fine && t->cfg.sampler_gradient != 0;
    // the ray gradients of this call: stored, never accumulated; every pass below that runs adds its share
    if (rays.d_o) HIP_OK(hipMemsetAsync(rays.d_o, 0, N * 4 * f, c->stream));
    if (rays.d_d) HIP_OK(hipMemsetAsync(rays.d_d, 0, N * 4 * f, c->stream));
    // the networks this call computes gradients for: the fine one through its merged pass, the coarse one through the
    // sampler (or, without a fine network, through its own rgb)
    const bool computes[2] = {!fine || through_sampler, fine};
    if (t->mixed) {
        // mixed_float16 (src/ExecutionRun.py:220-221; DietNeRF scales the SUM of ray loss and consistency loss and unscales
        // once, src/DietNeRF.py:142-153,192-202): the caller's d_rgb is multiplied by the current loss scale on the device,
        // the single-pass chain runs on it (fp16 gradient buffers carrying the scale), and the result is UNSCALED and tested
        // before it is stored or, with accumulate, added to the unscaled gradients nerf_train_gradients left -- like with like.
        // The finiteness flag is reset only when this call starts a new gradient computation (accumulate = 0), so with
        // accumulate = 1 it collects over both calls and nerf_train_apply takes the one verdict.
        OptState* st = (OptState*)t->opt.p;
        if (!accumulate) launch_opt_begin(st, c->stream);
        if (dr) {
            launch_scale_by_loss_scale(dr, N * 3, st, (float*)t->d_rgb.p, c->stream);
            dr = (const float*)t->d_rgb.p;
        }
        if (accumulate)
            for (int w = 0; w < 2; ++w)
                if (computes[w] && t->net[w].present)
                    HIP_OK(hipMemcpyAsync(t->gsave[w].p, t->net[w].grad, t->nblob * f, hipMemcpyDeviceToDevice, c->stream));
    }
    t->acc_grads = accumulate && !t->mixed;      // (mixed: the scaled result overwrites, the addition happens after unscaling)

    if (!dr) {      // no colour term: the zero buffer the sampler-only coarse pass has
        HIP_OK(hipMemsetAsync(t->zero_rgb.p, 0, N * 3 * f, c->stream));
        dr = (const float*)t->zero_rgb.p;
    }
    // the depth / weights cotangents of the last pass, folded into its dL/dw (carrying the loss scale like dr)
    const TPass& pl = t->pass[fine ? 1 : 0];
    const PassDims& dl = fine ? df : dc;
    const float* g_w = nullptr;
    if (x.d_depth || x.d_weights) {
        launch_render_output_fold((const float*)pl.w.p, (const float*)pl.z.p, dl.N, dl.S, x.d_depth, x.d_weights, nullptr,
                                  (const OptState*)t->opt.p, (float*)t->g_wfold.p, nullptr, false, c->stream);
        g_w = (const float*)t->g_wfold.p;
    }

    const TPass& pc = t->pass[0];
    if (!fine) {
        if (int q = composite_backward_pass(c, t, 0, dc, o, d, dr, g_w, nullptr, rays)) return q;     // (its depths are data)
    } else {
        float* d_zm = through_sampler ? (float*)t->d_zm.p : nullptr;
        if (int q = composite_backward_pass(c, t, 1, df, o, d, dr, g_w, d_zm, rays)) return q;
        // the depths' own cotangents join the pass's d_z AFTER the compositing backward, which stores there (as the
        // distortion loss's dL/dz does in gradients_impl); only the sampler consumes them
        if (d_zm && (x.d_depth || x.d_z))
            launch_render_output_fold((const float*)pl.w.p, (const float*)pl.z.p, dl.N, dl.S, x.d_depth, nullptr, x.d_z,
                                      (const OptState*)t->opt.p, nullptr, d_zm, true, c->stream);
        if (through_sampler) {
            launch_unmerge_grad((const float*)t->z_new.p, (const float*)pc.z.p, d_zm, N, Sc, Sf, (float*)t->d_zf.p,
                                c->stream);
            launch_sample_pdf_bwd((const float*)pc.w.p, (const float*)pc.z.p, N, Sc, Sf, uf, seed, ray_base,
                                  (const float*)t->d_zf.p, (float*)t->d_wext.p, c->stream);
            // the coarse network: no direct rgb term, only dL/d(weights_coarse) from the sampler
            HIP_OK(hipMemsetAsync(t->zero_rgb.p, 0, N * 3 * f, c->stream));
            if (int q = composite_backward_pass(c, t, 0, dc, o, d, (const float*)t->zero_rgb.p, (const float*)t->d_wext.p,
                                                nullptr, rays))
                return q;
        } else if (!accumulate) {
            HIP_OK(hipMemsetAsync(t->net[0].grad, 0, t->nblob * f, c->stream));   // render() does not depend on it
        }
    }
    if (int q = join_side(c, t)) return q;
    if (t->mixed) {
        float* g[2]; const float* add[2]; int n = 0;
        for (int w = 0; w < 2; ++w)
            if (computes[w] && t->net[w].present) {
                g[n] = t->net[w].grad;
                add[n] = accumulate ? (const float*)t->gsave[w].p : nullptr;
                ++n;
            }
        launch_unscale_check(g[0], n > 1 ? g[1] : nullptr, t->nblob, (OptState*)t->opt.p, c->stream, false, add[0],
                             n > 1 ? add[1] : nullptr);
    }
    HIP_OK(hipGetLastError());
    return 0;
}

// ---- the same graph in two calls, with the activations kept in between (RenderSlot) -------------------------------------
static void swap_grad_members(TPass& a, TPass& b) {
    for (int l = 0; l < 10; ++l) std::swap(a.D[l], b.D[l]);
    std::swap(a.dxa, b.dxa);
    std::swap(a.dxb, b.dxb);
    std::swap(a.rs, b.rs);
}
// the slot's stash becomes TrainState::pass (which forward_pass / the backward passes work on), keeping the working gradient buffers
static void slot_swap_in(TrainState* t, RenderSlot& s) {
    for (int w = 0; w < 2; ++w) {
        std::swap(t->pass[w], s.pass[w]);
        swap_grad_members(t->pass[w], s.pass[w]);
    }
    std::swap(t->z_new, s.z_new);
}
static void slot_swap_out(TrainState* t, RenderSlot& s) {
    for (int w = 0; w < 2; ++w) {
        swap_grad_members(t->pass[w], s.pass[w]);
        std::swap(t->pass[w], s.pass[w]);
    }
    std::swap(t->z_new, s.z_new);
}

// The scope of one call through the render graph, left on every path (HIP_OK returns included): acc_grads does not outlive
// it, and a slot's stash is TrainState::pass for exactly its duration.  The slot takes its stash back only after the side
// stream has joined (the fine pass's batched weight-gradient launch reads it).
struct SlotLease {
    nerf_ctx* c;
    TrainState* t;
    RenderSlot* s;
    SlotLease(nerf_ctx* c_, TrainState* t_, RenderSlot* s_ = nullptr) : c(c_), t(t_), s(s_) {
        if (s) slot_swap_in(t, *s);
    }
    ~SlotLease() {
        if (s) {
            (void)join_side(c, t);
            slot_swap_out(t, *s);
        }
        t->acc_grads = false;
    }
    SlotLease(const SlotLease&) = delete;
    SlotLease& operator=(const SlotLease&) = delete;
};

int render_gradients_impl(nerf_ctx* c, const float* rays_o, const float* rays_d, const float* d_rgb_in, int64_t N, int Sc,
                          int Sf, const float* u_c, const float* u_f, uint64_t seed, int64_t ray_base, bool accumulate,
                          int mem) {
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (!rays_o || !rays_d || !d_rgb_in) return fail("NULL argument");
    bool fine;
    if (int r = check_samples(t, N, Sc, Sf, &fine)) return r;
    const size_t f = sizeof(float);
    Staging st(c, mem);
    const float* o = st.in(t->o, rays_o, N * 4 * f);
    const float* d = st.in(t->d, rays_d, N * 4 * f);
    const float* dr = st.in(t->tgt, d_rgb_in, N * 3 * f);
    const float* uc = st.in(t->u_c, u_c, (size_t)N * Sc * f);
    const float* uf = st.in(t->u_f, fine ? u_f : nullptr, (size_t)N * (fine ? Sf : 0) * f);
    if (st.err) return st.err;
    const PassDims dc = pass_dims(N, Sc), df = pass_dims(N, Sc + Sf);
    if (int r = ensure_render_bwd(c, t, dc, df, fine, accumulate)) return r;
    SlotLease lease(c, t);                        // (no slot: the activations stay in TrainState::pass)
    if (int r = render_forward_core(c, t, dc, df, fine, o, d, uc, uf, seed, ray_base)) return r;
    return render_backward_core(c, t, dc, df, fine, o, d, uf, seed, ray_base, dr, accumulate);
}

int render_forward_impl(nerf_ctx* c, int slot, const float* rays_o, const float* rays_d, int64_t N, int Sc, int Sf,
                        const float* u_c, const float* u_f, uint64_t seed, int64_t ray_base, int mem,
                        bool want_depth = false) {    // want_depth: the last pass's depth sum -> TrainState::depth
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (!rays_o || !rays_d) return fail("NULL argument");
    if (slot < 0 || slot >= kMaxRenderSlots) return fail("slot %d out of range (0..%d)", slot, kMaxRenderSlots - 1);
    bool fine;
    if (int r = check_samples(t, N, Sc, Sf, &fine)) return r;
    if (want_depth) if (int r = ensure(c, t->depth, N * sizeof(float))) return r;
    if ((size_t)slot >= t->slots.size()) t->slots.resize((size_t)slot + 1);
    RenderSlot& s = t->slots[slot];
    s.valid = false;
    const size_t f = sizeof(float);
    // the slot keeps its own copies of the rays and draws: the caller's buffers need not outlive this call
    auto keep = [&](DevBuf& b, const float* src, size_t bytes) -> int {
        if (int r = ensure(c, b, bytes)) return r;
        return copy_from_caller(c, b.p, src, bytes, mem);
    };
    if (int r = keep(s.o, rays_o, N * 4 * f)) return r;
    if (int r = keep(s.d, rays_d, N * 4 * f)) return r;
    s.has_uc = u_c != nullptr;
    s.has_uf = fine && u_f != nullptr;
    if (s.has_uc) if (int r = keep(s.u_c, u_c, (size_t)N * Sc * f)) return r;
    if (s.has_uf) if (int r = keep(s.u_f, u_f, (size_t)N * Sf * f)) return r;
    const float* uc = s.has_uc ? (const float*)s.u_c.p : nullptr;
    const float* uf = s.has_uf ? (const float*)s.u_f.p : nullptr;
    SlotLease lease(c, t, &s);
    if (int r = render_forward_core(c, t, pass_dims(N, Sc), pass_dims(N, Sc + Sf), fine, (const float*)s.o.p,
                                    (const float*)s.d.p, uc, uf, seed, ray_base, want_depth ? (float*)t->depth.p : nullptr))
        return r;
    s.N = N; s.Sc = Sc; s.Sf = fine ? Sf : 0; s.seed = seed; s.ray_base = ray_base;
    s.valid = true;
    return 0;
}

// g: the caller's cotangents (nerf_render_grads; at least one is set).  nerf_train_render_backward passes d_rgb alone.
// d_rays_orig, d_rays_dirs: the caller's (N, 4) ray-gradient outputs (nerf_train_render_backward_rays), null otherwise.
int render_backward_impl(nerf_ctx* c, int slot, const nerf_render_grads& g, bool accumulate, int mem,
                         float* d_rays_orig = nullptr, float* d_rays_dirs = nullptr) {
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (slot < 0 || (size_t)slot >= t->slots.size() || !t->slots[slot].valid)
        return fail("slot %d holds no forward pass (nerf_train_render_forward first; a backward pass consumes it, and so does "
                    "an optimizer step)", slot);
    RenderSlot& s = t->slots[slot];
    const bool fine = s.Sf > 0;
    const PassDims dc = pass_dims(s.N, s.Sc), df = pass_dims(s.N, s.Sc + s.Sf);
    const size_t ns = (size_t)(fine ? df.M : dc.M) * sizeof(float);
    Staging st(c, mem);
    const float* dr = st.in(t->tgt, g.d_rgb, s.N * 3 * sizeof(float));
    OutputGrads x;
    x.d_depth = st.in(t->in_dd, g.d_depth, s.N * sizeof(float));
    x.d_weights = st.in(t->in_dw, g.d_weights, ns);
    x.d_z = st.in(t->in_dz, g.d_z, ns);
    RayGrads rays;
    rays.d_o = st.out(t->out_ro, d_rays_orig, s.N * 4 * sizeof(float));
    rays.d_d = st.out(t->out_rd, d_rays_dirs, s.N * 4 * sizeof(float));
    if (st.err) return st.err;
    if (int r = ensure_render_bwd(c, t, dc, df, fine, accumulate, x.d_depth || x.d_weights)) return r;
    s.valid = false;                              // consumed, whatever happens below
    SlotLease lease(c, t, &s);
    if (int r = render_backward_core(c, t, dc, df, fine, (const float*)s.o.p, (const float*)s.d.p,
                                     s.has_uf ? (const float*)s.u_f.p : nullptr, s.seed, s.ray_base, dr, accumulate, x, rays))
        return r;
    return rays.any() ? st.finish() : 0;      // (a host caller's ray gradients leave here; the blobs leave through copy_out)
}

// The outputs of a gradient / render call, each only if the caller asks for it: rgb (N x 3) and the two gradient blobs,
// device -> host or device -> device by `mem`, synchronous for a host caller.  grad_fine needs the call's fine pass (Sf > 0
// samples and a fine network); without one it fails after the copies before it are enqueued.
int copy_out(nerf_ctx* c, int mem, int Sf, float* grad_coarse, float* grad_fine, float* rgb_out = nullptr,
             const void* rgb = nullptr, long long N = 0) {
    const TrainState* t = c->train;
    const size_t nb = t->nblob * sizeof(float);
    if (rgb_out) if (int r = copy_to_caller(c, rgb_out, rgb, N * 3 * sizeof(float), mem)) return r;
    if (grad_coarse) if (int r = copy_to_caller(c, grad_coarse, t->net[0].grad, nb, mem)) return r;
    if (grad_fine) {
        if (!(Sf > 0 && t->net[1].present)) return fail("grad_fine requested but no fine pass ran (Sf = %d)", Sf);
        if (int r = copy_to_caller(c, grad_fine, t->net[1].grad, nb, mem)) return r;
    }
    if (mem == NERF_MEM_HOST) HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int read_metrics(nerf_ctx* c, bool fine, float* metrics) {
    if (!metrics) return 0;
    float h[2] = {0.f, 0.f};
    HIP_OK(hipMemcpyAsync(h, c->train->scal.p, 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    const float* lw = c->train->loss_w;                                // (1, 1: the products are exact)
    metrics[0] = fine ? lw[0] * h[0] + lw[1] * h[1] : lw[0] * h[0];    // src/NeRF.py:151,157
    metrics[1] = (float)(-10.0 * log10((double)h[0]));                  // get_psnr, UtilsNeuralRadianceField.py:123-132
    metrics[2] = fine ? (float)(-10.0 * log10((double)h[1])) : 0.f;
    return 0;
}

int apply_impl(nerf_ctx* c) {
    // Adam (gated on the device by the latest verdict: a dropped step leaves weights, moments and the iteration count
    // alone), then the training matrices are re-laid out from the blob either way
    TrainState* t = c->train;
    OptState* st = (OptState*)t->opt.p;
    for (RenderSlot& sl : t->slots) sl.valid = false;      // kept activations belong to the weights that made them
    for (int w = 0; w < 2; ++w) {
        TNet& n = t->net[w];
        if (!n.present) continue;
        launch_adam(n.blob, n.m, n.v, n.grad, t->nblob, t->cfg.learning_rate, t->cfg.beta_1, t->cfg.beta_2, t->cfg.epsilon,
                    st, c->stream);
        if (int r = relayout_net(c, n)) return r;
        n.render_dirty = true;
    }
    launch_opt_tick(st, t->cfg.beta_1, t->cfg.beta_2, c->stream);
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace

namespace nerf {

void train_free(nerf_ctx* c) {
    TrainState* t = c->train;
    if (!t) return;
    for (auto& n : t->net) {
        if (n.blob) (void)hipFree(n.blob);
        if (n.grad) (void)hipFree(n.grad);
        if (n.m) (void)hipFree(n.m);
        if (n.v) (void)hipFree(n.v);
        if (n.mats) (void)hipFree(n.mats);
        if (n.fstream) (void)hipFree(n.fstream);
        if (n.fcst) (void)hipFree(n.fcst);
        if (n.bstream) (void)hipFree(n.bstream);
    }
    for (int32_t* bi : t->bidx) if (bi) (void)hipFree(bi);
    for (TPass& p : t->pass) free_pass(p);
    for (RenderSlot& sl : t->slots) free_slot(sl);
    if (t->side) { (void)hipStreamSynchronize(t->side); (void)hipStreamDestroy(t->side); }
    if (t->ev_fork) (void)hipEventDestroy(t->ev_fork);
    if (t->ev_join) (void)hipEventDestroy(t->ev_join);
    free_buf(t->partial_side);
    DevBuf* bs[] = {&t->Gc, &t->Ga, &t->Gb, &t->G9, &t->Graw, &t->dsig, &t->dA0, &t->partial, &t->d_rgb, &t->d_wext, &t->d_zf, &t->tgt,
                    &t->o, &t->d, &t->u_c, &t->u_f, &t->scal, &t->gmax, &t->z_new, &t->d_zm, &t->zero_rgb, &t->opt,
                    &t->gsave[0], &t->gsave[1], &t->macc, &t->d_wdist, &t->dist_ray, &t->dacc, &t->depth, &t->g_wfold, &t->in_dd,
                    &t->in_dw, &t->in_dz, &t->out_ro, &t->out_rd};
    for (DevBuf* b : bs) free_buf(*b);
    delete t;
    c->train = nullptr;
}

int train_window_guard(nerf_ctx* c) {
    TrainState* t = c->train;
    if (!t) return 0;
    // A slot's backward pass runs on the trainer's backward streams and scales its weight gradients by the table of the day:
    // both must be the ones its forward pass ran under.  The rule is the simple one: no change while a pass is held.
    for (size_t s = 0; s < t->slots.size(); ++s)
        if (t->slots[s].valid)
            return fail("the encoding window cannot change while render slot %zu holds a forward pass: run its "
                        "nerf_train_render_backward first (an optimizer step or nerf_train_render_release drops it)", s);
    return join_side(c, t);      // the side stream's gradient reduction reads the scale table the caller is about to overwrite
}

int train_on_window(nerf_ctx* c) {
    TrainState* t = c->train;
    if (!t) return 0;
    for (TNet& n : t->net)
        if (n.present) if (int r = relayout_net(c, n)) return r;
    return 0;
}

const float* train_master_blob(const nerf_ctx* c, int which) {
    return c->train && c->train->net[which].present ? c->train->net[which].blob : nullptr;
}

int train_on_load(nerf_ctx* c, int which) {
    TrainState* t = c->train;
    if (!t) return 0;
    TNet& n = t->net[which];
    if (!n.present) return init_net(c, t, which);
    HIP_OK(hipMemcpyAsync(n.blob, c->net[which].host_blob.data(), t->nblob * sizeof(float), hipMemcpyHostToDevice,
                          c->stream));
    n.render_dirty = n.host_stale = false;
    return relayout_net(c, n);
}

// The render path's view of a network that is being trained.  After optimizer steps its operand streams are
// re-packed from the trained blob on the device (enqueued on the ctx stream: a render between steps does not synchronise);
// to_host additionally brings NetWeights::host_blob up to date (nerf_train_end, a restarting nerf_train_begin: the next
// trainer starts from it).
int train_flush_weights(nerf_ctx* c, int which, bool to_host) {
    TrainState* t = c->train;
    if (!t || !t->net[which].present) return 0;
    TNet& n = t->net[which];
    NetWeights& nw = c->net[which];
    if (n.render_dirty) {
        if (int r = repack_render_streams(c, which, n.blob)) return r;
        n.render_dirty = false;
        n.host_stale = true;
    }
    if (to_host && n.host_stale) {
        HIP_OK(hipMemcpyAsync(nw.host_blob.data(), n.blob, t->nblob * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
        n.host_stale = false;
    }
    return 0;
}

}  // namespace nerf

extern "C" {

int nerf_train_begin(nerf_ctx* c, const nerf_train_config* cfg) {
    ENTER(c);
    if (!cfg) return fail("nerf_train_config is NULL");
    if (!(cfg->learning_rate > 0.f)) return fail("learning_rate must be positive");
    if (!c->net[0].loaded) return fail("load the coarse network's weights before nerf_train_begin");
    if (c->train) {
        // a trainer restarted without nerf_train_end goes on from the TRAINED weights ("the weights currently loaded")
        for (int w = 0; w < 2; ++w)
            if (int r = train_flush_weights(c, w, true)) return r;
        train_free(c);
    }
    TrainState* t = new TrainState();
    t->nblob = nerf_blob_size(&c->cfg);
    c->train = t;
    t->cfg = *cfg;
    t->loss_w[0] = t->loss_w[1] = 1.f;
    t->dist_w[0] = t->dist_w[1] = 0.f;
    t->mixed = cfg->mixed_float16 != 0;
    {
        OptState h{};
        h.scale = t->mixed ? (cfg->initial_loss_scale > 0.f ? cfg->initial_loss_scale : 32768.f) : 1.f;
        h.inv_scale = 1.0f / h.scale;
        h.adam_corr = (float)(sqrt(1.0 - (double)cfg->beta_2) / (1.0 - (double)cfg->beta_1));      // t = 1
        h.finite = 1; h.apply_ok = 1; h.good = 0;
        h.growth = cfg->dynamic_growth_steps > 0 ? cfg->dynamic_growth_steps : 2000;
        h.dynamic = t->mixed ? 1 : 0;
        h.iterations = 0; h.skipped = 0;
        if (int r = ensure(c, t->opt, sizeof(OptState))) { train_free(c); return r; }
        HIP_OK(hipMemcpy(t->opt.p, &h, sizeof(OptState), hipMemcpyHostToDevice));
    }
    // the fused trainer unless NERF_TRAIN_FORWARD=gemm asks for the layer-wise exact-fp32 one (TrainState::reference)
    const char* fw = getenv("NERF_TRAIN_FORWARD");
    t->reference = fw && strcmp(fw, "gemm") == 0;
    // the fine pass's batched weight-gradient launch on a second stream (see TrainState::overlap) unless NERF_TRAIN_OVERLAP=0
    const char* ov = getenv("NERF_TRAIN_OVERLAP");
    t->overlap = !(ov && strcmp(ov, "0") == 0);
    if (t->mixed && t->reference) {
        train_free(c);
        return fail("mixed_float16 training runs on the fused trainer only: unset NERF_TRAIN_FORWARD");
    }
    for (int w = 0; w < 2; ++w)
        if (c->net[w].loaded)
            if (int r = init_net(c, t, w)) { train_free(c); return r; }
    return 0;
}

int nerf_train_end(nerf_ctx* c) {
    ENTER(c);
    for (int w = 0; w < 2; ++w)
        if (int r = train_flush_weights(c, w, true)) return r;
    HIP_OK(hipStreamSynchronize(c->stream));
    train_free(c);
    return 0;
}

int nerf_train_loss_scale(nerf_ctx* c, float* loss_scale, int64_t* steps_applied, int64_t* steps_skipped) {
    if (!c || !c->train) return fail("nerf_train_begin has not been called");
    OptState h;
    HIP_OK(hipMemcpyAsync(&h, c->train->opt.p, sizeof(OptState), hipMemcpyDeviceToHost, c->stream));
    HIP_OK(hipStreamSynchronize(c->stream));
    if (loss_scale) *loss_scale = h.scale;
    if (steps_applied) *steps_applied = h.iterations;
    if (steps_skipped) *steps_skipped = h.skipped;
    return 0;
}

int nerf_train_read_metric_sums(nerf_ctx* c, double* sums, int64_t* steps) {
    ENTER(c);
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    double h[4] = {0, 0, 0, 0};
    if (t->macc.p) {
        HIP_OK(hipMemcpyAsync(h, t->macc.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemsetAsync(t->macc.p, 0, sizeof h, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    if (sums) { sums[0] = h[0]; sums[1] = h[1]; sums[2] = h[2]; }
    if (steps) *steps = (int64_t)h[3];
    return 0;
}

int nerf_train_set_learning_rate(nerf_ctx* c, float lr) {
    if (!c || !c->train) return fail("nerf_train_begin has not been called");
    if (!(lr > 0.f)) return fail("learning_rate must be positive");
    c->train->cfg.learning_rate = lr;
    return 0;
}

int nerf_train_set_loss_weights(nerf_ctx* c, float coarse_mse_weight, float fine_mse_weight) {
    if (!c || !c->train) return fail("nerf_train_begin has not been called");
    if (!(coarse_mse_weight >= 0.f) || !(fine_mse_weight >= 0.f) || !(coarse_mse_weight <= 3.0e38f) ||
        !(fine_mse_weight <= 3.0e38f))
        return fail("loss weights must be finite and non-negative (got %g, %g)", coarse_mse_weight, fine_mse_weight);
    c->train->loss_w[0] = coarse_mse_weight;
    c->train->loss_w[1] = fine_mse_weight;
    return 0;
}

int nerf_train_set_distortion_weights(nerf_ctx* c, float coarse, float fine) {
    if (!c || !c->train) return fail("nerf_train_begin has not been called");
    if (!(coarse >= 0.f) || !(coarse <= 3.0e38f))
        return fail("distortion weight `coarse` must be finite and non-negative (got %g)", coarse);
    if (!(fine >= 0.f) || !(fine <= 3.0e38f))
        return fail("distortion weight `fine` must be finite and non-negative (got %g)", fine);
    c->train->dist_w[0] = coarse;
    c->train->dist_w[1] = fine;
    return 0;
}

int nerf_train_read_distortion_sums(nerf_ctx* c, double* sums, int64_t* steps) {
    ENTER(c);
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    double h[3] = {0, 0, 0};
    if (t->dacc.p) {
        HIP_OK(hipMemcpyAsync(h, t->dacc.p, sizeof h, hipMemcpyDeviceToHost, c->stream));
        HIP_OK(hipMemsetAsync(t->dacc.p, 0, sizeof h, c->stream));
        HIP_OK(hipStreamSynchronize(c->stream));
    }
    if (sums) { sums[0] = h[0]; sums[1] = h[1]; }
    if (steps) *steps = (int64_t)h[2];
    return 0;
}

int nerf_distortion_loss(nerf_ctx* c, const float* weights, const float* z, int64_t N, int32_t S, float* loss_per_ray,
                         float* d_weights, float* d_z, int mem) {
    ENTER(c);
    if (!weights) return fail("weights is NULL");
    if (!z) return fail("z is NULL");
    if (N < 0) return fail("bad N = %lld (need N >= 0)", (long long)N);
    if (S < 1) return fail("bad S = %d (need S >= 1)", S);
    if (!(c->cfg.far_boundary > c->cfg.near_boundary))
        return fail("the distortion loss needs far_boundary > near_boundary (got %g, %g)", c->cfg.near_boundary,
                    c->cfg.far_boundary);
    const size_t f = sizeof(float);
    Staging st(c, mem);
    const float* dw = st.in(c->b_in0, weights, (size_t)N * S * f);
    const float* dz = st.in(c->b_in1, z, (size_t)N * S * f);
    float* dl = st.out(c->b_in2, loss_per_ray, (size_t)N * f);
    float* gw = st.out(c->b_zc, d_weights, (size_t)N * S * f);
    float* gz = st.out(c->b_zf, d_z, (size_t)N * S * f);
    if (st.err) return st.err;
    launch_distortion(dw, dz, N, S, c->cfg.near_boundary, c->cfg.far_boundary, nullptr, 1.0f, dl, gw, false, gz, false, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_train_gradients(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, const float* target_rgb, int64_t N,
                         int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                         float* grad_coarse, float* grad_fine, float* metrics, int mem) {
    ENTER(c);
    if (int r = gradients_impl(c, rays_orig, rays_dirs, target_rgb, N, Sc, Sf, u_coarse, u_fine, seed, mem)) return r;
    // (mixed_float16: the gradients come back unscaled; the skip-or-apply verdict and the loss-scale move belong to
    // nerf_train_apply, which tests the blobs it is given)
    if (int r = copy_out(c, mem, Sf, grad_coarse, grad_fine)) return r;
    return read_metrics(c, Sf > 0 && c->train->net[1].present, metrics);
}

int nerf_train_render_gradients(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, const float* d_rgb, int64_t N,
                                int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                                int64_t ray_base, int32_t accumulate, float* rgb_out, float* grad_coarse,
                                float* grad_fine, int mem) {
    ENTER(c);
    if (int r = render_gradients_impl(c, rays_orig, rays_dirs, d_rgb, N, Sc, Sf, u_coarse, u_fine, seed, ray_base,
                                      accumulate != 0, mem)) return r;
    const bool fine = Sf > 0 && c->train->net[1].present;
    return copy_out(c, mem, Sf, grad_coarse, grad_fine, rgb_out, c->train->pass[fine ? 1 : 0].rgb.p, N);
}

int nerf_train_render_forward(nerf_ctx* c, int32_t slot, const float* rays_orig, const float* rays_dirs, int64_t N, int32_t Sc,
                              int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed, int64_t ray_base,
                              float* rgb_out, int mem) {
    ENTER(c);
    if (int r = render_forward_impl(c, slot, rays_orig, rays_dirs, N, Sc, Sf, u_coarse, u_fine, seed, ray_base, mem)) return r;
    const RenderSlot& s = c->train->slots[slot];
    return copy_out(c, mem, s.Sf, nullptr, nullptr, rgb_out, s.pass[s.Sf > 0 ? 1 : 0].rgb.p, N);
}

int nerf_train_render_backward(nerf_ctx* c, int32_t slot, const float* d_rgb, int32_t accumulate, float* grad_coarse,
                               float* grad_fine, int mem) {
    ENTER(c);
    const bool fine = c->train && slot >= 0 && (size_t)slot < c->train->slots.size() && c->train->slots[slot].Sf > 0;
    if (grad_fine && !fine) return fail("grad_fine requested but slot %d ran no fine pass", slot);   // (before it is consumed)
    if (c->train && !d_rgb) return fail("NULL argument");
    if (int r = render_backward_impl(c, slot, nerf_render_grads{d_rgb, nullptr, nullptr, nullptr}, accumulate != 0, mem)) return r;
    return copy_out(c, mem, c->train->slots[slot].Sf, grad_coarse, grad_fine);
}

int nerf_train_render_forward_outputs(nerf_ctx* c, int32_t slot, const float* rays_orig, const float* rays_dirs, int64_t N,
                                      int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                                      int64_t ray_base, const nerf_train_outputs* outs, int mem) {
    ENTER(c);
    if (!outs) return fail("nerf_train_outputs is NULL");
    if (int r = render_forward_impl(c, slot, rays_orig, rays_dirs, N, Sc, Sf, u_coarse, u_fine, seed, ray_base, mem,
                                    outs->depth != nullptr)) return r;
    const RenderSlot& s = c->train->slots[slot];
    const TPass& p = s.pass[s.Sf > 0 ? 1 : 0];
    const size_t f = sizeof(float), ns = (size_t)N * (s.Sc + s.Sf) * f;
    if (outs->depth) if (int r = copy_to_caller(c, outs->depth, c->train->depth.p, N * f, mem)) return r;
    if (outs->weights) if (int r = copy_to_caller(c, outs->weights, p.w.p, ns, mem)) return r;
    if (outs->z) if (int r = copy_to_caller(c, outs->z, p.z.p, ns, mem)) return r;
    return copy_out(c, mem, s.Sf, nullptr, nullptr, outs->rgb, p.rgb.p, N);      // (synchronises for a host caller)
}

int nerf_train_render_backward_outputs(nerf_ctx* c, int32_t slot, const nerf_render_grads* g, int32_t accumulate,
                                       float* grad_coarse, float* grad_fine, int mem) {
    ENTER(c);
    if (!g) return fail("nerf_render_grads is NULL");
    if (!g->d_rgb && !g->d_depth && !g->d_weights && !g->d_z)
        return fail("all four cotangents of nerf_render_grads are NULL: nothing to differentiate");
    const bool fine = c->train && slot >= 0 && (size_t)slot < c->train->slots.size() && c->train->slots[slot].Sf > 0;
    if (grad_fine && !fine) return fail("grad_fine requested but slot %d ran no fine pass", slot);   // (before it is consumed)
    if (int r = render_backward_impl(c, slot, *g, accumulate != 0, mem)) return r;
    return copy_out(c, mem, c->train->slots[slot].Sf, grad_coarse, grad_fine);
}

int nerf_train_set_ray_gradients(nerf_ctx* c, int32_t on) {
    ENTER(c);
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (on && t->reference)
        return fail("ray gradients run on the fused trainer only: unset NERF_TRAIN_FORWARD");
    if (t->ray_grads == (on != 0)) return 0;
    t->ray_grads = on != 0;
    // the encoding tiles are a property of how a network's backward stream is packed: re-pack both from the master weights
    // (the kept activations of the slots do not depend on it)
    for (int w = 0; w < 2; ++w) {
        TNet& n = t->net[w];
        if (!n.present) continue;
        if (int r = ensure_fused(c, t, n)) return r;
        if (int r = relayout_net(c, n)) return r;
    }
    return 0;
}

int nerf_train_render_backward_rays(nerf_ctx* c, int32_t slot, const nerf_render_grads* g, int32_t accumulate, float* grad_coarse,
                                    float* grad_fine, float* d_rays_orig, float* d_rays_dirs, int mem) {
    ENTER(c);
    if (!g) return fail("nerf_render_grads is NULL");
    if (!g->d_rgb && !g->d_depth && !g->d_weights && !g->d_z)
        return fail("all four cotangents of nerf_render_grads are NULL: nothing to differentiate");
    if (c->train && !c->train->ray_grads)
        return fail("ray gradients are switched off: call nerf_train_set_ray_gradients(ctx, 1) first");
    const bool fine = c->train && slot >= 0 && (size_t)slot < c->train->slots.size() && c->train->slots[slot].Sf > 0;
    if (grad_fine && !fine) return fail("grad_fine requested but slot %d ran no fine pass", slot);   // (before it is consumed)
    if (int r = render_backward_impl(c, slot, *g, accumulate != 0, mem, d_rays_orig, d_rays_dirs)) return r;
    return copy_out(c, mem, c->train->slots[slot].Sf, grad_coarse, grad_fine);
}

int nerf_ray_position_grads(nerf_ctx* c, const float* d_points, const float* z, int64_t N, int32_t S, float* d_rays_orig,
                            float* d_rays_dirs, int mem) {
    ENTER(c);
    if (!d_points) return fail("d_points is NULL");
    if (!z) return fail("z is NULL");
    if (N < 0) return fail("bad N = %lld (need N >= 0)", (long long)N);
    if (S < 1) return fail("bad S = %d (need S >= 1)", S);
    const size_t f = sizeof(float);
    Staging st(c, mem);
    const float* dp = st.in(c->b_in0, d_points, (size_t)N * S * 3 * f);
    const float* zz = st.in(c->b_in1, z, (size_t)N * S * f);
    float* go = st.out(c->b_out[0], d_rays_orig, (size_t)N * 4 * f);
    float* gd = st.out(c->b_out[1], d_rays_dirs, (size_t)N * 4 * f);
    if (st.err) return st.err;
    if (go && N > 0) HIP_OK(hipMemsetAsync(go, 0, (size_t)N * 4 * f, c->stream));
    if (gd && N > 0) HIP_OK(hipMemsetAsync(gd, 0, (size_t)N * 4 * f, c->stream));
    launch_ray_position_reduce(dp, zz, N, S, go, gd, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_render_output_grads(nerf_ctx* c, const float* weights, const float* z, int64_t N, int32_t S, const float* d_depth,
                             const float* d_weights, const float* d_z, float* g_w, float* g_z, int mem) {
    ENTER(c);
    if (!weights) return fail("weights is NULL");
    if (!z) return fail("z is NULL");
    if (N < 0) return fail("bad N = %lld (need N >= 0)", (long long)N);
    if (S < 1) return fail("bad S = %d (need S >= 1)", S);
    const size_t f = sizeof(float), ns = (size_t)N * S * f;
    Staging st(c, mem);
    const float* w = st.in(c->b_in0, weights, ns);
    const float* zz = st.in(c->b_in1, z, ns);
    const float* dd = st.in(c->b_in2, d_depth, (size_t)N * f);
    const float* dw = st.in(c->b_zc, d_weights, ns);
    const float* dz = st.in(c->b_zf, d_z, ns);
    float* gw = st.out(c->b_out[0], g_w, ns);
    float* gz = st.out(c->b_out[1], g_z, ns);
    if (st.err) return st.err;
    launch_render_output_fold(w, zz, N, S, dd, dw, dz, nullptr, gw, gz, false, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_train_render_release(nerf_ctx* c) {
    ENTER(c);
    TrainState* t = c->train;
    if (!t) return 0;
    HIP_OK(hipStreamSynchronize(c->stream));
    if (t->side) HIP_OK(hipStreamSynchronize(t->side));
    for (RenderSlot& sl : t->slots) free_slot(sl);
    t->slots.clear();
    (void)hipGetLastError();      // (a failed allocation while filling slots is what usually brings a caller here: start clean)
    return 0;
}

int nerf_train_apply(nerf_ctx* c, const float* grad_coarse, const float* grad_fine, int mem) {
    ENTER(c);
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (grad_coarse) if (int r = copy_from_caller(c, t->net[0].grad, grad_coarse, t->nblob * sizeof(float), mem)) return r;
    if (grad_fine) {
        if (!t->net[1].present) return fail("grad_fine given but no fine network is loaded");
        if (int r = copy_from_caller(c, t->net[1].grad, grad_fine, t->nblob * sizeof(float), mem)) return r;
    }
    if (mem == NERF_MEM_HOST && (grad_coarse || grad_fine)) HIP_OK(hipStreamSynchronize(c->stream));
    // LossScaleOptimizer.apply_gradients: test what is about to be applied (the caller's all-reduced blobs, or the ctx's
    // own after nerf_train_gradients [+ nerf_train_render_gradients]); a non-finite step is skipped on the device
    take_verdict(c, true);
    return apply_impl(c);
}

int nerf_train_step(nerf_ctx* c, const float* rays_orig, const float* rays_dirs, const float* target_rgb, int64_t N,
                    int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed, float* metrics,
                    int mem) {
    ENTER(c);
    if (int r = gradients_impl(c, rays_orig, rays_dirs, target_rgb, N, Sc, Sf, u_coarse, u_fine, seed, mem)) return r;
    const bool fine = Sf > 0 && c->train->net[1].present;
    // data-parallel: with a communicator (nerf_comm_init) every rank passes its shard of the batch and the gradient
    // blobs are averaged here, one all-reduce each, before the identical Adam update
    for (int w = 0; w < 2; ++w)
        if (c->train->net[w].present)
            if (int r = comm_allreduce_mean(c, c->train->net[w].grad, c->train->nblob)) return r;
    // a non-finite shard gradient makes the all-reduced blob non-finite on EVERY rank: the finiteness test is repeated on
    // the reduced blobs so that all ranks reach the same verdict (drop the step, halve the scale) by themselves
    // (repeated whenever the ctx has a communicator, one rank included: one small kernel)
    take_verdict(c, c->comm != nullptr);
    if (int r = apply_impl(c)) return r;                 // gated on the device by the verdict
    return read_metrics(c, fine, metrics);
}

int nerf_train_get_gradients(nerf_ctx* c, int which, float* blob, size_t n_floats, int mem) {
    ENTER(c);
    TrainState* t = c->train;
    if (!t) return fail("nerf_train_begin has not been called");
    if (!blob) return fail("blob is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail("which must be 0 (coarse) or 1 (fine)");
    if (!t->net[which].present) return fail("network %d has no weights loaded", which);
    if (n_floats != t->nblob) return fail("gradient blob has %zu floats, expected %zu", n_floats, t->nblob);
    if (int r = copy_to_caller(c, blob, t->net[which].grad, t->nblob * sizeof(float), mem)) return r;
    if (mem == NERF_MEM_HOST) HIP_OK(hipStreamSynchronize(c->stream));
    return 0;
}

int nerf_get_weights(nerf_ctx* c, int which, float* blob, size_t n_floats, int mem) {
    ENTER(c);
    if (!blob) return fail("blob is NULL");
    if (which != NERF_NET_COARSE && which != NERF_NET_FINE) return fail("which must be 0 (coarse) or 1 (fine)");
    if (!c->net[which].loaded) return fail("network %d has no weights loaded", which);
    const size_t want = nerf_blob_size(&c->cfg);
    if (n_floats != want) return fail("weight blob has %zu floats, expected %zu", n_floats, want);
    TrainState* t = c->train;
    if (t && t->net[which].present) {
        if (int r = copy_to_caller(c, blob, t->net[which].blob, want * sizeof(float), mem)) return r;
        HIP_OK(hipStreamSynchronize(c->stream));
        return 0;
    }
    const hipMemcpyKind kind = mem == NERF_MEM_DEVICE ? hipMemcpyHostToDevice : hipMemcpyHostToHost;
    HIP_OK(hipMemcpy(blob, c->net[which].host_blob.data(), want * sizeof(float), kind));
    return 0;
}

}  // extern "C"
