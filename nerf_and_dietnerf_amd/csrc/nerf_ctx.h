// nerf_ctx.h -- the context object behind the C ABI, shared by every unit with entry points: nerf_api.hip (render path), field_api.hip
// (field queries), train_api.hip (training path), mesh_kernels.hip, volume_kernels.hip.  Internal: not part of include/nerf_mi355.h.
#pragma once
#include "../../include/nerf_mi355.h"

#include <string>
#include <utility>
#include <vector>

#include "nerf_kernels.h"

namespace nerf {

int fail(const char* fmt, ...);   // sets the thread-local message of nerf_last_error(), returns 1

#define HIP_OK(expr)                                                                                    \
    do {                                                                                                \
        hipError_t e__ = (expr);                                                                        \
        if (e__ != hipSuccess) return nerf::fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                                                 __FILE__, __LINE__);                                   \
    } while (0)

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct NetWeights {
    void* stream[kStreamKinds] = {};   // the operand streams render_streams() lists for this network (null: not kept)
    float* cst[kConstBlocks] = {};     // kConstBytes each
    bool loaded = false;
    std::vector<float> host_blob;   // last blob handed to nerf_load_weights (Keras order): seed of the trainer
    float* dev_blob = nullptr;      // ... and its copy on the device, which nerf_load_weights re-packs the streams from
};

// The record of one culled pass (cull_kernels.hip): verdict bits, the scan's slot per mask byte (both grow-only), the row count.
// The render path keeps one on the ctx, the trainer one per TPass: a slot's backward pass reads it long after its forward pass.
struct SampleCompaction { DevBuf mask, first; long long rows = -1; };   // rows < 0: no compaction, every sample ran

// Per-launch gate of the rgb-skipping f16x3 kernel (mlp_f16x3.hip), one per network.  That kernel adds the tiles it ran and
// the tiles it skipped to `dev`; a copy of the two counters travels to the page-locked `host` behind a launch, and once its event
// has completed the host knows the share of skipped tiles of the launches since the previous copy.  A network whose share
// stays under kMinShare pays the vote for nothing (a trained scene: 0.002), so its next kFullRun launches run the full kernel
// and the one after them probes again.  Both kernels give the same bits, so the gate can change speed and nothing else.
// Reset with the weights (repack_render_streams).
struct RgbSkipGate {
    static constexpr int kFullRun = 63;          // launches on the full kernel between two probes
    static constexpr int kCopyEvery = 8;         // launches of the rgb-skipping kernel between two copies once a share is known
    static constexpr unsigned kMinShareDen = 4;  // kMinShare = 1 / 4: a skipped tile saves ~5 %, one not skipped costs ~1.8 %
    unsigned long long* dev = nullptr;           // {tiles, skipped}, cumulative since the weights were loaded
    unsigned long long* host = nullptr;
    hipEvent_t ev = nullptr;
    bool pending = false;                        // a copy is in flight (host is not to be read)
    bool discard = false;                        // ... and it counts launches of weights since replaced: no verdict from it
    unsigned long long seen[2] = {0, 0};         // the counters at the previous completed copy
    int full_left = 0, since_copy = 0;
    bool known = false;                          // a share has been seen since the reset
};

struct TrainState;   // train_api.hip
struct CommState;    // comm_api.hip

}  // namespace nerf

struct nerf_ctx {
    nerf_config cfg;
    int sampling = NERF_SAMPLING_LINEAR;       // coarse depths: nerf_ctx_set_sampling
    int ray_space = NERF_RAYS_WORLD;           // rays nerf_render_image generates: nerf_ctx_set_ray_space
    float ndc_near_plane = 1.0f;
    bool box_on = false;                       // scene box, in the space of the rays the depth kernel sees: nerf_ctx_set_scene_box
    nerf::SceneBox box = {};
    int grid_R = 0;                            // occupancy grid over the box (0: none): nerf_ctx_set_occupancy_grid / nerf_occupancy_bake
    int grid_cur = 0;                          // which of b_grid holds it; the other is the dilation's second array
    nerf::DevBuf b_grid[2];                    // grid_R^3 / 32 words each
    nerf::DevBuf b_gbounds, b_gstate;          // per-ray (a, b) and state of draw_z_values under a grid (grow-only)
    // sample culling (cull_kernels.hip): a switch acts only while the ctx holds a grid (culling_acts)
    bool cull_on = false;                      // nerf_ctx_set_sample_culling: the render path's switch
    bool train_cull_on = false;                // nerf_ctx_set_train_sample_culling: the trainer's switch
    long long cull_samples = 0, cull_kept = 0; // totals over the culled passes since nerf_ctx_read_culling
    uint32_t* cull_rows = nullptr;             // page-locked word the row count M of a pass is copied to
    nerf::SampleCompaction cull;               // the render path's record (the trainer's: TPass::cull)
    nerf::DevBuf b_csums;                      // the scan's tile sums + total; this and the next line: scratch of one forward pass
    nerf::DevBuf b_cxyz, b_cdirs, b_craw;      // the M compact rows: points, directions, raw (sized after M is known)
    std::vector<hipEvent_t> cull_ev;           // with timing on, six per culled RENDER pass: verdict+scan | read M | gather | (MLP) | expand
    size_t cull_ev_used = 0;
    // mesh extraction (mesh_kernels.hip): the pending mesh of nerf_isosurface and its scratch, all grow-only
    bool mesh_on = false;
    long long mesh_V = 0, mesh_T = 0;
    nerf::DevBuf b_mesh_v, b_mesh_n, b_mesh_t;                             // vertices, normals, triangles
    nerf::DevBuf b_mesh_sigma, b_mesh_mask, b_mesh_first, b_mesh_count, b_mesh_tfirst, b_mesh_sums;
    nerf::DevBuf b_lattice;                    // a host caller's lattice: baked, before it leaves; a volume, staged in
    nerf::DevBuf b_sh_table;                   // nerf_sh_radiance_lattice: the call's directions (D, 3), then its projection (K, D)
    int num_cus = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;         // device-to-host copies of nerf_render_image(NERF_MEM_HOST), beside the kernels
    std::vector<hipEvent_t> copy_ev;           // "batch k is done" events the copy stream waits on (ring)
    nerf::NetWeights net[2];
    // Device gather tables of the operand streams (nerf_kernels.h::build_stream_tables), built on first use: rt[k] the table
    // of stream kind k where k is its own table source (StreamDesc::table), rt_cst[b] the table of constant block b.  The
    // render path's streams and the fused trainer's stash-forward stream are all re-packed through them.
    int32_t* rt[nerf::kStreamKinds] = {};
    int32_t* rt_cst[nerf::kConstBlocks] = {};
    bool rt_built = false;
    // Encoding window (nerf_ctx_set_encoding_window): the per-octave weights as given, and -- while a window is on -- the
    // scale table over the blob (nerf_kernels.h::build_scale_table) every re-pack multiplies by and every writer into a
    // trainer's gradient blob scales its contribution with.  Off (never set, or all ones): win_on false, no kernel sees a table.
    bool win_on = false;
    float win_xyz[10] = {1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f};
    float win_dir[4] = {1.f, 1.f, 1.f, 1.f};
    std::vector<float> win_host;               // the table on the host (source of the upload)
    float* win_scale = nullptr;                // ... and on the device (blob size; kept once allocated)
    // scratch arena (grow-only).  Staging (nerf::Staging, host-memory calls): b_orig, b_dirs (rays), b_u0, b_u1 (draws), b_in0,
    // b_in1, b_in2 (other arguments), b_out[i] (member i of nerf_outputs); an entry also stages in b_zc, b_zf or b_raw where the
    // passes it runs leave that buffer alone.  The passes (draw_z_values, dev_render, dev_render_rays, run_mlp's callers, the
    // bake): b_zc, b_zf, b_raw, b_wc here, b_g* and b_c* above; the bake, the lattice and the vertex colours also generate their
    // points into b_in0 / b_in1.
    nerf::DevBuf b_orig, b_dirs, b_zc, b_zf, b_raw, b_wc, b_u0, b_u1, b_in0, b_in1, b_in2;
    nerf::DevBuf b_out[7];
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    size_t ev_used = 0;
    long long timed_rows = 0;
    unsigned long long* nonfinite = nullptr;   // device counter fed by the MLP kernels
    nerf::RgbSkipGate skip_gate[2];            // nerf_api.hip: rgb_skip_wanted / rgb_skip_launched
    nerf::TrainState* train = nullptr;         // optimizer state + training buffers (nerf_train_begin)
    nerf::CommState* comm = nullptr;           // RCCL communicator + slab buffers (nerf_comm_init)
};

namespace nerf {

int ensure(nerf_ctx* c, DevBuf& b, size_t bytes);   // grow-only device buffer
int h2d(nerf_ctx* c, DevBuf& b, const void* src, size_t bytes);
int enter(nerf_ctx* c);                             // NULL check + hipSetDevice
// library buffer -> caller's buffer (device to host, or device to device, by `mem`) and caller's buffer -> library buffer, on the
// ctx stream; neither synchronises: a host caller's entry point does, once
int copy_to_caller(nerf_ctx* c, void* dst, const void* src_dev, size_t bytes, int mem);
int copy_from_caller(nerf_ctx* c, void* dst_dev, const void* src, size_t bytes, int mem);

// The pointer arguments of one entry point that takes `int mem`: made at its top, finished at its end.  For a device caller
// in() and out() hand the caller's pointer back and finish() does nothing (the call stays asynchronous); for a host caller in()
// uploads into `b`, out() grows `b` and remembers the copy back, finish() enqueues those copies in the order they were
// registered and synchronises once.  A NULL argument gives NULL.  The caller names the buffer: which arena buffers a pass
// leaves alone is the entry point's knowledge (see the arena in nerf_ctx).  An output registered on the buffer its input was
// staged into shares it (nerf_rays_to_ndc in place).  A failure is kept in `err` and makes every later in() / out() a no-op
// that gives NULL: check it once, before the launches; a call that returns before finish() copies nothing back.
struct Staging {
    Staging(nerf_ctx* c, int mem);
    template <class T> const T* in(DevBuf& b, const T* src, size_t bytes) { return (const T*)stage(b, (void*)src, bytes, true); }
    template <class T> T* out(DevBuf& b, T* dst, size_t bytes) { return (T*)stage(b, dst, bytes, false); }
    int finish();
    int err = 0;

private:
    void* stage(DevBuf& b, void* caller, size_t bytes, bool upload);
    nerf_ctx* c;
    bool host;
    struct { void* dst; const void* src; size_t bytes; } back[7];   // (nerf_outputs has the most outputs of any entry: seven)
    int n_back = 0;
};
#define ENTER(c) do { if (int r__ = nerf::enter(c)) return r__; } while (0)
int sampling_ok(const nerf_ctx* c);                 // nerf_api.hip: the ctx's bounds suit its sampling mode (lindisp: near > 0)
inline int lattice_n_ok(const char* what, int n) { return n < 2 || n > 512 ? fail("%s: n must be in 2..512 (got %d)", what, n) : 0; }
// nerf_api.hip: network `which` on M device-resident points (view: NULL for n_angles == 0) -> raw (M, 4) in the ctx's precision, on the ctx
// stream: what nerf_model_predict runs, for a caller that makes its own points.  Before it: a lattice size outside 2..512, refused by name.
int eval_points(nerf_ctx* c, int which, const float* xyz, const float* view, long long M, float* raw);
// The coarse depths of N rays as this ctx draws them (bounds, sampling mode, scene box, occupancy grid): every call site that
// has rays.  Without a grid it launches what it always launched and cannot fail; with one it may grow two scratch buffers.
int draw_z_values(nerf_ctx* c, const float* o, const float* d, long long N, int S, const float* u, uint64_t seed,
                   long long ray_base, float* z);   // nerf_api.hip; device pointers, enqueued on the ctx stream

// a culling switch (cull_on, train_cull_on) acts only while the ctx holds a grid
inline bool culling_acts(const nerf_ctx* c, bool flag) { return flag && c->box_on && c->grid_R > 0; }
// nerf_api.hip: the compaction of one pass's N * S samples under the grid, for the render path and the trainer alike.  On
// success rec.rows = M, the cull_samples / cull_kept counters have advanced and, for M > 0, the kept samples' points (and
// directions, when the network has them) are the M rows of c->b_cxyz / b_cdirs.  stamp: record the render path's stage events.
int compact_samples(nerf_ctx* c, SampleCompaction& rec, const float* o, const float* d, const float* z, long long N, int S,
                    bool stamp);

void train_free(nerf_ctx* c);                       // train_api.hip: releases c->train (called by nerf_ctx_destroy)
void comm_free(nerf_ctx* c);                        // comm_api.hip: releases c->comm (called by nerf_ctx_destroy)
int comm_allreduce_mean(nerf_ctx* c, float* buf, size_t n);   // comm_api.hip: no-op without a communicator / one rank
int comm_world(const nerf_ctx* c);                            // ranks of the ctx's communicator (1 without one)
// nerf_api.hip: the ctx's gather tables, built and uploaded once; every operand stream network `which` keeps (allocated on
// first use) re-packed from a device blob of its weights, enqueued on the ctx stream -- after a weight load and after
// optimizer steps alike
int ensure_render_tables(nerf_ctx* c);
int repack_render_streams(nerf_ctx* c, int which, const float* dev_blob);
// the device scale table of the ctx's encoding window, NULL while it is off: what launch_repack, launch_relayout and the
// gradient reductions take
inline const float* window_scale(const nerf_ctx* c) { return c->win_on ? c->win_scale : nullptr; }
// train_api.hip, both no-ops without a trainer.  train_window_guard, before the window changes: refuses while a render slot
// holds a forward pass, and makes the ctx stream wait for the side stream's gradient reduction (it reads the table).
// train_on_window, after: both networks' operand streams (the reference trainer: matrices) re-packed under the new window.
// train_master_blob: the device blob of the master weights of network `which` while a trainer holds it, else NULL.
int train_window_guard(nerf_ctx* c);
int train_on_window(nerf_ctx* c);
const float* train_master_blob(const nerf_ctx* c, int which);
int train_on_load(nerf_ctx* c, int which);          // train_api.hip: no-op without a trainer
int train_flush_weights(nerf_ctx* c, int which, bool to_host = false);
// (train_flush_weights: train_api.hip, no-op unless optimizer steps changed the weights)

}  // namespace nerf
