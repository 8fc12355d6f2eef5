// nerf_kernels.h -- internal declarations shared by the HIP translation units of libnerf_mi355.so.
// gfx950 (MI355X) only.  Nothing here is part of the C ABI (see include/nerf_mi355.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace nerf {

// ---- fixed network geometry of the fused kernel (all BASELINE configs) ----
// n_angles_for_model 2 and 1 share the kernels: with 1 the y component of the view direction is still
// encoded on device but its weight rows are zeros (padding entries of the gather tables below).
constexpr int kLx = 5;           // n_pos_enc_dim_xyz
constexpr int kLd = 4;           // n_pos_enc_view_dir
constexpr int kHidden = 256;
constexpr int kLast = 128;
constexpr int kXyzDim = 3 + 6 * kLx;   // 33
constexpr int kDirDim = 6 * kLd;       // 24
// Fewer octaves (1 <= Lx <= kLx, 1 <= Ld <= kLd) run on the same kernels, the way n_angles 1 does: the octaves the network
// does not have are still encoded on device, but their weight rows are zeros.  Every gather table is written for the
// (kLx, kLd) blob (kLxWide: the wide-PE kernels') and then aimed at the network's own (lx, ld) blob (aim_gather).
// weight_tables.hip: the Dense layers' (in, out) of an (lx, ld, n_angles) network in Keras creation order (src/NeRF.py:249-339)
// -> the layer count, 11, or 12 for the xyz-only network.  The one place the shapes are written.
int layer_dims(int lx, int ld, int n_angles, int dims[12][2]);
// Floats of the weight blob of that network (Keras get_weights() order: kernel (in, out) row-major, bias, per layer)
size_t blob_floats(int lx, int ld, int n_angles);
// idx[i], i < blob_floats(layout_lx, kLd, n_angles): 1 + the index of the same weight in the (lx, ld) blob, 0 where the
// (layout_lx, kLd) layout holds an octave row the (lx, ld) network does not have (a zero); layout_lx = kLx or kLxWide
void blob_expand_index(int lx, int ld, int n_angles, int32_t* idx, int layout_lx = kLx);
// A table written for the (pe_layout_lx(lx), kLd) blob, re-aimed at the (lx, ld) blob: the slots of the octave rows the network
// does not have become padding.  f16: entries are 2 * (src + 1) + is_lo (the 16-bit streams); else src + 1
void aim_gather(int lx, int ld, int n_angles, int32_t* idx, size_t n, bool f16);

// ---- weight stream geometry (see DESIGN.md "weight stream") ----
// A "quad" is the A operand of 4 consecutive MFMA k-steps for one 32-wide output tile:
// 64 lanes x 4 floats = 1 KiB, lane-linear, read with one ds_read_b128 per lane.
constexpr int kQuadBytes = 1024;
constexpr int kChunkQuads = 16;
constexpr int kChunkBytes = kQuadBytes * kChunkQuads;   // 16 KiB = one LDS ring slot
constexpr int kRingChunks = 8;   // power of two
constexpr int kRingBytes = kChunkBytes * kRingChunks;   // 128 KiB

// quads per output tile for each layer body
constexpr int kQpuPE = 5;                 // 17 k-steps (15 sin/cos pairs + raw xyz) padded to 20
constexpr int kQpuHid = 32;               // 128 k-steps
constexpr int kQpuSkip = kQpuPE + kQpuHid;  // layer 4: [xyz_enc(33), hidden(256)]
constexpr int kQpuLast = kQpuHid + 3;     // layer 8: [hidden(256), dir_enc(24)] -> 128
constexpr int kChunksPE = (8 * kQpuPE + 15) / 16;      // 3
constexpr int kChunksHid = (8 * kQpuHid) / 16;         // 16
constexpr int kChunksSkip = (8 * kQpuSkip + 15) / 16;  // 19
constexpr int kChunksLast = (4 * kQpuLast + 15) / 16;  // 9
constexpr int kStreamChunks = kChunksPE + 3 * kChunksHid + kChunksSkip + 3 * kChunksHid + kChunksLast;  // 127
constexpr size_t kStreamBytes = size_t(kStreamChunks) * kChunkBytes;
constexpr size_t kStreamBytesXyzF32 = size_t(142) * kChunkBytes;   // the xyz-only network's fp32 stream (12 Dense layers, mlp_fp32.hip)
constexpr size_t kStreamBytesF16 = size_t(66) * 32 * kQuadBytes;   // f16x3 stream: 66 chunks of 32 KiB (mlp_f16x3.hip)
constexpr size_t kStreamBytesF16Hi = size_t(33) * 32 * kQuadBytes; // single-pass fp16 stream: hi fragments only
constexpr size_t kStreamBytesF16Sig = size_t(62) * 32 * kQuadBytes; // f16x3 sigma-only stream (coarse render pass)
constexpr size_t kStreamBytesF16Skip = size_t(67) * 32 * kQuadBytes; // f16x3 sigma-first stream (rgb-skipping render pass)
constexpr size_t kStreamBytesF16Xyz = size_t(73) * 32 * kQuadBytes;    // the xyz-only network's streams (12 Dense layers)
constexpr size_t kStreamBytesF16HiXyz = size_t(37) * 32 * kQuadBytes;

// ---- constant region (biases + head weights), floats ----
constexpr int kConstBias = 0;                       // 8 x 256 hidden-layer biases (layers 0..7)
constexpr int kConstBias8 = 2048;                   // 128
constexpr int kConstWrgb = 2176;                    // [3][128]
constexpr int kConstBHead = 2560;                   // b_r, b_g, b_b, b_sigma
constexpr int kConstWsigH = 2564;                   // [256]  sigma head, hidden part
constexpr int kConstWsigD = 2820;                   // [3][2][4] sigma head, dir part (g, half, e)
constexpr int kConstFloats = 3136;                  // the LDS carve of the constants (largest user: the xyz-only trainer's backward: 3120 + 16 gmax slots)
constexpr int kConstBytes = kConstFloats * 4;

// LDS carve of the MLP kernel
constexpr int kLdsRing = 0;
constexpr int kLdsConst = kRingBytes;
constexpr int kLdsTotal = kRingBytes + kConstBytes;   // 142,464 B of the 160 KiB

struct MlpArgs {
    const float* wstream;   // packed A-operand stream of one network (kStreamBytes)
    const float* wconst;    // constant region (kConstFloats)
    const float* in_a;      // mode 0: rays_orig (N,4)   | mode 1: xyz (M,3)
    const float* in_b;      // mode 0: rays_dirs (N,4)   | mode 1: view_dirs (M,3)
    const float* z;         // mode 0: (N,S)             | mode 1: unused
    float* raw;             // (M,4) raw [r,g,b,sigma]
    unsigned long long* nonfinite;   // device counter: rows whose raw output is not finite (may be null)
    long long M;            // number of samples (rows)
    int S;                  // samples per ray (mode 0)
    int mode;
    float alpha;            // LeakyReLU slope
    // training forward (mlp_f16x3 "stash" kernels only): where the activation of layer l = 0..8 (0..9 for the xyz-only
    // network: ..., 8 = its extra 256-wide layer, 9 = the 128-wide one) is written, fragment-major with st_ld[l] elements
    // per row (rows padded to a multiple of 128); unused (null) when rendering
    float* st_ptr[10];
    int st_ld[10];
    // ... and where the LeakyReLU' mask bits of layer l's output go: one uint4 per (row, lane half), see mlp_f16x3.hip
    uint32_t* mask_ptr[10];
    int diag_wrap;          // diagnostic only (NERF_DIAG_STASH_WRAP=1): every workgroup's stash rows land in the first 8192 rows (cache-resident)
};

// mlp_fp32.hip
void launch_mlp_fp32(const MlpArgs& a, int num_cus, hipStream_t stream, bool xyz_only = false);
void mlp_fp32_set_attributes();
// gather table of the fp32 stream of the (kLx, kLd) blob (kStreamBytes / 4 entries; n_angles 0: kStreamBytesXyzF32 / 4) and of
// its constant block (kConstFloats): entry = src + 1, 0 = padding
void build_fp32_gather(int n_angles, int32_t* stream_idx, int32_t* const_idx);

// mlp_f16x3.hip
// single_pass: hi*hi only; xyz_only: the 12-layer network without view directions (its own streams / constants)
void launch_mlp_f16x3(const MlpArgs& a, int num_cus, hipStream_t stream, bool single_pass = false, bool xyz_only = false);
// forward that also writes a.st_ptr / a.mask_ptr (training); single_pass: the mixed_float16-class arithmetic
void launch_mlp_f16x3_stash(const MlpArgs& a, int num_cus, hipStream_t stream, bool single_pass = false, bool xyz_only = false);
// gather tables of the 3-pass (or hi-only) stream (kStreamBytesF16[Hi][Xyz] / 2 entries: 2 * (src + 1) + is_lo) and of the
// 16-bit kernels' constant block (kConstFloats: src + 1; the same from either stream); 0 = padding
void build_f16x3_gather(int n_angles, bool hi_only, int32_t* stream_idx, int32_t* const_idx);
void mlp_f16x3_set_attributes();
// sigma-only coarse render (3-pass, n_angles 1 or 2, the kLx build only): a.raw receives sigma alone, (M,) floats; its
// stream (kStreamBytesF16Sig) ends in layer 8's sigma tile, its constants are the full stream's
void launch_mlp_f16x3_sig(const MlpArgs& a, int num_cus, hipStream_t stream);
void build_f16x3_sig_gather(int n_angles, int32_t* stream_idx /* kStreamBytesF16Sig / 2 */);
// rgb-skipping render (3-pass, n_angles 1 or 2, the kLx build only), for a caller that reads no per-sample rgb: a.raw as the
// full kernel's, except that a 128-row tile whose every row has raw sigma <= 0 (or lies past M) is written {0, 0, 0, sigma}
// without its rgb being computed -- such a row has alpha = 0 exactly and its rgb reaches no pixel.  Its stream
// (kStreamBytesF16Skip) holds layer 8 sigma tile first, its constants are the full stream's.
// skip_count (nullable; a kernel argument of its own, so MlpArgs and with it every other kernel's argument layout stay as they
// are): [0] += the 128-row tiles the launch ran, [1] += those it skipped
void launch_mlp_f16x3_rgbskip(const MlpArgs& a, int num_cus, hipStream_t stream, unsigned long long* skip_count = nullptr);
void build_f16x3_rgbskip_gather(int n_angles, int32_t* stream_idx /* kStreamBytesF16Skip / 2 */);

// mlp_f16x3_wide.hip -- the same entry points for networks with n_pos_enc_dim_xyz 6..10: kernels that encode kLxWide octaves,
// gather tables for the (kLxWide, kLd) blob layout (same stream sizes).  No exact-fp32 render kernel exists for them.
constexpr int kLxWide = 10;
namespace wide {
void launch_mlp_f16x3(const MlpArgs& a, int num_cus, hipStream_t stream, bool single_pass = false, bool xyz_only = false);
void launch_mlp_f16x3_stash(const MlpArgs& a, int num_cus, hipStream_t stream, bool single_pass = false, bool xyz_only = false);
void build_f16x3_gather(int n_angles, bool hi_only, int32_t* stream_idx, int32_t* const_idx);
void mlp_f16x3_set_attributes();
}  // namespace wide
// mlp_bf16x3.hip / mlp_bf16x3_wide.hip -- the bf16 build of mlp_f16x3.hip's 3-pass RENDER kernels (NERF_PRECISION_BF16X3):
// bf16 hi/lo streams of the same geometry (kStreamBytesF16 / kStreamBytesF16Xyz / kStreamBytesF16Sig) and the same constants.
// No single-pass and no stash variant.  Their streams are re-packed from the fp16 twins' gather tables (same slots), rounded
// to bf16.
namespace bf16 {
void launch_mlp_bf16x3(const MlpArgs& a, int num_cus, hipStream_t stream, bool xyz_only = false);
void launch_mlp_bf16x3_sig(const MlpArgs& a, int num_cus, hipStream_t stream);      // the kLx build only, as the fp16 one
void mlp_bf16x3_set_attributes();
namespace wide {
void launch_mlp_bf16x3(const MlpArgs& a, int num_cus, hipStream_t stream, bool xyz_only = false);
void mlp_bf16x3_set_attributes();
}  // namespace wide
}  // namespace bf16
// the octaves of the blob layout the kernels of an (lx, .) network are packed for: kLx, or kLxWide for lx > kLx
inline int pe_layout_lx(int lx) { return lx > kLx ? kLxWide : kLx; }

// ---- the render path's resident operand streams, stated once ----
// Every stream is a gather table over the weight blob plus one device re-pack (launch_repack).  The re-pack after a weight
// load and after optimizer steps (nerf_api.hip: repack_render_streams), kernel choice (pick_render_kernel) and the
// host-sanitizer tool (tools/pack_asan_test.cpp) all walk render_streams(); none of them names a stream on its own.
enum StreamKind { kF16x3, kF16Hi, kBf16x3, kF16x3Sig, kBf16x3Sig, kFp32, kF16x3Skip, kStreamKinds };   // in re-pack order
enum ConstBlock { kConstFp32, kConst16, kConstBlocks };   // the fp32 kernel's constants / the ones every 16-bit kernel reads
enum StreamElem { kElemF16, kElemBf16, kElemF32 };        // what a slot holds: an fp16 or bf16 hi / lo part, or the fp32 value
struct StreamDesc {
    size_t bytes;        // 0: this network does not keep the stream
    ConstBlock cst;      // the constant block its kernels read
    StreamKind table;    // the kind whose gather table the re-pack reads (the bf16 kinds: their fp16 twins', same slots)
    StreamElem elem;     // ... and what it rounds a gathered weight to
};
// the streams network `which` (0 = coarse, 1 = fine) of an (lx, n_angles) config keeps.  Wide-PE networks (lx > kLx) have no
// fp32 and no sigma-only streams; xyz-only networks the ...Xyz sizes and no sigma-only streams; sigma-only: the coarse network;
// the sigma-first stream of the rgb-skipping kernel: either network that has view directions and the kLx build
inline void render_streams(int lx, int n_angles, int which, StreamDesc d[kStreamKinds]) {
    const bool wd = lx > kLx, xyz = n_angles == 0;
    const size_t b3 = xyz ? kStreamBytesF16Xyz : kStreamBytesF16, b1 = xyz ? kStreamBytesF16HiXyz : kStreamBytesF16Hi;
    const size_t bs = !wd && !xyz && which == 0 ? kStreamBytesF16Sig : 0, bf = wd ? 0 : xyz ? kStreamBytesXyzF32 : kStreamBytes;
    d[kF16x3] = {b3, kConst16, kF16x3, kElemF16};
    d[kF16Hi] = {b1, kConst16, kF16Hi, kElemF16};
    d[kBf16x3] = {b3, kConst16, kF16x3, kElemBf16};
    d[kF16x3Sig] = {bs, kConst16, kF16x3Sig, kElemF16};
    d[kBf16x3Sig] = {bs, kConst16, kF16x3Sig, kElemBf16};
    d[kFp32] = {bf, kConstFp32, kFp32, kElemF32};
    d[kF16x3Skip] = {!wd && !xyz ? kStreamBytesF16Skip : 0, kConst16, kF16x3Skip, kElemF16};
}
// The table builder of a kind that is its own table source: stream_idx (bytes / 2 entries, the fp32 kind: bytes / 4), written
// for the (pe_layout_lx(lx), kLd) blob; -> whether the kind owns its constant block, i.e. const_idx (kConstFloats entries) was
// written too.  kF16x3 owns kConst16 (every config keeps that stream), kFp32 owns kConstFp32.
inline bool build_stream_gather(int lx, int n_angles, StreamKind k, int32_t* stream_idx, int32_t* const_idx) {
    if (k == kFp32) { build_fp32_gather(n_angles, stream_idx, const_idx); return true; }
    if (k == kF16x3Sig) { build_f16x3_sig_gather(n_angles, stream_idx); return false; }
    if (k == kF16x3Skip) { build_f16x3_rgbskip_gather(n_angles, stream_idx); return false; }
    (lx > kLx ? wide::build_f16x3_gather : build_f16x3_gather)(n_angles, k == kF16Hi, stream_idx, k == kF16x3 ? const_idx : nullptr);
    return k == kF16x3;
}
// weight_tables.hip: every table of an (lx, ld, n_angles) config, aimed at its own blob -- stream[k] for each kind either
// network keeps that is its own table source (empty otherwise), cst[b] for each constant block a kept kind owns
struct StreamTables { std::vector<int32_t> stream[kStreamKinds], cst[kConstBlocks]; };
void build_stream_tables(int lx, int ld, int n_angles, StreamTables& t);
// weight_tables.hip: the encoding window (nerf_ctx_set_encoding_window) as a scale table over the (lx, ld, n_angles) blob, one
// float per blob element: w_xyz[k] on the rows of octave k of the xyz encoding in layers 0 and 4, w_dir[k] on the rows of
// octave k of the direction encoding in layers 8 and 10 (n_angles 1 or 2), 1 everywhere else (pass-through rows, hidden rows,
// biases, the xyz-only network's layers 8..11).  w_xyz: lx values, w_dir: ld values.
void build_scale_table(int lx, int ld, int n_angles, const float* w_xyz, const float* w_dir, std::vector<float>& scale);
// aux_kernels.hip: the one device re-pack.  out[i], i < n: the weight slot idx[i] names, rounded to `elem` (fp16 / bf16: hi
// = the rounded weight, lo = the rounded rest; fp32: the weight), 0 for padding; and, with const_idx, cst[i] for i <
// kConstFloats the same way in fp32 (a table's constant block rides in its stream's launch).  scale (nullable: none): a
// device scale table over the blob; every gathered weight is then fl32(blob[i] * scale[i]).
void launch_repack(StreamElem elem, const float* blob, const float* scale, const int32_t* idx, void* out, size_t n,
                   const int32_t* const_idx, float* cst, hipStream_t s);

// mlp_f16_2t.hip -- single-pass fp16 render kernel with two 32-sample tiles per wave (same hi-only stream / constants)
void launch_mlp_f16_2t(const MlpArgs& a, int num_cus, hipStream_t stream);
void mlp_f16_2t_set_attributes();

// mlp_bwd_f16x3.hip -- the trainer's fused data-gradient chain (the stash forward's counterpart)
constexpr size_t kBwdStreamBytes = size_t(73) * 32 * kQuadBytes;   // transposed-weight stream incl. the encoding tiles (73 chunks: the xyz-only network's)
constexpr int kBwdXyzLd = 64;                                      // floats per row of an encoding-gradient buffer
// "pair16" gradient buffers of the fused float32-policy trainer: the backward chain stores every pre-activation gradient as the fp16 (hi, lo) pair it
// packs as the next MFMA operand anyway, in the value's fp32 slot -- {hi01, hi23, lo01, lo23} per four consecutive
// features of a row -- with the chain's per-row power-of-two scale still on it (its inverse is stored per row,
// MlpBwdArgs::rs_ptr), and the weight-gradient GEMM (gemm_atb_p, train_kernels.hip) stages that operand with byte permutes
// and one packed multiply instead of scaling and splitting fp32 rows on the fly.  The chain no longer forms the
// true-scale value at all (a select and a multiply per value less than the fp32 buffers they replaced).  The mixed_float16
// policy's single-pass chain stores plain fp16 gradients instead.
struct MlpBwdArgs {
    const void* wstream;     // backward operand stream of one network (build_bwd_gather / launch_repack)
    const float* wconst;     // the forward kernel's constant block (rgb head weights are read from it)
    const float* graw;       // (Mp, 4) gradient w.r.t. the raw network output [r, g, b, sigma]; padding rows zero
    const uint32_t* mask_ptr[10];  // LeakyReLU' bit records of layers 0..8 (0..9: xyz-only network), written by the stash forward
    float* d_ptr[10];        // d_ptr[l], l = 0..7: (Mp, 256) gradient w.r.t. layer l's pre-activation; d_ptr[8]: G9 (Mp, 128)
                             // xyz-only network: d_ptr[8] = (Mp, 256) of its extra layer, d_ptr[9] = (Mp, 128) of the last one
    float* dx_ptr[2];        // dx variant: (Mp, 64) gradient w.r.t. the xyz encoding through layer 4 / through layer 0
    uint16_t* rs_ptr[10];    // pair16 (3-pass kernels): per buffer d_ptr[l] and row the power of two r with true D = stored D' * r,
                             // as the upper half of r's fp32 bits
    float* dsig;             // optional (Mp): column 3 of graw as a contiguous vector -- the sigma head's weight gradient rides in the
                             // weight-gradient GEMM of layer 8, which stages C8 anyway (GemmAtb::sig_g)
    unsigned* gmax;          // 9 x 64 slots: bits of max|.| of G9 (slot group 0) and of D_(8-k) (slot group k); xyz-only
                             // network: 10 groups, group 0 = d_ptr[9], group k = d_ptr[9 - k]
    long long Mp;            // rows, multiple of 128
    float alpha;
    int ld, ld9;             // row pitch (floats) of d_ptr[0..7] / d_ptr[8]
};
// single_pass: hi*hi products only, gradients rounded to fp16 between layers (the mixed_float16 policy's backward)
void launch_mlp_bwd_f16x3(const MlpBwdArgs& a, bool dx, bool single_pass, int num_cus, hipStream_t stream,
                          bool xyz_only = false);
void mlp_bwd_f16x3_set_attributes();
// layout_lx: the octaves of the blob layout the table indexes (kLx, or kLxWide: the chain's two encoding tiles hold up to 64
// rows); entries as the fp16 streams' (2 * (src + 1) + is_lo), re-packed by launch_repack(kElemF16, ...)
void build_bwd_gather(int n_angles, bool dx, bool hi_only, int32_t* idx /* kBwdStreamBytes / 2 */, int layout_lx = kLx);

// aux_kernels.hip
void launch_raygen(const float c2w_host[16], float fov, int H, int W,
                   long long ray_begin, long long ray_count, float* orig /*nullable*/, float* dirs,
                   hipStream_t stream);
// world rays -> NDC rays (near plane z = -near_plane, both scale factors 1 / tan(fov / 2) as the raygen's); out may be in
void launch_rays_to_ndc(const float* orig, const float* dirs, long long N, float fov, float near_plane, float* out_orig,
                        float* out_dirs, hipStream_t stream);
// lindisp: strata uniform in 1/z (needs near_b > 0) instead of in z.  With rays (N,4) AND a box, every ray the box narrows
// draws on its own interval (aux_kernels.hip: ray_box_interval); with bounds AND state (launch_ray_grid_bounds' outputs,
// below) a ray of state 0 draws with the host's constants, any other on its own (a, b); with neither, every ray on
// [near_b, far_b].
struct SceneBox { float lo[3], hi[3]; };
void launch_z_values(float near_b, float far_b, bool lindisp, long long N, int S, const float* u, uint64_t seed,
                     long long ray_base, float* z, hipStream_t stream, const float* orig = nullptr,
                     const float* dirs = nullptr, const SceneBox* box = nullptr, const float* bounds = nullptr,
                     const int* state = nullptr);
// bounds (N,2): (a, b) of a narrowed ray, (near_b, far_b) of any other; narrowed (N) 0 / 1, nullable
void launch_ray_box_bounds(const SceneBox& box, float near_b, float far_b, const float* orig, const float* dirs, long long N,
                           float* bounds, int* narrowed, hipStream_t stream);
// Occupancy grid (aux_kernels.hip: ray_grid_interval): bits = R^3 / 32 device words over the box, cell (ix, iy, iz) = bit
// ix + R (iy + R iz).  bounds (N,2) and state (N; 0 untouched / 1 box only / 2 grid; nullable) of every ray, walked once
void launch_ray_grid_bounds(const SceneBox& box, float near_b, float far_b, const uint32_t* bits, int R, const float* orig,
                            const float* dirs, long long N, float* bounds, int* state, hipStream_t stream);
// field_kernels.hip (to launch_raw_rgba): the fills and drains of field_api.hip's queries.  Baking: the sample points (n_cells * spc, 3)
// of cells [cell_begin, cell_begin + n_cells), as many unit view directions (nullable); raw (n_cells * spc, 4) -> their bits; one
// step of 26-neighbour growth.  cell_begin, n_cells: multiples of 64
void launch_grid_points(const SceneBox& box, int R, long long cell_begin, long long n_cells, int spc, uint64_t seed,
                        float* xyz, float* view, hipStream_t stream);
void launch_grid_threshold(const float* raw, long long cell_begin, long long n_cells, int spc, float threshold,
                           uint32_t* bits, hipStream_t stream);
void launch_grid_dilate(const uint32_t* src, uint32_t* dst, int R, hipStream_t stream);
// points [begin, begin + count) of the n^3 lattice over the box (x fastest) and as many copies of view_dir
// (view nullable); column 3 of raw (count, 4); the view directions -normal ((0, 0, 1) for a zero normal); the sigmoid of
// columns 0..2 of raw (count, 4)
void launch_lattice_points(const SceneBox& box, int n, long long begin, long long count, const float view_dir[3], float* xyz,
                           float* view, hipStream_t stream);
void launch_raw_sigma(const float* raw, long long count, float* sigma, hipStream_t stream);
void launch_mesh_view(const float* normals, long long count, float* view, hipStream_t stream);
void launch_raw_rgb(const float* raw, long long count, float* rgb, hipStream_t stream);
// The radiance volume (nerf_radiance_lattice has the format, nerf_volume_sample and nerf_volume_march the rules).  The bake,
// still field_kernels.hip: the direction camera c2w's ray generator gives the pixel whose ray passes through each of xyz
// (count, 3); raw (count, 4) -> texels (count, 4), sigmoid of columns 0..2 and ReLU of column 3.
void launch_camera_view(const float c2w[16], const float* xyz, long long count, float* view, hipStream_t stream);
void launch_raw_rgba(const float* raw, long long count, float* texels, hipStream_t stream);
// The SH radiance lattice (nerf_sh_radiance_lattice has the rule), field_kernels.hip too: vertices [begin, begin + count) of the
// lattice, each D times, with the D directions of the device table (D, 3) (view nullable); raw (count * D, 4) -> texels (count,
// C(degree)) by the device projection table proj (K, D).
void launch_sh_lattice_points(const SceneBox& box, int n, long long begin, long long count, int D, const float* table, float* xyz,
                              float* view, hipStream_t stream);
void launch_sh_project(const float* raw, long long count, int degree, int D, const float* proj, float* texels, hipStream_t stream);
// mesh_kernels.hip's exclusive scan for bit-mask items: out[i] = set bits of in[0..i), *total_dev = set bits of all N bytes;
// sums: scratch of scan_sums_words(N) words.  No atomics: the result does not depend on the launch.
size_t scan_sums_words(long long N);
void launch_scan_popc(const uint8_t* in, long long N, uint32_t* sums, uint32_t* out, uint32_t* total_dev, hipStream_t stream);
// cull_kernels.hip (sample culling under an occupancy grid: sample_kept has the rule).  mask: ceil(N S / 64) 64-bit words, bit
// t = sample t is kept (nullable); verdict (N S) int32 1 / 0 (nullable).  first: launch_scan_popc of the mask's bytes.
// gather: the kept samples' points (M,3) and ray directions (M,3; nullable) in ascending sample index; expand: raw (total,4)
// -- sigma_only: (total,) -- from the M compact rows, zeros for a culled sample.
void launch_sample_keep(const SceneBox& box, const uint32_t* bits, int R, const float* orig, const float* dirs, const float* z,
                        long long N, int S, uint64_t* mask, int* verdict, hipStream_t stream);
void launch_sample_gather(const float* orig, const float* dirs, const float* z, long long N, int S, const uint8_t* mask,
                          const uint32_t* first, float* xyz, float* view, hipStream_t stream);
void launch_raw_expand(const float* compact, long long total, bool sigma_only, const uint8_t* mask, const uint32_t* first,
                       float* raw, hipStream_t stream);
// ... and the backward half of a culled training pass (nerf_ctx_set_train_sample_culling).  graw_gather: the kept rows of
// graw (total,4) as compact (Mp,4), rows M.. zero.  (The encoding backward is train_kernels.h::launch_pe_bwd given mask, first.)
void launch_graw_gather(const float* graw, long long total, long long M, long long Mp, const uint8_t* mask, const uint32_t* first,
                        float* compact, hipStream_t stream);
size_t sample_pdf_lds_bytes(int S, int Sf);
void launch_sample_pdf(const float* weights, const float* z, long long N, int S, int Sf, const float* u,
                       uint64_t seed, long long ray_base, float* z_new, float* z_merged,
                       hipStream_t stream);
void launch_composite(const float* raw, const float* z, long long N, int S, float* rgb, float* weights,
                      float* cumprod, float* alpha, float* rgb_samples, float* depth, hipStream_t stream);
// the weights alone, from a compact (N*S,) sigma vector (launch_mlp_f16x3_sig's output): bit-identical to launch_composite's
void launch_composite_weights(const float* sigma, const float* z, long long N, int S, float* weights, hipStream_t stream);
void launch_posenc(const float* x, long long M, int n_enc, int passthrough, float* out, hipStream_t stream);

}  // namespace nerf
