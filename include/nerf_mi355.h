/*
 * nerf_mi355.h -- C ABI of libnerf_mi355.so, the MI355X (gfx950) NeRF volumetric renderer.
 *
 * Drop-in boundary for the render hot path of Sahar-E/NeRF-and-DietNeRF.  The reference has no
 * FFI of its own; its seam is the late-bound Python call `src.UtilsNeuralRadianceField.render_rays`
 * (src/NeRF.py:180-188).  Each entry point below names the reference function it replaces.
 * Plain pointers and sizes only: no torch / TensorFlow types cross this boundary.
 *
 * Conventions
 *   - all arrays are C-contiguous fp32 unless stated; rays are (N,4) homogeneous rows exactly as the
 *     reference passes them (origin w=1, direction w=0); only xyz is read (src/UtilsNRF.py:204).
 *   - `mem` says where EVERY pointer of that call lives: NERF_MEM_HOST (library stages through its
 *     own device arena) or NERF_MEM_DEVICE (pointers are used in place on the ctx's stream).
 *   - every function returns 0 on success, non-zero on error; nerf_last_error() gives the
 *     thread-local message.  The library never aborts the process and never falls back to a CPU path.
 *   - a ctx is single-caller (not re-entrant), owns one HIP stream, the device copies of both
 *     networks' weights and a scratch arena; the caller owns all in/out buffers.
 *   - calls are synchronous on return for NERF_MEM_HOST; for NERF_MEM_DEVICE they are enqueued on the
 *     ctx stream and the caller synchronises with nerf_ctx_synchronize() (or its own stream, if it
 *     installed one with nerf_ctx_set_stream()).
 */
#ifndef NERF_MI355_H
#define NERF_MI355_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 6 also covers the forward-facing-scene entries added after it (nerf_ctx_set_sampling, nerf_ctx_set_ray_space,
 * nerf_rays_to_ndc), the scene-box entries (nerf_ctx_set_scene_box, nerf_ray_box_bounds, nerf_get_z_values_rays) and the
 * occupancy-grid entries (nerf_ctx_set_occupancy_grid, nerf_ctx_get_occupancy_grid, nerf_occupancy_bake,
 * nerf_ray_occupancy_bounds) and the mesh entries (nerf_density_lattice, nerf_isosurface, nerf_isosurface_fetch,
 * nerf_mesh_colors) and the distortion-loss entries (nerf_train_set_distortion_weights, nerf_train_read_distortion_sums,
 * nerf_distortion_loss) and the radiance-volume entries (nerf_radiance_lattice, nerf_volume_sample, nerf_volume_march,
 * nerf_volume_render_image) and their spherical-harmonic forms (nerf_sh_radiance_lattice, nerf_sh_volume_sample,
 * nerf_sh_volume_march, nerf_sh_volume_render_image), all marked "ABI 6+" below: they are additive -- no existing entry, struct or default changes -- so the
 * number that gates compatibility stays; a caller that may meet an older library of ABI 6 probes them with dlsym. */
#define NERF_ABI_VERSION 6

enum { NERF_NET_COARSE = 0, NERF_NET_FINE = 1 };
enum { NERF_MEM_HOST = 0, NERF_MEM_DEVICE = 1 };
/* arithmetic of the 256-wide contractions; everything else is always fp32 */
enum {
    NERF_PRECISION_FP32 = 0,   /* v_mfma_f32_32x32x2_f32: exact fp32 fma chains (parity mode)      */
    NERF_PRECISION_F16X3 = 1,  /* 3-pass split-fp16 MFMA (hi*hi + hi*lo + lo*hi), fp32 accumulate.  fp32-class between two
                                  limits: |activations| < 65504 (beyond: non-finite rows, counted by nerf_ctx_read_nonfinite),
                                  and NOT TOO SMALL -- the lo half of an activation is an fp16 subnormal (absolute step
                                  2^-24) below |y| = 2^-4 and hi itself below 2^-14, so the mode loses bits as a layer's
                                  activations shrink, with every value finite and NOTHING COUNTED.  Measured on the shipped
                                  checkpoint (layer-1 activations: mean 0.14, max 1.8) with that layer scaled by 2^k: raw
                                  outputs 1.7e-6 of the fp32 network at k = 0, 1.1e-5 at -4, 2.3e-4 at -8, 2.5e-3 at -12;
                                  final RGB leaves 1e-4 at k = -9 (mean |y| 2.7e-4, max 3.5e-3).  NERF_PRECISION_BF16X3 is
                                  the mode for such weights (8.9e-6 / 1.3e-5 at every k).  DESIGN.md section 4.1b */
    NERF_PRECISION_F16 = 2,    /* 1-pass fp16 MFMA, fp32 accumulate, activations rounded to fp16 between layers: the
                                  numerics class of the reference's production policy (mixed_float16,
                                  src/ExecutionRun.py:220-221); NOT the fp32 parity mode */
    NERF_PRECISION_BF16X3 = 3  /* 3-pass split-bf16 MFMA (hi*hi + hi*lo + lo*hi), fp32 accumulate: ~16 significant bits per
                                  operand (fp32-class results, 1e-4 RGB) with fp32's exponent range -- nothing saturates at
                                  65504.  Render path only: the trainer's kernels do not depend on the ctx precision */
};

/* ABI 6+: where the coarse depths of a ray fall (nerf_ctx_set_sampling) */
enum {
    NERF_SAMPLING_LINEAR = 0,  /* stratified, uniform in depth between near and far: get_z_values, src/UtilsCV.py:565-581 */
    NERF_SAMPLING_LINDISP = 1  /* stratified, uniform in DISPARITY 1/z ("lindisp"): half of the samples lie nearer than
                                  2 near far / (near + far); for scenes whose content runs from ~1 unit to (almost) infinity */
};
/* ABI 6+: the space of the rays nerf_render_image generates from a camera (nerf_ctx_set_ray_space) */
enum {
    NERF_RAYS_WORLD = 0,       /* world-space pinhole rays: get_rays_directions, src/UtilsCV.py:467-499 */
    NERF_RAYS_NDC = 1          /* the same rays re-parameterised in normalised device coordinates (see nerf_rays_to_ndc) */
};

/* Network + frustum description: the 9 net/render keys of src/ConfigurationKeys.py:64-111. */
typedef struct nerf_config {
    int32_t n_pos_enc_xyz;    /* n_pos_enc_dim_xyz   (5)   accepted: 1..10; 6..10 with precision f16x3 / bf16x3 / f16 only */
    int32_t n_pos_enc_dir;    /* n_pos_enc_view_dir  (4)   accepted: 1..4 */
    int32_t n_angles;         /* n_angles_for_model  (2)   accepted: 0 (xyz-only network), 1, 2 */
    int32_t hidden_dim;       /* hidden_layer_dim    (256) accepted: 256 only */
    int32_t last_hidden_dim;  /* last_hidden_layer_dim (128) accepted: 128 only
                               * Anything else fails nerf_ctx_create (nerf_blob_size returns 0) with a message naming the
                               * accepted ranges.  Weight blobs follow the reference's Keras layer shapes for the given
                               * values (src/NeRF.py:249-339): layer 0 has 3 + 6 n_pos_enc_xyz inputs, the view-direction
                               * block 2 n_pos_enc_view_dir (n_angles + 1). */
    float leaky_relu_alpha;   /* leaky_relu_alpha    (0.05) */
    float near_boundary;      /* NeRF.near_boundary, src/NeRF.py:45 */
    float far_boundary;       /* NeRF.far_boundary,  src/NeRF.py:46 */
    int32_t precision;        /* NERF_PRECISION_*    */
    int32_t device;           /* HIP device ordinal  */
} nerf_config;

/* Output set of render_rays()/render(); any pointer may be NULL (= not wanted).
 * Shapes for N rays and S samples of the LAST pass (S = Sc if no fine net, else Sc+Sf). */
typedef struct nerf_outputs {
    float* rgb;          /* (N,3)   render_result           src/UtilsNRF.py:114  */
    float* weights;      /* (N,S)   alpha * cumprod         :113                 */
    float* cumprod;      /* (N,S)   exclusive transmittance :112                 */
    float* alpha;        /* (N,S)                           :111                 */
    float* rgb_samples;  /* (N,S,3) sigmoid(net rgb)        :101                 */
    float* z;            /* (N,S)   sample depths           src/NeRF.py:132-134  */
    float* depth;        /* (N)     sum_s w*z               src/ExecutionRun.py:346 (optional 7th) */
} nerf_outputs;

typedef struct nerf_ctx nerf_ctx;

/* ---- lifecycle --------------------------------------------------------------------------- */
int nerf_abi_version(void);
const char* nerf_last_error(void);
/* replaces NeRF.__init__/init_network (src/NeRF.py:27-79): validates cfg, creates stream + arena */
int nerf_ctx_create(const nerf_config* cfg, nerf_ctx** out);
void nerf_ctx_destroy(nerf_ctx* ctx);
int nerf_ctx_synchronize(nerf_ctx* ctx);
/* run on a caller-owned hipStream_t (e.g. torch's current stream; NULL = HIP's default stream);
 * NERF_STREAM_OWN restores the ctx's own stream */
#define NERF_STREAM_OWN ((void*)(intptr_t)-1)
int nerf_ctx_set_stream(nerf_ctx* ctx, void* hip_stream);
/* change the frustum (near/far) or precision after creation */
int nerf_ctx_set_bounds(nerf_ctx* ctx, float near_boundary, float far_boundary);
int nerf_ctx_set_precision(nerf_ctx* ctx, int precision);
/* ABI 6+, forward-facing scenes.  A new ctx is NERF_SAMPLING_LINEAR / NERF_RAYS_WORLD: the reference's behaviour.
 * nerf_ctx_set_sampling: NERF_SAMPLING_LINDISP draws the coarse depths of EVERY call that draws them (nerf_get_z_values,
 * nerf_render, nerf_render_image and the sharded calls, nerf_train_step / _gradients, nerf_train_render_*) as
 *   z = 1 / (1/near + (1/far - 1/near) (s + u) / S),   near <= z < far,
 * with the draws u the linear mode would use.  It needs near_boundary > 0: the setter, and later any of those calls
 * (the bounds may change in between), fail with "lindisp needs near_boundary > 0".
 * nerf_ctx_set_ray_space: NERF_RAYS_NDC makes the calls that generate rays from a camera -- nerf_render_image,
 * nerf_render_image_sharded, nerf_render_image_sharded_outputs -- pass them through the transform of nerf_rays_to_ndc
 * (same fov, this ndc_near_plane > 0) before they render.  In NDC the scene lies between 0 and 1 along every ray: the
 * caller sets that with nerf_ctx_set_bounds(ctx, 0, 1).  Calls that take rays (nerf_render, the trainer) render what they
 * are given; nerf_get_rays_directions stays world-space.  ndc_near_plane is ignored for NERF_RAYS_WORLD. */
int nerf_ctx_set_sampling(nerf_ctx* ctx, int mode);
int nerf_ctx_set_ray_space(nerf_ctx* ctx, int space, float ndc_near_plane);
/* ABI 6+, scene box: an optional axis-aligned box lo[3] < hi[3] gives every ray its own depth range.  A new ctx has none
 * (NULL, NULL turns it off again), and without one nothing changes.  The box lives in the space of the rays the depth
 * kernel is given: world rays, or NDC rays under NERF_RAYS_NDC (nerf_render_image applies it AFTER the transform).
 * For a ray (o, d) depths are the parameter t of o + t d, as everywhere here; d is not normalised.  In float32, every
 * operation rounded on its own:
 *   1. per axis a with d_a != 0: t0 = (lo_a - o_a) / d_a, t1 = (hi_a - o_a) / d_a, axis interval [min(t0,t1), max(t0,t1)];
 *   2. per axis with d_a == 0 (either sign of zero): no constraint if lo_a <= o_a <= hi_a, otherwise the ray MISSES
 *      (a branch: a ray that runs along a face of the box is inside);
 *   3. tn = the largest lower end, tf = the smallest upper end, a = max(tn, near), b = min(tf, far);
 *   4. the ray HITS if no axis said "misses" and b > a; it is NARROWED if it hits and (a > near or b < far);
 *   5. a narrowed ray draws its coarse depths with the sampling mode's own formula on [a, b], constants computed per ray:
 *      linear   z = linspace(a, b, S)[s] + (u (b - a)) / S  (first and last linspace entries exactly a and b; as with
 *               near / far the last stratum may pass b, by up to (b - a) / S),
 *      lindisp  z = 1 / (1/a + (1/b - 1/a) (s + u) / S), held in [a, b)  (a >= near > 0 keeps it legal);
 *   6. a ray that is not narrowed -- it misses, or the box contains its whole [near, far] -- draws exactly the depths of a
 *      ctx without a box, bit for bit.  A miss is not an error and produces no special value.
 * Every call that draws coarse depths and has rays follows the box: nerf_get_z_values_rays, nerf_render,
 * nerf_render_image and both sharded calls, nerf_train_step / nerf_train_gradients, nerf_train_render_gradients and
 * nerf_train_render_forward (a slot records the depths it drew: its backward pass uses them whatever the box is by then).
 * nerf_get_z_values has no rays and nerf_render_rays takes the depths from its caller: both ignore the box.  Fine
 * sampling, compositing, the networks and the backward pass consume the depths and are unchanged.
 * The setter refuses non-finite values and lo_a >= hi_a ("scene box needs finite lo < hi on every axis"). */
int nerf_ctx_set_scene_box(nerf_ctx* ctx, const float* lo3, const float* hi3);
/* ABI 6+, occupancy grid: R x R x R bits over the scene box say where the network has density; a ray is then sampled from
 * the first occupied cell it enters to the last one it leaves, at the same sample count.  Off by default.  A grid needs a
 * box ("an occupancy grid needs a scene box"), and setting, changing or clearing the box drops the grid.  R is a multiple
 * of 4 in [4, 256]; cell (ix, iy, iz) is bit ix + R (iy + R iz) of a little-endian uint32 array of R^3 / 32 words.
 * The ray rule, in float32, every operation rounded on its own (no FMA):
 *   1. (a0, b0) = steps 1-3 of the box rule (the ray clipped to the box and to near / far).  No hit (an axis said
 *      "misses", or not b0 > a0): the ray is untouched, state 0.
 *   2. cell_a = (hi_a - lo_a) / R; the start cell per axis is clamp(floor(((o_a + a0 d_a) - lo_a) / cell_a), 0, R - 1).
 *   3. plane k of an axis lies at t = ((lo_a + cell_a k) - o_a) / d_a, recomputed from k at every step, never accumulated;
 *      the first plane of an axis is k = cell + 1 for d_a > 0, k = cell for d_a < 0; an axis with d_a == 0 never steps.
 *   4. Amanatides-Woo walk from t = a0: the next axis is the one with the smallest plane parameter tm (ties: the lowest
 *      axis index, strict <); the current cell's segment is [t, te], te = tm held in [t, b0]; an occupied cell sets a' = t
 *      the first time and b' = te every time; the walk stops when tm reaches b0 (not tm < b0), when the stepped index
 *      leaves the grid, or after 3R + 3 steps; otherwise t = te and the walk goes on in the next cell.
 *   5. if an occupied cell was met, b' > a' (as the box rule asks b > a of a hit: cells touched in one point do not
 *      count) and a' > a0 or b' < b0 (as the box rule asks a > near or b < far of "narrowed": a grid that is full along the
 *      ray is the box alone), the ray is NARROWED BY THE GRID to [a', b'], state 2, and draws its depths by the box rule's
 *      step 5 on that interval (linear and lindisp alike; a' >= near > 0 keeps lindisp legal).
 *   6. otherwise the ray keeps exactly what a ctx with the box alone gives it, bit for bit: state 1 and (a0, b0) if the box
 *      narrows it, state 0 and (near, far) if not.  Nothing is ever left unsampled.
 * Every call listed under the scene box follows the grid; a training slot keeps the depths it drew.  nerf_ray_box_bounds
 * and nerf_get_z_values keep their meaning.  The library never rebuilds a grid on its own: it is the caller's snapshot of
 * the network, and training on with a stale grid is the caller's choice.
 * set: `bits` is a HOST pointer to R^3 / 32 words (copied before the call returns); NULL, 0 clears the grid.
 * get: writes *R = 0 when there is no grid; bits (HOST, R^3 / 32 words) may be NULL to ask for R only. */
int nerf_ctx_set_occupancy_grid(nerf_ctx* ctx, const uint32_t* bits, int32_t R);
int nerf_ctx_get_occupancy_grid(nerf_ctx* ctx, uint32_t* bits, int32_t* R);
/* ABI 6+: bake the grid from network `which` (0 coarse / 1 fine) in the ctx's precision: a cell is occupied if sigma (raw
 * column 3 of nerf_model_predict, the same kernels) exceeds sigma_threshold at any of its samples_per_cell points (1..8):
 * point 0 is the float32 centre lo_a + cell_a (i_a + 0.5), further points are Philox-jittered inside the cell (seed).  The
 * set is then grown by `dilate` cells (0..2, 26-neighbourhood).  *n_occupied (nullable) = the occupied cells afterwards.
 * Fails without a box, if the network is not loaded, if sigma_threshold is not finite and > 0, if samples_per_cell is
 * outside 1..8; a bake that fails leaves the ctx without a grid. */
int nerf_occupancy_bake(nerf_ctx* ctx, int which, int32_t R, float sigma_threshold, int32_t samples_per_cell, int32_t dilate,
                        uint64_t seed, int64_t* n_occupied);

/* ---- ABI 6+, a triangle mesh out of the density field ---------------------------------------------------------------------
 * nerf_density_lattice: raw sigma (column 3 of nerf_model_predict before the ReLU, the same kernels, the ctx's precision) of
 * network `which` at the n^3 lattice points of the scene box, n in 2..512.  Point (ix, iy, iz) is element
 * ix + n (iy + n iz) of sigma (n, n, n); its position is p_a = lo_a + step_a * float(i_a), step_a = (hi_a - lo_a) / float(n - 1),
 * in float32, every operation rounded on its own (no FMA).  view_dir3 (HOST, 3 floats) is the view direction of every point,
 * NULL = (0, 0, 1) as in the bake; it is ignored for n_angles == 0.  The points go through the network in chunks of at most
 * 2^20.  Fails without a box ("a density lattice needs a scene box"), if the network is not loaded, or if n is outside 2..512. */
int nerf_density_lattice(nerf_ctx* ctx, int which, int32_t n, const float* view_dir3, float* sigma, int mem);
/* nerf_isosurface: the surface s = iso of a volume s (n, n, n), n in 2..512, laid out and placed as above on the box lo3 < hi3
 * (HOST, explicit: the volume need not come from a network), as an indexed triangle mesh by marching tetrahedra on the
 * 6-tetrahedra split of every cube along its (0,0,0)-(1,1,1) diagonal.  Neighbouring cubes agree on every face diagonal, so
 * the mesh is closed wherever the surface does not leave the lattice.  The result is canonical (no atomics, no hashing):
 *   Inside.    A point is inside iff s > iso; NaN is outside.  iso must be finite.
 *   Edges.     Every tetrahedron edge runs from a lattice point p to p + e, e one of 7 types, in this order:
 *              100, 010, 001, 110, 011, 101, 111 (x, y, z offsets).
 *   Vertices.  An edge whose ends differ in "inside" carries exactly one vertex; vertices are numbered in increasing order of
 *              key = 7 * pointindex(p) + type.  Position, per axis: p0 + t (p1 - p0) with p0, p1 the positions of p and p + e
 *              and t = (iso - s0) / (s1 - s0), s0 = s(p); float32, separate operations; a t that is not finite is 0.5.
 *   Triangles. Cubes are visited in order cx + (n - 1) (cy + (n - 1) cz), the tetrahedra of a cube in lexicographic order of
 *              the axis permutation (a, b, c): 012, 021, 102, 120, 201, 210; corners c0 = cube base, c1 = c0 + e_a,
 *              c2 = c1 + e_b, c3 = c2 + e_c.  One or three corners inside: one triangle on the three edges at the odd corner,
 *              in corner order.  Two inside (I0, I1) and two outside (O0, O1), each pair in corner order: the quad
 *              (I0O0, I0O1, I1O1, I1O0).  The polygon is oriented counter-clockwise seen from the outside (normal from inside
 *              to outside), decided from the case and the permutation's parity alone, never from positions: where a lattice
 *              value equals iso, vertices coincide and triangles have zero area.  It is then rotated so that its lowest
 *              vertex id comes first and emitted as (q0, q1, q2) and, for a quad, (q0, q2, q3).
 *   Normals.   Gradient at a lattice point, per axis: (s[i + 1] - s[i - 1]) / (2 step_a), at the faces the one-sided
 *              difference over step_a.  At a vertex g = g0 + t (g1 - g0); the normal is -g / |g|,
 *              |g| = sqrt((gx gx + gy gy) + gz gz), or (0, 0, 0) when |g| is 0 or not finite.
 * The counts are not known in advance, so there are two calls: the first builds the mesh in the ctx's arena and returns the
 * counts (both always fit int32 for n <= 512; a count that did not would fail the call), the second copies it out: vertices
 * (V, 3) float32, normals (V, 3) float32 or NULL, triangles (T, 3) int32; `mem` says where the call's own arrays live.  The
 * mesh stays until the next first call (which replaces it, and leaves none if it fails) or nerf_ctx_destroy; a fetch without
 * one fails ("no pending mesh").  With 0 vertices the fetch succeeds and writes nothing. */
int nerf_isosurface(nerf_ctx* ctx, const float* sigma, int32_t n, const float* lo3, const float* hi3, float iso,
                    int64_t* n_vertices, int64_t* n_triangles, int mem);
int nerf_isosurface_fetch(nerf_ctx* ctx, float* vertices, float* normals, int32_t* triangles, int mem);
/* nerf_mesh_colors: network `which` at V vertices, seen against their normals -- view direction -normal, a ray that sees the
 * surface travels against its normal; a zero normal uses (0, 0, 1) -- through the sigmoid nerf_ray_marching applies for
 * rgb_samples.  vertices, normals, rgb: (V, 3).  The directions are ignored for n_angles == 0. */
int nerf_mesh_colors(nerf_ctx* ctx, int which, const float* vertices, const float* normals, int64_t V, float* rgb, int mem);

/* ---- ABI 6+, a radiance volume: the network baked to an RGB-sigma lattice, and the lattice ray-marched ---------------------
 * The volume is an (n, n, n, 4) float32 array indexed [iz, iy, ix, channel], n in 2..512, over a box lo3 < hi3: vertex i of axis
 * a lies at lo_a + step_a * float(i), step_a = (hi_a - lo_a) / float(n - 1), as in nerf_density_lattice.  Channels 0..2 are the
 * colour after the sigmoid (as nerf_mesh_colors writes it), channel 3 the density after the ReLU, fmaxf(raw sigma, 0) (as
 * nerf_ray_marching takes it).  16 bytes a vertex: 256 MiB at n = 256, 2 GiB at n = 512.  A volume is a snapshot of one
 * network under one view direction (or one camera); nothing rebuilds it, and it is no parity mode of the renderer.
 *
 * nerf_radiance_lattice: nerf_density_lattice with all four channels -- the same checks, chunks, kernels, the ctx's precision
 * and encoding window.  At most one of view_dir3 (HOST, 3 floats) and camera_c2w16 (HOST, row-major 4x4 as nerf_render_image
 * takes it) may be given.  Neither: direction (0, 0, 1) at every vertex, as the density lattice and the occupancy bake.
 * view_dir3: that direction at every vertex.  camera_c2w16: every vertex p gets the direction the ray generator gives the pixel
 * whose ray passes through p: q = p - t with t = (c[3], c[7], c[11]); s = -((c[2] q_x + c[6] q_y) + c[10] q_z), float32, every
 * operation rounded on its own; the direction is q / s (one division per component) if s > 0 and finite, otherwise that of the
 * central ray, (-c[2], -c[6], -c[10]).  A camera is refused while the ctx's ray space is NDC (the box is then not in world
 * space).  Directions are ignored for n_angles == 0.  Fails without a box ("a radiance lattice needs a scene box"), if the
 * network is not loaded, if n is outside 2..512, if both view_dir3 and camera_c2w16 are given. */
int nerf_radiance_lattice(nerf_ctx* ctx, int which, int32_t n, const float* view_dir3, const float* camera_c2w16, float* volume,
                          int mem);
/* nerf_volume_sample: the volume at M points (M, 3) -> out (M, 4), trilinear, one thread per point; lo3, hi3 HOST.  float32,
 * every operation rounded on its own, no FMA.  Per axis: g = (p - lo) / step; the cell i = g >= 0 ? (g < n - 1 ? (int)floor(g)
 * : n - 2) : 0, so a NaN lands in cell 0; f = g - float(i), clamped to [0, 1] by comparisons (a NaN stays).  The cell is in
 * [0, n - 2] wherever the volume is read: no input, finite or not, reads outside the array.  Per channel, along x first,
 * v00 = v000 + f_x (v100 - v000) (subtract, multiply, add), then along y, then along z.  A point outside the box takes the
 * value of the nearest face; a NaN coordinate gives NaN. */
int nerf_volume_sample(nerf_ctx* ctx, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* points,
                       int64_t M, float* out, int mem);
/* nerf_volume_march: N rays (N, 4) through the volume.  rgb (N, 3), depth (N), opacity (N): any may be NULL, not all three.
 * n_steps >= 1, t_min in [0, 1).  Per ray, float32, every operation rounded on its own, sequentially in k:
 *   1. (hit, a, b) = the scene-box rule (nerf_ctx_set_scene_box, steps 1-4) on the box (lo3, hi3) and the ctx's near / far.
 *      A ray with a non-finite component in its origin or direction is a miss.
 *   2. No hit: rgb, depth and opacity are exact zeros.
 *   3. D = (b - a) / float(n_steps), T = 1, sums 0.
 *   4. k = 0 .. n_steps - 1: z_k = a + (float(k) + 0.5) D; p = o + d z_k; v = nerf_volume_sample's value at p;
 *      e = expf(-(v.sigma D)), alpha = 1 - e, w = alpha T; rgb += w v.rgb (multiply, add); depth += w z_k;
 *      T = T (1 - alpha); if T < t_min the ray stops after this step.
 *   5. opacity = 1 - T.
 * There is no 1e9 last interval: a ray may leave the box partly transparent, rgb is premultiplied, and blending it over a
 * background by opacity is the caller's business.  D is in units of the ray parameter, like the network render's intervals
 * (no |d| factor), so the density scale is the network's.  Stopping at t_min changes rgb and opacity by at most t_min and depth
 * by at most t_min b (the dropped tail carries total weight T < t_min). */
int nerf_volume_march(nerf_ctx* ctx, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* rays_orig,
                      const float* rays_dirs, int64_t N, int32_t n_steps, float t_min, float* rgb, float* depth, float* opacity,
                      int mem);
/* nerf_volume_render_image: the march of the rays nerf_render_image prepares for the slab [ray_begin, +ray_count) of an H x W
 * image (ray_count <= 0: the whole image) -- the ray generator and, on an NDC ctx, nerf_rays_to_ndc -- made on the device in
 * batches; the results equal nerf_get_rays_directions (+ nerf_rays_to_ndc) + nerf_volume_march bit for bit. */
int nerf_volume_render_image(nerf_ctx* ctx, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* c2w,
                             float fov, int32_t H, int32_t W, int64_t ray_begin, int64_t ray_count, int32_t n_steps, float t_min,
                             float* rgb, float* depth, float* opacity, int mem);

/* ---- ABI 6+, view-dependent colour in the radiance volume: spherical harmonics per vertex (additive entry points) ----------
 * The format.  Degree L in 0..3, K = (L + 1)^2 basis functions.  A texel is C(L) = 4 ceil((3 K + 1) / 4) float32 -- 4 / 16 /
 * 28 / 52 for L = 0 / 1 / 2 / 3 -- so every texel is 16-byte aligned.  Channel 3 k + c holds the coefficient of basis
 * function k for colour channel c (k < K, c < 3), channel 3 K the density after the ReLU, fmaxf(raw sigma, 0); the channels
 * after it are exact zeros.  The volume is (n, n, n, C(L)) float32 indexed [iz, iy, ix, channel] on the lattice of
 * nerf_radiance_lattice, n in 2..512: n^3 C(L) 4 bytes, 1.75 GiB at n = 256, L = 2.  Coefficients are in the colour domain
 * (after the sigmoid, not logits); the colour towards u is clamp(sum_k Y_k(u) coef_k, 0, 1), the clamp by comparisons
 * (x < 0 ? 0 : x > 1 ? 1 : x: a NaN stays NaN).  A degree-L volume whose coefficients above degree L' < L are +0 gives the
 * bits of the degree-L' volume with the same (finite) coefficients: the extra terms add +-0 to sums that are not -0.
 *   Basis.     Real, orthonormal on the sphere, u = (x, y, z), float32, the constants rounded to float32, every operation
 *              rounded on its own, no FMA, in exactly this order (xx = x x, yy = y y, zz = z z, xy = x y, yz = y z, xz = x z):
 *                Y0  = 0.28209479177387814
 *                Y1  = 0.4886025119029199 y             Y2  = 0.4886025119029199 z          Y3 = 0.4886025119029199 x
 *                Y4  = 1.0925484305920792 xy            Y5  = 1.0925484305920792 yz
 *                Y6  = 0.31539156525252005 ((3 zz) - 1) Y7  = 1.0925484305920792 xz
 *                Y8  = 0.5462742152960396 (xx - yy)
 *                Y9  = 0.5900435899266435 (y ((3 xx) - yy))       Y10 = 2.890611442640554 (xy z)
 *                Y11 = 0.4570457994644658 (y ((5 zz) - 1))        Y12 = 0.3731763325901154 (z ((5 zz) - 3))
 *                Y13 = 0.4570457994644658 (x ((5 zz) - 1))        Y14 = 1.445305721320277 (z (xx - yy))
 *                Y15 = 0.5900435899266435 (x (xx - (3 yy)))
 *   Direction. u = d / |d|: s = (d_x d_x + d_y d_y) + d_z d_z, r = sqrt(s) correctly rounded, one correctly-rounded division
 *              per component.  If s is 0 or not finite (a zero, NaN, Inf or overflowing d), u = (0, 0, 1).
 *   Limits.    The volume answers for d / |d|, while the ray generator's directions have length 1 / cos of the angle to the
 *              optical axis and the network sees that length.  A fit over the full sphere includes directions no camera saw.
 *              Like every volume it is a snapshot of one network: nothing rebuilds it.
 *
 * nerf_sh_radiance_lattice: the bake.  dirs (D, 3) and proj (K, D), both HOST, D in 1..64, are the caller's projection table.
 * For every vertex the network `which` is evaluated at the D directions dirs[j] exactly as given (the network takes raw
 * directions: their length is the caller's choice), by the chunk loop and kernels of nerf_radiance_lattice -- the ctx's
 * precision, encoding window and n_angles act as there; for n_angles == 0 the directions are ignored and the same path runs.
 * colour_j[c] = the sigmoid of raw_j[c] as nerf_mesh_colors writes it; coef[k][c] = proj[k][0] colour_0[c], then
 * + proj[k][j] colour_j[c] for j = 1 .. D - 1 in that order, each multiply and each add rounded on its own; sigma =
 * fmaxf(raw_0[3], 0).  A pass through the network takes max(1, floor(2^20 / D)) vertices (D points each).  The table is kept
 * in a device buffer of the ctx for the duration of the call.
 *   The default table (what the Python helper sh_quadrature builds): the L + 1 Gauss-Legendre nodes in cos(theta) times
 *   2 L + 1 equally spaced azimuths phi_m = (m + 1/2) 2 pi / (2 L + 1), node-major, D = 1 / 6 / 15 / 28, unit directions
 *   (sin(theta) cos(phi), sin(theta) sin(phi), cos(theta)); proj[k][j] = q_j Y_k(dirs_j) with q_j = 2 pi w_node / (2 L + 1),
 *   in float64, rounded once.  It is exact for the products Y_k Y_k' up to degree L.
 * Fails, in this order: which not 0 or 1; no scene box ("an SH radiance lattice needs a scene box"); n outside 2..512; degree
 * outside 0..3; D outside 1..64; a NULL table; a non-finite entry of dirs or proj; an all-zero direction; network not loaded. */
int nerf_sh_radiance_lattice(nerf_ctx* ctx, int which, int32_t n, int32_t degree, const float* dirs, const float* proj,
                             int32_t D, float* volume, int mem);
/* nerf_sh_volume_sample: the SH volume at M points (M, 3) seen along dirs (M, 3) -> out (M, 4) = (r, g, b, sigma).  The cell
 * and the weights are nerf_volume_sample's (the cell index is in [0, n - 2] for every input).  u and Y_k from dirs as above.
 * At each of the cell's 8 vertices colour_c = Y_0 coef_0c, then + Y_k coef_kc for k = 1 .. K - 1 in order (multiply, add); the
 * four values (r, g, b, sigma) are interpolated along x, then y, then z as in nerf_volume_sample; the colour is then clamped. */
int nerf_sh_volume_sample(nerf_ctx* ctx, const float* volume, int32_t n, int32_t degree, const float* lo3, const float* hi3,
                          const float* points, const float* dirs, int64_t M, float* out, int mem);
/* nerf_sh_volume_march: nerf_volume_march with nerf_sh_volume_sample's value in step 4, u and Y_k computed once per ray from
 * the ray's direction.  Non-finite rays are misses, misses give exact zeros, t_min acts as there.
 * nerf_sh_volume_render_image: nerf_volume_render_image likewise.  One lane works on a ray at degrees 0 and 1, eight lanes
 * (one cell vertex each) at degrees 2 and 3; the results do not depend on that (profiles/sh_volume_measure.json has both). */
int nerf_sh_volume_march(nerf_ctx* ctx, const float* volume, int32_t n, int32_t degree, const float* lo3, const float* hi3,
                         const float* rays_orig, const float* rays_dirs, int64_t N, int32_t n_steps, float t_min, float* rgb,
                         float* depth, float* opacity, int mem);
int nerf_sh_volume_render_image(nerf_ctx* ctx, const float* volume, int32_t n, int32_t degree, const float* lo3,
                                const float* hi3, const float* c2w, float fov, int32_t H, int32_t W, int64_t ray_begin,
                                int64_t ray_count, int32_t n_steps, float t_min, float* rgb, float* depth, float* opacity,
                                int mem);

/* replaces Keras load_weights / model.get_weights() order (src/ExecutionRun.py:228-231):
 * `blob` = the 22 tensors of one network, kernel(in,out) row-major then bias, layer order of
 * src/NeRF.py:319-337 (dense .. dense_10).  HOST pointer.  n_floats must equal nerf_blob_size(). */
size_t nerf_blob_size(const nerf_config* cfg);
int nerf_load_weights(nerf_ctx* ctx, int which, const float* blob, size_t n_floats);

/* Coarse-to-fine positional encoding (additive entry points; the ABI version does not move): a weight in [0, 1] on every
 * octave of the two sinusoidal encodings, as BARF opens them from low to high frequency and FreeNeRF masks them.  Under a
 * window every network evaluation of the library -- every render and predict entry, the lattice, the bake, the vertex colours,
 * every trainer pass -- sees, per component c,
 *     xyz:  [ x_c, w_xyz[0] sin(2^0 pi x_c), w_xyz[0] cos(2^0 pi x_c), ..., w_xyz[L-1] sin(.), w_xyz[L-1] cos(.) ]
 *     dir:  [ w_dir[0] sin, w_dir[0] cos, ... ]
 * and the pass-through component always has weight 1.  nerf_positional_encoding, the bare operator, stays unwindowed.
 * How: the encoding only ever enters a dense layer, so the weight of octave k is folded into the rows of that octave in
 * layers 0 and 4 (xyz) and 8 and 10 (directions) while the kernels' operand streams are packed -- every packed weight is
 * fl32(weight * w), split or rounded as before -- the master weights are never scaled: nerf_get_weights, checkpoints and
 * Adam's moments stay in the unwindowed parametrisation, and gradients are with respect to the master weights: what the
 * gradient entry points return, the optimizer applies and the data-parallel all-reduce sums is w times the gradient the
 * kernels compute with respect to the windowed weights, applied to the contribution of the call at hand only (accumulated
 * gradients are not rescaled; under mixed_float16 the loss-scale verdict is unchanged).  A row with weight 0 is not trained.
 * w_xyz: n_pos_enc_xyz values, w_dir: n_pos_enc_dir values, HOST pointers; NULL = all ones.  A value that is not finite or
 * outside [0, 1] fails and names its index.  w_dir on an n_angles = 0 context is accepted and has no effect.  All ones, or
 * two NULLs, is "off": the library then launches exactly what it launches without a window.
 * The window belongs to the context: it survives nerf_train_begin, nerf_train_end, nerf_load_weights and the slot calls.
 * Setting it re-packs what exists (the render streams of loaded networks, both networks of a running trainer) on the context's
 * stream, without a synchronise.  It fails while a render slot holds a forward pass (nerf_train_render_forward without its
 * backward): a slot's backward must run under the window of its forward.  An occupancy grid is kept: it is a snapshot of the
 * network as windowed when it was baked.  Data-parallel ranks must each be given the same window.
 * nerf_ctx_get_encoding_window: the weights in force (ones when off; either pointer may be NULL) and whether a window is on. */
int nerf_ctx_set_encoding_window(nerf_ctx* ctx, const float* w_xyz, const float* w_dir);
int nerf_ctx_get_encoding_window(nerf_ctx* ctx, float* w_xyz, float* w_dir, int32_t* active);

/* ---- the functions on the path, one entry each ---------------------- */
/* get_rays_directions, src/UtilsCV.py:467-499.  c2w row-major (4,4) HOST; dirs (H*W,4). */
int nerf_get_rays_directions(nerf_ctx* ctx, const float* c2w, float fov, int32_t H, int32_t W,
                             float* dirs, int mem);
/* ABI 6+: world rays -> NDC rays, for callers that bring their own rays (nerf_render, the trainer, a ray dataset).  The
 * reference carries this transform as dead code only.  Cameras look down -z; the near plane is z = -ndc_near_plane; fov is
 * the field of view the rays were generated with: get_rays_directions uses ONE tangent for both axes and no aspect term,
 * so both NDC scale factors are k = 1 / tan(fov / 2).  With tn = -(n + o_z) / d_z and p = o + tn d (the origin moved onto
 * the near plane):
 *   o' = (-k p_x / p_z, -k p_y / p_z, 1 + 2n / p_z)                                     -- o'_z = -1
 *   d' = (-k (d_x / d_z - p_x / p_z), -k (d_y / d_z - p_y / p_z), -2n / p_z)            -- (o' + d')_z = +1: infinity
 * w components are copied.  [n, infinity) along the world ray becomes [0, 1) along the NDC ray.  A ray with d_z == 0
 * comes out non-finite (not guarded).  rays (N,4) in, (N,4) out; in place is allowed as out_orig == rays_orig AND
 * out_dirs == rays_dirs.  The fused kernels take the view direction from the direction they are given: under NDC that is
 * d', not the world direction (no difference for n_angles 0). */
int nerf_rays_to_ndc(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, int64_t N, float fov,
                     float ndc_near_plane, float* out_orig, float* out_dirs, int mem);
/* get_z_values(near,far,N,1,S)[:,0,:], src/UtilsCV.py:565-581.  u (N,S) uniform draws or NULL
 * (= on-device Philox keyed by seed and global ray index ray_base+r).  z (N,S).  Follows nerf_ctx_set_sampling.  It has
 * no rays, so it IGNORES the scene box: nerf_get_z_values_rays is the call that follows it. */
int nerf_get_z_values(nerf_ctx* ctx, int64_t N, int32_t S, const float* u, uint64_t seed,
                      int64_t ray_base, float* z, int mem);
/* ABI 6+: nerf_get_z_values for callers that have rays (N,4): the coarse depths nerf_render and the trainer draw for them,
 * following the sampling mode AND the scene box (without a box: exactly nerf_get_z_values). */
int nerf_get_z_values_rays(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, int64_t N, int32_t S,
                           const float* u, uint64_t seed, int64_t ray_base, float* z, int mem);
/* ABI 6+: steps 1-4 of nerf_ctx_set_scene_box for N rays, from the device function the depth kernels call.
 * bounds (N,2): (a, b) of a narrowed ray, (near, far) of any other; narrowed (N) int32 0 / 1, or NULL.  Fails without a box. */
int nerf_ray_box_bounds(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, int64_t N, float* bounds,
                        int32_t* narrowed, int mem);
/* ABI 6+: the occupancy-grid rule for N rays, from the device function the depth kernels call.  bounds (N,2): (a', b') of
 * a ray the grid narrows, (a0, b0) of one only the box narrows, (near, far) of any other; state (N) int32 2 / 1 / 0, or
 * NULL.  Fails without a grid. */
int nerf_ray_occupancy_bounds(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, int64_t N, float* bounds,
                              int32_t* state, int mem);
/* ABI 6+, sample culling: under an occupancy grid, the samples of a render pass that lie in EMPTY cells skip the network.
 * Off by default.  The flag may be set with or without a grid and acts only while the ctx holds one; dropping the grid (a new
 * box, nerf_ctx_set_occupancy_grid(NULL, 0)) leaves the flag as it is.  The rule for sample (ray, s), in float32, every
 * operation rounded on its own (no FMA), comparisons instead of fmin / fmax:
 *   1. p_a = o_a + d_a z, multiply then add: the point the network kernels form themselves.
 *   2. inside = lo_a <= p_a <= hi_a on all three axes; a NaN compares false, so the sample is not inside.
 *   3. i_a = clamp(floor((p_a - lo_a) / cell_a), 0, R - 1), cell_a = (hi_a - lo_a) / R (step 2 of the grid rule): a point on
 *      the hi face belongs to cell R - 1, a point on an interior cell face to the upper cell.
 *   4. the sample is CULLED iff inside and bit i_x + R (i_y + R i_z) is 0.  Every other sample is KEPT: the grid knows
 *      nothing outside the box, and a ray that misses the box renders as before, bit for bit.
 * A culled sample has the raw network output (0, 0, 0, 0): alpha and weight exactly 0, the transmittance untouched,
 * rgb_samples = sigmoid(0).  The kept samples run through the same network kernels as compacted rows in ascending sample
 * index (no atomics: the result does not depend on the launch).  The host reads the row count of every pass (one 4-byte copy
 * and a stream synchronise per network pass), so a culled render call is not asynchronous.  A culled pass counts its rows in
 * 32 bits: a nerf_render_rays / nerf_render call with N * S above 2^31 - 1 samples in one pass fails under the flag where it
 * would run without it (nerf_render_image batches its rays and stays far below).
 * nerf_render_rays, nerf_render, nerf_render_image and the sharded calls follow the flag.  nerf_train_* (one-call and slot
 * paths, so DietNeRF's consistency render too) IGNORE it: the trainer has a switch of its own,
 * nerf_ctx_set_train_sample_culling. */
int nerf_ctx_set_sample_culling(nerf_ctx* ctx, int on);
/* ABI 6+, sample culling in the TRAINER: a separate switch, off by default, independent of nerf_ctx_set_sample_culling (which
 * the trainer keeps ignoring).  It may be set with or without a grid and with or without a running trainer, acts only while
 * the ctx holds a grid, survives the grid being dropped, and nerf_train_begin does not reset it.  Under it the network passes
 * of every training entry point -- nerf_train_step (the data-parallel step included: ranks may keep different row counts, only
 * the gradient blobs are reduced), nerf_train_gradients, nerf_train_render_gradients, nerf_train_render_forward / _backward
 * and so DietNeRF's consistency render -- run on the kept samples only, forward and backward:
 *   - The verdict for a sample is exactly steps 1-4 of nerf_ctx_set_sample_culling, from the same device function, evaluated
 *     on the depths the pass actually runs on: the coarse depths; in nerf_train_step / nerf_train_gradients the Sf new fine
 *     depths; in the render-gradient paths the Sc + Sf merged depths.
 *   - A culled sample has the raw network output (0, 0, 0, 0) as a CONSTANT: it is never a network row, forward or backward,
 *     contributes nothing to any weight gradient and nothing to dL/dz through the network input.  The verdict is piecewise
 *     constant in z and carries no gradient.
 *   - Compositing and its backward pass run on all N * S samples as without the flag; the compositing's own dL/dz terms
 *     (through the deltas) stay.
 *   - The kept samples are compacted rows in ascending sample index (no atomics).  Rows are independent in every kernel
 *     involved, so under a grid that is full the losses and gradients are bit-identical to the flag being off.
 *   - A pass keeps its compaction record (verdict bits, scan offsets, row count) with its activations: the backward half uses
 *     exactly the rows the forward half made, and a slot of nerf_train_render_forward keeps the record as it keeps its depths
 *     -- its backward pass does not depend on what the flag or the grid are by then.
 *   - A pass that keeps no row launches no network kernel and contributes exact zeros to that network's gradient (stored or
 *     accumulated as the call asks); loss, metrics, the mixed_float16 verdict and Adam behave as for any finite step.
 *   - Culled cells receive NO gradient: density can reappear there only through a re-bake of the grid with dilation.
 * The host reads the row count of every network pass (one 4-byte copy and a stream synchronise per pass, two per step with a
 * fine network): a culled training call is NOT asynchronous -- "the step never waits for the GPU" holds only with the flag
 * off.  Row counts are 32-bit: a pass with N * S above 2^31 - 1 samples fails under the flag with the render path's message.
 * Passes run this way add to the counters of nerf_ctx_read_culling (samples seen, rows run). */
int nerf_ctx_set_train_sample_culling(nerf_ctx* ctx, int on);
/* The verdict of that rule for N rays x S depths z (N,S), from the device function the render path calls: keep (N,S) int32,
 * 1 kept / 0 culled.  Fails without a grid. */
int nerf_sample_occupancy(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, const float* z, int64_t N, int32_t S,
                          int32_t* keep, int mem);
/* Samples seen and samples kept, summed over all culled network passes since the last call (either may be NULL); clears both. */
int nerf_ctx_read_culling(nerf_ctx* ctx, int64_t* samples, int64_t* kept);
/* get_z_vals_from_prob_dist_func, src/UtilsCV.py:502-539.  weights,z (N,S); u (N,Sf) or NULL;
 * z_new (N,Sf) sorted.  If z_merged != NULL also writes sort(concat(z_new,z)) (N,S+Sf)
 * (src/NeRF.py:132). */
int nerf_sample_pdf(nerf_ctx* ctx, const float* weights, const float* z, int64_t N, int32_t S,
                    int32_t Sf, const float* u, uint64_t seed, int64_t ray_base, float* z_new,
                    float* z_merged, int mem);
/* positional_encoding_for_xyz / _for_views, src/UtilsNRF.py:52-85 (standalone, for tests/tools;
 * the render path computes the encoding in-register inside the MLP kernel). x (M,3). */
int nerf_positional_encoding(nerf_ctx* ctx, const float* x, int64_t M, int32_t n_enc,
                             int32_t with_passthrough, float* out, int mem);
/* model_predict, src/UtilsNRF.py:214-234 + Keras model call src/NeRF.py:316-339.
 * xyz (M,3), view_dirs (M,3) -> raw (M,4) [r,g,b,sigma]. */
int nerf_model_predict(nerf_ctx* ctx, int which, const float* xyz, const float* view_dirs,
                       int64_t M, float* raw, int mem);
/* ray_marching, src/UtilsNRF.py:88-115.  raw (N,S,4), z (N,S). */
int nerf_ray_marching(nerf_ctx* ctx, const float* raw, const float* z, int64_t N, int32_t S,
                      const nerf_outputs* outs, int mem);
/* render_rays, src/UtilsNRF.py:181-211 (the seam NeRF.render_rays binds, src/NeRF.py:180-188). */
int nerf_render_rays(nerf_ctx* ctx, int which, const float* rays_orig, const float* rays_dirs,
                     const float* z, int64_t N, int32_t S, const nerf_outputs* outs, int mem);
/* NeRF.render, src/NeRF.py:109-134: stratified coarse pass -> inverse-CDF resample -> fine pass on
 * sort(concat).  Sf == 0 (or no fine weights loaded) = coarse only.  u_coarse (N,Sc), u_fine (N,Sf)
 * or NULL for on-device Philox(seed, ray_base + r). */
int nerf_render(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, int64_t N,
                int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                int64_t ray_base, const nerf_outputs* outs, int mem);
/* NeRF.render_image, src/NeRF.py:190-246, for the ray slab [ray_begin, ray_begin+ray_count) of the
 * row-major H*W image (ray_count <= 0 = whole image).  Outputs are slab-sized.  batch = rays per
 * internal pass (0 = library default: the whole slab up to 262144 rays; a quarter of it when per-sample outputs go to
 * host memory, so that copies overlap compute); results do not depend on it.  u_* index by GLOBAL ray. */
int nerf_render_image(nerf_ctx* ctx, const float* c2w, float fov, int32_t H, int32_t W,
                      int64_t ray_begin, int64_t ray_count, int64_t batch, int32_t Sc, int32_t Sf,
                      const float* u_coarse, const float* u_fine, uint64_t seed,
                      const nerf_outputs* outs, int mem);

/* ABI 3: page-locked (pinned) host memory for the buffers of NERF_MEM_HOST calls.  Any host memory works; with
 * buffers from nerf_host_alloc the outputs of nerf_render_image leave the device by DMA on a second stream WHILE the
 * next batch of rays computes (the reference concatenates its per-batch results at the end, src/NeRF.py:226-237), and
 * the host-memory entry point runs at the device-resident rate.  Not tied to a ctx; usable from any GPU of the node. */
int nerf_host_alloc(size_t bytes, void** out);
int nerf_host_free(void* p);

/* ---- multi-GPU assembly from C ------------------------------------------
 * One process (or thread + ctx) per GPU.  Rank 0 obtains an id and hands it to the others by any means (file, MPI,
 * a torch store); every rank then joins.  nerf_render_image_sharded renders this rank's contiguous slab of the H*W
 * rays (equal slabs of ceil(H*W/world) rays, as nerf_and_dietnerf_amd/sharding.py), all-gathers the RGB slabs with ONE
 * ncclAllGather on the ctx stream and writes the whole (H*W,3) image on every rank.  The Philox counter is the
 * global ray index: the image does not depend on the number of GPUs.  RCCL is bound at run time (dlopen); the
 * environment variable NERF_RCCL_LIB names another library with the same six nccl* entry points (a site's own RCCL
 * build; the tests' two-ranks-on-one-GPU stand-in). */
#define NERF_COMM_ID_BYTES 128
int nerf_comm_unique_id(void* id /* NERF_COMM_ID_BYTES, out */);
int nerf_comm_init(nerf_ctx* ctx, const void* id, int32_t rank, int32_t world);
int nerf_comm_destroy(nerf_ctx* ctx);
int nerf_render_image_sharded(nerf_ctx* ctx, const float* c2w, float field_of_view, int32_t H, int32_t W,
                              int64_t batch, int32_t n_coarse, int32_t n_fine, uint64_t seed,
                              float* rgb /* (H*W,3) */, int mem);
/* ABI 4: the same assembly for EVERY requested output of NeRF.render_image (src/NeRF.py:239-246) -- one ncclAllGather of
 * equal padded slabs per non-NULL pointer of `outs`; each destination holds the WHOLE image
 * ((H*W,3), (H*W,S), (H*W,S,3), (H*W) for depth; S = n_coarse + n_fine, or n_coarse without a fine network) on every
 * rank.  What the reference's video loop needs per frame is weights and z (depth = sum_s w*z, src/ExecutionRun.py:339-356)
 * -- or the fused `depth` output alone; its special ray plots take all six (:487).  Host destinations leave on the
 * ctx's copy stream, one output's copy under the next output's gather (page-locked buffers from nerf_host_alloc move by
 * DMA).  nerf_render_image_sharded is this call with rgb alone. */
int nerf_render_image_sharded_outputs(nerf_ctx* ctx, const float* c2w, float field_of_view, int32_t H, int32_t W,
                                      int64_t batch, int32_t n_coarse, int32_t n_fine, uint64_t seed,
                                      const nerf_outputs* outs, int mem);

/* ---- status ------------------------------------------------------------------------------ */
/* Synchronises and returns (then clears) the number of sample rows whose network output was not finite
 * since the last read.  NERF_PRECISION_F16X3 needs |activations| < 65504 (fp16 range); a non-zero count
 * there means: switch this model to NERF_PRECISION_BF16X3 (fp32's range: about 3.4e38; the only fp32-class mode of
 * a network with n_pos_enc_dim_xyz 6..10) or to NERF_PRECISION_FP32.  NERF_PRECISION_BF16X3 counts as well: there a
 * non-zero count means the fp32 network itself overflows or holds NaN weights.  The reference has no such check (TF
 * propagates NaN silently).
 * There is NO watch for the opposite limit of NERF_PRECISION_F16X3: activations far below 2^-4 lose their lo half to
 * fp16 subnormals and the result degrades with every value finite (figures at the enum above; final RGB of the shipped
 * checkpoint leaves 1e-4 once a layer's activations are 2^-9 of their trained size).  A zero count therefore says "no
 * overflow", not "fp32-class"; weights with very small hidden activations belong in NERF_PRECISION_BF16X3, whose error does
 * not depend on the scale. */
int nerf_ctx_read_nonfinite(nerf_ctx* ctx, int64_t* rows);

/* ---- training ---------------------------------------------------
 * Replaces NeRF.train_step (src/NeRF.py:136-178) under model.compile(optimizer=Adam(lr))
 * (src/ExecutionRun.py:226-227), fp32 policy:
 *   z = get_z_values(jitter); coarse render -> MSE; z_from_dist = inverse-CDF(weights_coarse) -- differentiated
 *   through, as the reference's tape does (no stop_gradient in src/UtilsCV.py:502-539); fine render on the
 *   Sf new samples only -> MSE; loss = sum; gradients of both networks; Adam; metrics loss/psnr_coarse/psnr_fine.
 * Weights, gradients and Adam moments are flat blobs in Keras get_weights() order (as nerf_load_weights). */
typedef struct nerf_train_config {
    float learning_rate;       /* Adam(optimizer_lr), src/ExecutionRun.py:226 */
    float beta_1, beta_2;      /* Keras defaults 0.9, 0.999 */
    float epsilon;             /* Keras default 1e-7 */
    int32_t sampler_gradient;  /* 1 = reference behaviour; 0 = treat z_from_dist as data (classic NeRF) */
    /* ABI 2: the reference's production policy (mixed_float16, src/ExecutionRun.py:220-221; loss-scaled branch of
     * train_step, src/NeRF.py:159-163; LossScaleOptimizer, src/ExecutionRun.py:262).  0 = the fp32 policy (fp32-class
     * products).  1 = fp16 compute: forward and data gradients with ONE fp16 MFMA pass per product, activations /
     * gradients rounded to fp16 between layers, fp32 accumulation, fp32 master weights and weight gradients; the
     * loss is scaled before the backward pass, gradients are unscaled and tested: a step with a non-finite gradient is
     * SKIPPED and halves the scale, dynamic_growth_steps finite steps in a row double it (Keras 2.7 dynamic loss
     * scaling: initial 2^15, growth interval 2000).  All three network variants (n_angles 2, 1, 0). */
    int32_t mixed_float16;
    float initial_loss_scale;      /* 0 -> 32768 */
    int32_t dynamic_growth_steps;  /* 0 -> 2000 */
} nerf_train_config;

/* Starts a trainer on the weights currently loaded (coarse required, fine optional); zero Adam moments.  Called while a
 * trainer is running it restarts the optimizer on the TRAINED weights (and resets the loss weights to 1, 1 and
 * nerf_train_set_ray_gradients to off).
 * Rendering between optimizer steps is allowed at any time (DietNeRF's consistency render, the epoch plots,
 * src/ExecutionRun.py:193-201): the render path's operand streams are re-packed from the trained weights on the device,
 * enqueued on the ctx stream, without a host round trip. */
int nerf_train_begin(nerf_ctx* ctx, const nerf_train_config* cfg);
/* Packs the trained weights for the render path and frees optimizer state and activation buffers. */
int nerf_train_end(nerf_ctx* ctx);
int nerf_train_set_learning_rate(nerf_ctx* ctx, float learning_rate);
/* ABI 5: the ray loss of nerf_train_step / nerf_train_gradients is coarse_mse_weight * MSE(coarse render) +
 * fine_mse_weight * MSE(fine render).  (1, 1) -- the state nerf_train_begin leaves -- is NeRF.train_step
 * (src/NeRF.py:151,157).  DietNeRF's train_step builds its ray loss differently (src/DietNeRF.py:160-170,
 * `loss = loss_for_rays` BEFORE `loss_for_rays += <fine MSE>`, then `loss += loss_for_rays`): 2 * MSE(coarse) +
 * MSE(fine) is what its tape differentiates -- (2, 1) here.  The weights act on the gradients and on the `loss` metric
 * (and its running sum); psnr_coarse / psnr_fine stay the plain per-pass values.  Finite, >= 0. */
int nerf_train_set_loss_weights(nerf_ctx* ctx, float coarse_mse_weight, float fine_mse_weight);
/* ABI 6+, distortion loss (mip-NeRF 360): a per-ray regulariser on the compositing weights of a pass, which pulls a ray's
 * weight into one compact interval and pushes weight spread along the ray ("floaters") to zero.  For a ray with depths
 * z_0 <= ... <= z_{S-1} and compositing weights w_i (the `weights` output of the pass), with the ctx's bounds
 * (nerf_ctx_set_bounds; 0 and 1 for NDC rays):
 *     t_i = (z_i - near) / (far - near),  t_S = 1;  sample i owns [t_i, t_{i+1}] (the last one, whose compositing interval
 *     is 1e9, owns [t_{S-1}, 1]);  m_i = (t_i + t_{i+1}) / 2,  d_i = t_{i+1} - t_i
 *     L_ray = sum_i sum_j w_i w_j |m_i - m_j|  +  (1/3) sum_i w_i^2 d_i          L = mean of L_ray over the batch's rays
 * and the objective of nerf_train_step / nerf_train_gradients becomes
 *     coarse_mse_weight * MSE(coarse) + fine_mse_weight * MSE(fine) + coarse * L(coarse pass) + fine * L(fine pass).
 * Finite, >= 0; (0, 0) -- the state nerf_train_begin leaves -- runs no kernel of it, and losses, gradients and step time are
 * those of a library without it, bit for bit.  The gradient reaches the network through dL/dw of the compositing and, for
 * the fine pass under sampler_gradient = 1, through dL/dz of the fine depths into the sampler and the coarse network (the
 * coarse depths are data).  Under mixed_float16 it carries the loss scale like every other gradient.  The `loss` metric and
 * its running sum stay the weighted MSE sum; L has running sums of its own, below.  A data-parallel step takes the mean over
 * each rank's shard before the blobs are averaged.  The regulariser belongs to the ray loss ONLY: the backward passes
 * through NeRF.render() that take a caller's d_rgb (nerf_train_render_gradients, nerf_train_render_forward /
 * nerf_train_render_backward) do not apply it.  Needs far > near at the next gradient computation. */
int nerf_train_set_distortion_weights(nerf_ctx* ctx, float coarse, float fine);
/* ABI 6+: every nerf_train_step / nerf_train_gradients with a non-zero distortion weight for a pass adds that pass's
 * UNWEIGHTED L to a running sum on the device; this call synchronises, returns the sums and the number of such gradient
 * computations since the last read, and clears them (either pointer may be NULL).  A pass whose weight is 0 adds nothing. */
int nerf_train_read_distortion_sums(nerf_ctx* ctx, double* sums /* [2]: L coarse, L fine */, int64_t* steps);
/* ABI 6+: the bare operator on caller data, beside nerf_ray_marching and nerf_sample_pdf: weights, z (N,S), z sorted along
 * each ray -> loss_per_ray (N) = L_ray, d_weights (N,S) = dL_ray/dw, d_z (N,S) = dL_ray/dz -- unscaled, per ray, no 1/N; any
 * output pointer may be NULL.  One ray per wavefront, no atomics: the same inputs give the same bits on every run.  Needs
 * S >= 1 and far > near. */
int nerf_distortion_loss(nerf_ctx* ctx, const float* weights, const float* z, int64_t N, int32_t S, float* loss_per_ray,
                         float* d_weights, float* d_z, int mem);
/* mixed_float16 policy: the current loss scale, the optimizer steps applied and the steps skipped so far (1 / n / 0
 * under the fp32 policy).  Any pointer may be NULL. */
int nerf_train_loss_scale(nerf_ctx* ctx, float* loss_scale, int64_t* steps_applied, int64_t* steps_skipped);
/* One NeRF.train_step on N rays: rays_orig/rays_dirs (N,4), target_rgb (N,3); u_coarse (N,Sc) / u_fine (N,Sf)
 * NULL -> on-device Philox(seed, ray index in the batch).  metrics (host, nullable): loss, psnr_coarse, psnr_fine;
 * passing it synchronises.  Sf = 0 (or no fine network) trains the coarse network alone (src/NeRF.py:153).
 * With a communicator (nerf_comm_init, world > 1) the step is data-parallel: every rank passes its own shard of the
 * batch and the two gradient blobs are averaged with one ncclAllReduce each before the (identical) Adam update;
 * metrics are this rank's.  Under mixed_float16 the finiteness test is repeated on the reduced blobs, so a non-finite
 * shard on ANY rank makes EVERY rank skip the step and halve its loss scale. */
int nerf_train_step(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, const float* target_rgb,
                    int64_t N, int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                    float* metrics, int mem);
/* ABI 4: Keras' History keeps the per-epoch MEANS of train_step's metrics (model.fit, src/ExecutionRun.py:186-201).  Every
 * nerf_train_step / nerf_train_gradients adds its loss, psnr_coarse and psnr_fine (the very values `metrics` would receive)
 * to running sums on the device; this call synchronises, returns the sums and the number of steps since the last read,
 * and clears them -- a training loop passes metrics = NULL per step (no synchronisation) and reads once per epoch. */
int nerf_train_read_metric_sums(nerf_ctx* ctx, double* sums /* [3]: loss, psnr_coarse, psnr_fine */, int64_t* steps);
/* The two halves of a step, for data-parallel training: gradients (kept in the ctx and optionally copied out
 * as blobs), then -- after the caller averaged them over ranks -- the Adam update (NULL = use the ctx's own).
 * mixed_float16 (ABI 3): nerf_train_gradients returns UNSCALED gradients and takes no verdict; nerf_train_apply tests
 * the blobs it is about to apply (the caller's all-reduced ones, or the ctx's own), skips a non-finite step and moves
 * the loss scale -- all on the device -- so every rank of a data-parallel job reaches the same verdict from the same
 * reduced blobs (a non-finite shard makes the sum non-finite everywhere). */
int nerf_train_gradients(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, const float* target_rgb,
                         int64_t N, int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine,
                         uint64_t seed, float* grad_coarse, float* grad_fine, float* metrics, int mem);
int nerf_train_apply(nerf_ctx* ctx, const float* grad_coarse, const float* grad_fine, int mem);
/* Backward through NeRF.render() itself (src/NeRF.py:109-134): the graph DietNeRF's consistency loss differentiates
 * when it renders an image under the tape (src/DietNeRF.py:204-222, render_image -> render per ray batch).  Unlike
 * train_step, the fine pass runs on sort(concat(z_fine, z_coarse)) (Sc + Sf samples) and only its rgb is an output.
 * d_rgb (N,3) = dL/d(render()[0]) supplied by the caller (e.g. from its embedding network); the call re-runs the
 * forward with activation stash on these N rays -- same draws as nerf_render with the same (seed, ray_base) -- and
 * leaves dL/d(weights) in the ctx's gradient blobs: overwriting them (accumulate = 0) or adding to what
 * nerf_train_gradients left there (accumulate = 1: the reference sums both losses before one Adam step), ready for
 * nerf_train_apply(ctx, NULL, NULL, mem).  The coarse network receives gradient only through the inverse-CDF sampler
 * (none with sampler_gradient = 0).  rgb_out / grad_coarse / grad_fine: optional copies.
 * mixed_float16 (ABI 4; the policy the reference always runs under, src/ExecutionRun.py:220-221): DietNeRF scales the
 * SUM of ray loss and consistency loss and unscales once (src/DietNeRF.py:142-153,192-202).  Here the caller's d_rgb is
 * multiplied by the current loss scale ON THE DEVICE, the single-pass fp16 chain runs on it (fp16 gradient buffers that
 * carry the scale, as in nerf_train_gradients), and the call leaves UNSCALED gradients: stored (accumulate = 0) or added to
 * the unscaled gradients nerf_train_gradients left (accumulate = 1) -- like with like.  The finiteness flag is reset by
 * accumulate = 0 (a new gradient computation; gradients that were computed and never applied do not decide this one's
 * verdict) and COLLECTS over nerf_train_gradients + accumulate = 1 calls; nerf_train_apply takes the one verdict on the
 * summed blobs: a non-finite d_rgb (or an overflow in the chain) skips the step and halves the scale. */
int nerf_train_render_gradients(nerf_ctx* ctx, const float* rays_orig, const float* rays_dirs, const float* d_rgb,
                                int64_t N, int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine,
                                uint64_t seed, int64_t ray_base, int32_t accumulate, float* rgb_out,
                                float* grad_coarse, float* grad_fine, int mem);
/* ABI 5: the same graph in two calls, the activations kept in between -- for callers whose d_rgb depends on the WHOLE image
 * (DietNeRF: the embedding network sees all 150 x 150 pixels before any gradient exists, src/DietNeRF.py:215-221).  The reference
 * renders the image once, under the tape; with nerf_render_image + nerf_train_render_gradients the forward runs twice.  Here:
 *   nerf_train_render_forward(slot = b, batch b of the rays, ...) for every batch -- rgb_out is that batch's part of the image,
 *     the forward of the tape itself (under mixed_float16: the single-pass fp16 network), its activations stay in slot b
 *     (about 1.7 MB per ray at 55 + 110 rows under the float32 policy, half under mixed_float16: a 150 x 150 image is 38 / 19
 *     GB of the device's 288 GB; slots are grow-only buffers, nerf_train_render_release or nerf_train_end frees them);
 *   ... the caller turns the image into d_rgb ...
 *   nerf_train_render_backward(slot = b, d_rgb of batch b, accumulate, ...) for every batch: exactly the backward half of
 *     nerf_train_render_gradients -- bit-identical gradients, same loss-scale handling -- on the kept activations.
 * A slot holds one forward pass: a backward pass consumes it, an optimizer step (nerf_train_apply / nerf_train_step) invalidates
 * every slot (the activations belong to the weights that made them), a new forward into the slot overwrites it.  The slot keeps
 * its own copies of rays and draws.  slot: 0..4095. */
int nerf_train_render_forward(nerf_ctx* ctx, int32_t slot, const float* rays_orig, const float* rays_dirs, int64_t N,
                              int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                              int64_t ray_base, float* rgb_out, int mem);
int nerf_train_render_backward(nerf_ctx* ctx, int32_t slot, const float* d_rgb, int32_t accumulate, float* grad_coarse,
                               float* grad_fine, int mem);
int nerf_train_render_release(nerf_ctx* ctx);
/* ABI 6+, differentiable render outputs: the same two calls with every output of NeRF.render() a training loss can be written
 * on -- depth supervision, a depth-smoothness or ray-entropy regulariser, any loss on more than the colour -- and a cotangent
 * for each.  The outputs are those of the LAST pass (the fine pass on the Sc + Sf merged, sorted depths; the coarse pass
 * when there is no fine one): S = Sc + Sf with a fine pass, else Sc. */
typedef struct nerf_train_outputs {   /* any pointer may be NULL */
    float* rgb;      /* (N,3) render()[0], the forward of the tape                  */
    float* depth;    /* (N)   sum_s w_s z_s of the last pass                        */
    float* weights;  /* (N,S) compositing weights of the last pass                  */
    float* z;        /* (N,S) its depths (merged and sorted with a fine pass)       */
} nerf_train_outputs;
typedef struct nerf_render_grads {    /* cotangents dL/d(output); any may be NULL = zero, not all four */
    const float* d_rgb;      /* (N,3) */
    const float* d_depth;    /* (N)   */
    const float* d_weights;  /* (N,S) */
    const float* d_z;        /* (N,S) */
} nerf_render_grads;
/* nerf_train_render_forward_outputs is nerf_train_render_forward with more outputs: same slot, same draws, same kernels; rgb
 * is bit-equal to nerf_train_render_forward's; weights and z are copies of what the slot keeps of its last pass; depth is the
 * compositing kernel's own sum (a buffer for it exists only once depth has been asked for).  Slots are interchangeable:
 * either forward call fills a slot that either backward call consumes.
 * nerf_train_render_backward_outputs is nerf_train_render_backward with the upstream gradient g.  With only g->d_rgb set it
 * launches exactly what nerf_train_render_backward launches and leaves bit-identical gradients.  Every rule of that call
 * holds: accumulate; mixed_float16 (the caller passes UNSCALED cotangents, all four are multiplied by the loss scale on the
 * device, and the unscaled result is tested and stored or added like with like); the slot is consumed; a slot filled under
 * nerf_ctx_set_train_sample_culling runs backward on its own record (compositing and its backward run on all samples, so the
 * new cotangents follow the flag exactly as d_rgb does).  One kernel, one thread per sample, no atomics, folds the three new
 * cotangents into the last pass -- in float32, multiply and add rounded separately, absent inputs counting as 0:
 *     g_w[r,s] = d_weights[r,s] + d_depth[r] * z[r,s]         g_z[r,s] = d_z[r,s] + d_depth[r] * w[r,s]
 * (times the loss scale; 1 under the float32 policy).  g_w enters the last pass's compositing backward as its external
 * dL/d(weights) -- the input the sampler's gradient uses on the coarse pass; g_z is ADDED to that pass's dL/dz after the
 * compositing backward has stored there, and travels on through the merge and the inverse-CDF sampler into the coarse network.
 * Where it has an effect: d_z and the d_depth * w term act only with a fine pass under sampler_gradient = 1, and only through
 * the Sf new depths; the coarse depths are data, their entries are dropped.  Without a fine pass or without the sampler term
 * they are ignored, and the gradients are bit-equal with and without d_z.  Nothing of this launches and no buffer grows unless
 * one of the three new cotangents or outputs is non-NULL.  sum_s w_s is 1 on every ray under this compositing (the last
 * sample's interval is 1e9), so there is no accumulated-opacity output: it would carry no gradient.
 * Errors: outs / g NULL, all four cotangents NULL, an empty or consumed slot. */
int nerf_train_render_forward_outputs(nerf_ctx* ctx, int32_t slot, const float* rays_orig, const float* rays_dirs, int64_t N,
                                      int32_t Sc, int32_t Sf, const float* u_coarse, const float* u_fine, uint64_t seed,
                                      int64_t ray_base, const nerf_train_outputs* outs, int mem);
int nerf_train_render_backward_outputs(nerf_ctx* ctx, int32_t slot, const nerf_render_grads* g, int32_t accumulate,
                                       float* grad_coarse, float* grad_fine, int mem);
/* ABI 6+: the bare operator on caller data, beside nerf_distortion_loss: the fold above for weights, z (N,S) and any subset of
 * d_depth (N), d_weights, d_z (N,S) (NULL = 0) -> g_w, g_z (N,S), either may be NULL; unscaled.  Needs S >= 1. */
int nerf_render_output_grads(nerf_ctx* ctx, const float* weights, const float* z, int64_t N, int32_t S, const float* d_depth,
                             const float* d_weights, const float* d_z, float* g_w, float* g_z, int mem);
/* ABI 6+, ray gradients: dL/d(rays_orig) and dL/d(rays_dirs) of the same scalar the render backward differentiates, with
 * respect to the ray arrays handed to the slot's forward call -- what pose refinement, registering a new photograph to a
 * trained scene, or any loss that moves cameras needs.  Both are (N,4) float32 with component 3 exactly 0.
 * Included is everything NeRF.render()'s graph routes through the rays:
 *   - the sample points p = o + d z of every network pass that takes part in the call: the last pass and, with a fine network
 *     under sampler_gradient = 1, the coarse pass, which is reached through the sampler
 *     (d_o = sum_s dL/dp_s, d_d = sum_s z_s dL/dp_s);
 *   - the view-direction input of those passes: the raw, un-normalised direction, components [0,1,2] for n_angles = 2 and
 *     [0,2] for n_angles = 1 (none for the xyz-only network).
 * Treated as data: the coarse depths (as everywhere in the trainer: the coarse depths are data), the near / far bounds, and
 * the per-ray bounds that a scene box or an occupancy grid derives from the ray.  Under NDC rays the gradients are with
 * respect to the NDC rays the call received.  Samples culled under nerf_ctx_set_train_sample_culling contribute nothing; a
 * ray whose samples are all culled gets zeros.  Without a fine pass or without the sampler term the coarse pass contributes
 * exactly what it contributes to the weights: nothing if a fine network exists and sampler_gradient = 0.  Under mixed_float16
 * the chain carries the loss scale as it does for the weights and the ray gradients are unscaled on the device from the
 * trainer's loss-scale state, without a host round trip; a non-finite ray gradient does not change the step verdict by
 * itself (the weight gradients of the same call decide it).
 * nerf_train_set_ray_gradients switches the feature on a running trainer: the encoding gradient is a by-product of how a
 * network's backward operand stream is packed, so the call re-packs both networks' backward streams with (on) or without
 * (off) the encoding tiles.  Off is the default and the state nerf_train_begin leaves -- a restarted trainer has it off
 * again.  While it is off nothing changes: the same kernels run, the same buffers exist and every entry point leaves the
 * same bits.  While it is on, the coarse network's backward chain runs its encoding-gradient variant (same arithmetic class;
 * its weight gradients need not be bit-equal to the off state's), the fine network's is the variant it already runs under
 * sampler_gradient = 1.  Kept slots stay valid across the switch.  The exact-fp32 reference trainer (NERF_TRAIN_FORWARD=gemm)
 * does not implement it: switching on fails there with an error that names the fused trainer.
 * nerf_train_render_backward_rays is nerf_train_render_backward_outputs plus the two ray outputs (either may be NULL); with
 * both NULL it is that call, bit for bit.  The ray gradients are stored, never accumulated (`accumulate` acts on the blobs).
 * Two kernels per pass, one ray per wavefront, fixed summation order, no atomics: the same inputs give the same bits on every
 * run.  Fails if the switch is off.  Not covered: nerf_train_step / nerf_train_gradients (the two-MSE ray loss is another
 * graph), the data-parallel path, gradients through box / grid / NDC bounds. */
int nerf_train_set_ray_gradients(nerf_ctx* ctx, int32_t on);
int nerf_train_render_backward_rays(nerf_ctx* ctx, int32_t slot, const nerf_render_grads* g, int32_t accumulate,
                                    float* grad_coarse, float* grad_fine, float* d_rays_orig, float* d_rays_dirs, int mem);
/* ABI 6+: the bare reduction on caller data, beside nerf_distortion_loss and nerf_render_output_grads: d_points (N,S,3) =
 * dL/dp per sample, z (N,S) -> d_rays_orig[r] = sum_s d_points[r,s], d_rays_dirs[r] = sum_s z[r,s] d_points[r,s], (N,4) with
 * component 3 = 0; either output may be NULL.  float32, the order of the kernel above.  Needs S >= 1. */
int nerf_ray_position_grads(nerf_ctx* ctx, const float* d_points, const float* z, int64_t N, int32_t S, float* d_rays_orig,
                            float* d_rays_dirs, int mem);
/* ABI 3: the gradient blob of a network as the ctx holds it now -- after nerf_train_gradients /
 * nerf_train_render_gradients the gradients just computed, after a data-parallel nerf_train_step the all-reduced mean
 * the Adam update used (what the reference's tape.gradient returns, src/NeRF.py:159-165). */
int nerf_train_get_gradients(nerf_ctx* ctx, int which, float* blob, size_t n_floats, int mem);
/* Current weights of a network as a blob (model.get_weights(), src/UtilsFiles.py:153-164 saves these). */
int nerf_get_weights(nerf_ctx* ctx, int which, float* blob, size_t n_floats, int mem);

/* ---- measurement ------------------------------------------------------------------------- */
/* When enabled, every fused PE+MLP kernel launch is bracketed by HIP events on the ctx stream.
 * nerf_ctx_read_timing synchronises, returns the summed kernel time / launch count / MLP rows
 * since the last read, and resets the counters. */
int nerf_ctx_enable_timing(nerf_ctx* ctx, int on);
int nerf_ctx_read_timing(nerf_ctx* ctx, double* mlp_ms, int64_t* n_launches, int64_t* n_rows);
/* With timing on, the culled passes' own stages by stream events, summed since the last call (synchronises, then clears):
 * ms4[0] verdict + scan, [1] the host's read of the row count (copy, synchronise, growing the compact buffers), [2] gather,
 * [3] expand; the network itself is nerf_ctx_read_timing's.  *n_passes (nullable) = the culled passes counted.
 * nerf_ctx_read_timing and nerf_ctx_enable_timing clear these events as well, so a caller who never asks for them keeps
 * nothing: to have both, call this one first. */
int nerf_ctx_read_culling_timing(nerf_ctx* ctx, double* ms4, int64_t* n_passes);

#ifdef __cplusplus
}
#endif
#endif /* NERF_MI355_H */
