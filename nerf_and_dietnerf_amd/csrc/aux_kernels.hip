// aux_kernels.hip -- the non-MLP functions of the render path as HIP kernels (gfx950):
//   raygen        get_rays_directions            src/UtilsCV.py:467-499 (+ origins, src/NeRF.py:209)
//   z_values      get_z_values                   src/UtilsCV.py:565-581
//   sample_pdf    get_z_vals_from_prob_dist_func src/UtilsCV.py:502-539 (+ sort(concat), src/NeRF.py:132)
//   composite     ray_marching                   src/UtilsNeuralRadianceField.py:88-115 (+ depth, ExecutionRun.py:346)
//   posenc        positional_encoding_for_*      src/UtilsNeuralRadianceField.py:52-85 (standalone; tests/tools)
// and two the reference does not have ("Ray and sampling space"):
//   rays_to_ndc   world rays -> NDC rays of a forward-facing scene
//   z_values, disparity-linear mode
//   scene box     ray_box_interval: the part of [near, far] a ray spends inside an axis-aligned box; the depth kernel's box
//                 source draws on it, ray_box_bounds returns it
//   repack        weight blob -> an operand stream of the MLP kernels, through a gather table (weight_tables.hip)
//
// All HBM-bound fp32/int32 work.  Evaluation order is the canonical one of oracle/nerf_oracle.py:
// sums / cumsum / cumprod run left to right along the sample axis and products are NOT contracted
// into FMAs (explicit __fmul_rn/__fadd_rn), so index selection in the sampler is bit-exact against
// the oracle and the other outputs differ only through expf.
#include "field_device.h"
#include "nerf_kernels.h"
#include "ray_box_device.h"
#include "sampling_device.h"

#include <algorithm>

namespace nerf {

// ------------------------------------------------------------------------------------------------
// raygen: one thread per ray of the slab [ray_begin, ray_begin + ray_count) of the H*W image.
// ------------------------------------------------------------------------------------------------
struct RaygenArgs {
    float c[16];
    float tan_half;
    int H, W;
    long long ray_begin, ray_count;
    float* orig;
    float* dirs;
};

__global__ void raygen_kernel(const RaygenArgs a) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= a.ray_count) return;
    const long long ray = a.ray_begin + t;
    const int i = (int)(ray / a.W), j = (int)(ray % a.W);
    // pixel centre -> NDC -> screen space (same tan for both axes, no aspect term)
    const float x_ndc = __fdiv_rn((float)j + 0.5f, (float)a.W);
    const float y_ndc = __fdiv_rn((float)i + 0.5f, (float)a.H);
    const float xs = __fsub_rn(__fmul_rn(2.0f, x_ndc), 1.0f);
    const float ys = __fsub_rn(1.0f, __fmul_rn(2.0f, y_ndc));
    const float xc = __fmul_rn(xs, a.tan_half);
    const float yc = __fmul_rn(ys, a.tan_half);
    float d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        // einsum('ij,...j') with v = (xc, yc, -1, 0): ((c0*x + c1*y) + c2*z) + c3*0
        float s = __fadd_rn(__fmul_rn(a.c[r * 4 + 0], xc), __fmul_rn(a.c[r * 4 + 1], yc));
        s = __fadd_rn(s, __fmul_rn(a.c[r * 4 + 2], -1.0f));
        s = __fadd_rn(s, __fmul_rn(a.c[r * 4 + 3], 0.0f));
        d[r] = s;
    }
    reinterpret_cast<float4*>(a.dirs)[t] = make_float4(d[0], d[1], d[2], d[3]);
    if (a.orig) reinterpret_cast<float4*>(a.orig)[t] = make_float4(a.c[3], a.c[7], a.c[11], a.c[15]);
}

// tf.tan(field_of_view / 2) (UtilsCV.py:488): tan of fp32(fov/2), evaluated in double and rounded once
static float raygen_tan_half(float fov) { return (float)tan((double)(fov * 0.5f)); }

void launch_raygen(const float c2w_host[16], float fov, int H, int W, long long ray_begin,
                   long long ray_count, float* orig, float* dirs, hipStream_t stream) {
    if (ray_count <= 0) return;
    RaygenArgs a;
    for (int i = 0; i < 16; ++i) a.c[i] = c2w_host[i];
    a.tan_half = raygen_tan_half(fov);
    a.H = H; a.W = W; a.ray_begin = ray_begin; a.ray_count = ray_count; a.orig = orig; a.dirs = dirs;
    hipLaunchKernelGGL(raygen_kernel, dim3(blocks_for(ray_count)), dim3(kBs), 0, stream, a);
}

// ------------------------------------------------------------------------------------------------
// rays_to_ndc: one thread per ray.  Cameras look down -z; n = distance of the near plane z = -n; k = 1 / tan_half is the
// NDC scale of BOTH axes (the raygen above has one tangent and no aspect term).
//   tn = -(n + o_z) / d_z;  p = o + tn d              (the origin moved onto the near plane: p_z = -n)
//   o' = (-k p_x / p_z, -k p_y / p_z, 1 + 2n / p_z)   (o'_z = -1)
//   d' = (-k (d_x / d_z - p_x / p_z), -k (d_y / d_z - p_y / p_z), -2n / p_z)   (o' + d' is the point at infinity: z = +1)
// w is copied.  d_z = 0 (a ray parallel to the near plane) gives non-finite rays: not guarded.  In place (out == in) is
// fine: a thread reads its own ray before it writes it.
// ------------------------------------------------------------------------------------------------
__global__ void rays_to_ndc_kernel(const float* orig, const float* dirs, long long N, float n, float two_n, float k,
                                   float* out_orig, float* out_dirs) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const float4 o = reinterpret_cast<const float4*>(orig)[t];
    const float4 d = reinterpret_cast<const float4*>(dirs)[t];
    const float tn = -__fdiv_rn(__fadd_rn(n, o.z), d.z);
    const float px = __fadd_rn(o.x, __fmul_rn(tn, d.x));
    const float py = __fadd_rn(o.y, __fmul_rn(tn, d.y));
    const float pz = __fadd_rn(o.z, __fmul_rn(tn, d.z));
    const float rx = __fdiv_rn(px, pz), ry = __fdiv_rn(py, pz), e = __fdiv_rn(two_n, pz);
    const float sx = __fdiv_rn(d.x, d.z), sy = __fdiv_rn(d.y, d.z);
    reinterpret_cast<float4*>(out_orig)[t] = make_float4(-__fmul_rn(k, rx), -__fmul_rn(k, ry), __fadd_rn(1.0f, e), o.w);
    reinterpret_cast<float4*>(out_dirs)[t] =
        make_float4(-__fmul_rn(k, __fsub_rn(sx, rx)), -__fmul_rn(k, __fsub_rn(sy, ry)), -e, d.w);
}

void launch_rays_to_ndc(const float* orig, const float* dirs, long long N, float fov, float near_plane, float* out_orig,
                        float* out_dirs, hipStream_t stream) {
    if (N <= 0) return;
    const float k = (float)(1.0 / (double)raygen_tan_half(fov));   // the raygen's own (rounded) tangent, inverted once
    hipLaunchKernelGGL(rays_to_ndc_kernel, dim3(blocks_for(N)), dim3(kBs), 0, stream, orig, dirs, N,
                       near_plane, 2.0f * near_plane, k, out_orig, out_dirs);
}

// ------------------------------------------------------------------------------------------------
// Scene box: ray_box_hit / ray_box_interval, the rule and its statement, are in ray_box_device.h
// (the volume march of volume_kernels.hip clips its rays with the same function).
// A narrowed ray draws its depths on [a, b] with constants of its own; any other ray -- a miss, or a box that contains
// its whole [near, far] -- keeps the host's constants and so the depths of a context without a box, bit for bit.
// This one function decides for the depth kernel and for nerf_ray_box_bounds.
// ------------------------------------------------------------------------------------------------
// nerf_ray_box_bounds: one thread per ray.  bounds (N,2) = (a, b) of a narrowed ray, (near, far) of any other.
__global__ void ray_box_bounds_kernel(const BoxArgs bx, const float* __restrict__ orig, const float* __restrict__ dirs,
                                      long long N, float* __restrict__ bounds, int* __restrict__ narrowed) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float a, b;
    const bool nar = ray_box_interval(bx, reinterpret_cast<const float4*>(orig)[r], reinterpret_cast<const float4*>(dirs)[r], &a, &b);
    reinterpret_cast<float2*>(bounds)[r] = nar ? make_float2(a, b) : make_float2(bx.near_b, bx.far_b);
    if (narrowed) narrowed[r] = nar ? 1 : 0;
}

void launch_ray_box_bounds(const SceneBox& box, float near_b, float far_b, const float* orig, const float* dirs, long long N,
                           float* bounds, int* narrowed, hipStream_t stream) {
    if (N <= 0) return;
    hipLaunchKernelGGL(ray_box_bounds_kernel, dim3(blocks_for(N)), dim3(kBs), 0, stream,
                       box_args(box, near_b, far_b), orig, dirs, N, bounds, narrowed);
}

// ------------------------------------------------------------------------------------------------
// Occupancy grid (include/nerf_mi355.h: nerf_ctx_set_occupancy_grid has the rule): R x R x R bits
// over the scene box, cell (ix, iy, iz) = bit ix + R (iy + R iz) of a little-endian uint32 array.  ray_grid_interval walks a
// ray through the cells of its box interval [a0, b0] (Amanatides-Woo) and returns the stretch from the first occupied cell
// it enters to the last one it leaves.  float32, every operation rounded on its own; a plane's parameter is recomputed from
// its index at every step, never accumulated.  -> 0: the ray keeps (near, far); 1: the box alone narrows it to (a0, b0);
// 2: the grid narrows it to (a, b).  A ray that meets no occupied cell (or meets occupied cells only in a point: b > a is
// asked for, as the box rule asks it of a hit), or whose occupied stretch is all of [a0, b0], is left to the box rule: nothing
// is ever left unsampled, and a full grid is the box alone, bit for bit.
// The cell index is held in [0, R) wherever the bits are read.
// The verdict on a single sample under the same grid (step 2's cell of the sample's own point) is sample_kept, in
// cull_kernels.hip beside the kernels that call it: device functions do not cross translation units in this build, so the
// cell index the two share is nerf_device.h's grid_cell_index.
// ------------------------------------------------------------------------------------------------
struct GridArgs {
    BoxArgs bx;
    const uint32_t* bits;
    int R;
};

__device__ __forceinline__ float grid_plane(float lo, float cell, int k, float o, float d) {
    return __fdiv_rn(__fsub_rn(__fadd_rn(lo, __fmul_rn(cell, (float)k)), o), d);
}

__device__ __forceinline__ int ray_grid_interval(const GridArgs& g, const float4 o, const float4 d, float* a, float* b) {
    const BoxArgs& bx = g.bx;
    const int R = g.R;
    // steps 1-3 of the box rule, from the function the box kernels decide with: a hit that the box does not narrow still
    // walks the grid
    float a0, b0;
    const bool hit = ray_box_hit(bx, o, d, &a0, &b0);
    const bool box_narrowed = hit && (a0 > bx.near_b || b0 < bx.far_b);
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    *a = bx.near_b; *b = bx.far_b;
    if (!hit) return 0;
    float cell[3], tp[3];
    int idx[3], step[3], plane[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        cell[ax] = __fdiv_rn(__fsub_rn(bx.hi[ax], bx.lo[ax]), (float)R);
        const float p = __fadd_rn(oo[ax], __fmul_rn(a0, dd[ax]));
        idx[ax] = grid_cell_index(p, bx.lo[ax], cell[ax], R);                   // NaN -> 0
        step[ax] = dd[ax] > 0.0f ? 1 : -1;
        plane[ax] = idx[ax] + (dd[ax] > 0.0f ? 1 : 0);
        tp[ax] = dd[ax] == 0.0f ? __builtin_huge_valf() : grid_plane(bx.lo[ax], cell[ax], plane[ax], oo[ax], dd[ax]);
    }
    float t = a0, ga = 0.f, gb = 0.f;
    bool found = false;
    const int max_steps = 3 * R + 3;
    for (int it = 0; it < max_steps; ++it) {
        int ax = 0;
        float tm = tp[0];
        if (tp[1] < tm) { ax = 1; tm = tp[1]; }
        if (tp[2] < tm) { ax = 2; tm = tp[2]; }
        float te = tm;
        if (te > b0) te = b0;
        if (te < t) te = t;
        const int bit = idx[0] + R * (idx[1] + R * idx[2]);       // < R^3 <= 2^24
        if ((g.bits[bit >> 5] >> (bit & 31)) & 1u) {
            if (!found) { ga = t; found = true; }
            gb = te;
        }
        if (!(tm < b0)) break;
        // the stepped axis, written without a dynamic index into the per-axis arrays (they stay in registers)
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k == ax) {
                idx[k] += step[k];
                plane[k] += step[k];
                tp[k] = grid_plane(bx.lo[k], cell[k], plane[k], oo[k], dd[k]);
            }
        if (idx[0] < 0 || idx[0] >= R || idx[1] < 0 || idx[1] >= R || idx[2] < 0 || idx[2] >= R) break;
        t = te;
    }
    if (found && gb > ga && (ga > a0 || gb < b0)) { *a = ga; *b = gb; return 2; }
    if (box_narrowed) { *a = a0; *b = b0; return 1; }
    return 0;
}

// One thread per ray: bounds (N,2), state (N).  The walk takes up to 3R + 3 steps, so unlike the box decision it is made
// once per ray, here, and z_values_kernel (kDepthBounds) reads the result.
__global__ void ray_grid_bounds_kernel(const GridArgs g, const float* __restrict__ orig, const float* __restrict__ dirs,
                                       long long N, float* __restrict__ bounds, int* __restrict__ state) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    float a, b;
    const int st = ray_grid_interval(g, reinterpret_cast<const float4*>(orig)[r], reinterpret_cast<const float4*>(dirs)[r], &a, &b);
    reinterpret_cast<float2*>(bounds)[r] = make_float2(a, b);
    if (state) state[r] = st;
}

void launch_ray_grid_bounds(const SceneBox& box, float near_b, float far_b, const uint32_t* bits, int R, const float* orig,
                            const float* dirs, long long N, float* bounds, int* state, hipStream_t stream) {
    if (N <= 0) return;
    GridArgs g;
    g.bx = box_args(box, near_b, far_b);
    g.bits = bits; g.R = R;
    hipLaunchKernelGGL(ray_grid_bounds_kernel, dim3(blocks_for(N)), dim3(kBs), 0, stream, g, orig, dirs, N,
                       bounds, state);
}

// ------------------------------------------------------------------------------------------------
// z_values: one thread per sample, z[r, s] = stratified_depth (sampling_device.h) on the ray's depth range.  The range is the
// context's [near, far] with the host's constants, unless the ray has one of its own (depth_consts_of_interval on its (a, b)):
//   kDepthHost    no ray has
//   kDepthBox     a ray the scene box narrows (ray_box_interval).  Every thread of a ray reads the ray's 32 bytes and takes
//                 the decision again: S threads, one cache line, no bounds buffer and no launch in front of this one
//   kDepthBounds  a ray of state 1 or 2 in the bounds / state that ray_grid_bounds_kernel left (its walk is made once per ray)
// One kernel, so a ray that keeps [near, far] has the depths of a context without a box under either source, and a state-1
// ray those the box source gives it, bit for bit.
// ------------------------------------------------------------------------------------------------
enum DepthSrc { kDepthHost, kDepthBox, kDepthBounds };
struct DepthRays {
    BoxArgs bx; const float* orig; const float* dirs;     // kDepthBox
    const float* bounds; const int* state;                // kDepthBounds
};

template <bool LINDISP, int SRC>
__global__ void z_values_kernel(const DepthRays rays, DepthConsts k, long long N, int S, const float* __restrict__ u,
                                uint64_t seed, long long ray_base, float* __restrict__ z) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= N * S) return;
    const long long r = m / S;
    const int s = (int)(m - r * S);
    if constexpr (SRC == kDepthBox) {
        float a, b;
        if (ray_box_interval(rays.bx, reinterpret_cast<const float4*>(rays.orig)[r],
                             reinterpret_cast<const float4*>(rays.dirs)[r], &a, &b))
            k = depth_consts_of_interval<LINDISP>(a, b, S);
    } else if constexpr (SRC == kDepthBounds) {
        if (rays.state[r] != 0) {
            const float2 ab = reinterpret_cast<const float2*>(rays.bounds)[r];
            k = depth_consts_of_interval<LINDISP>(ab.x, ab.y, S);
        }
    }
    const float uu = u ? u[m] : philox_uniform(seed, (uint64_t)(ray_base + r), s, 0u);
    z[m] = stratified_depth<LINDISP>(k, s, S, uu);
}

// the constants of [near, far]: inverses and differences in double, rounded once
static DepthConsts depth_consts_host(float near_b, float far_b, bool lindisp, int S) {
    if (lindisp)   // near_b > 0: the callers refuse anything else
        return {near_b, nextafterf(far_b, near_b), (float)(1.0 / (double)near_b),
                (float)(1.0 / (double)far_b - 1.0 / (double)near_b)};
    return {near_b, far_b, S > 1 ? (far_b - near_b) / (float)(S - 1) : 0.f, (float)((double)far_b - (double)near_b)};
}

void launch_z_values(float near_b, float far_b, bool lindisp, long long N, int S, const float* u, uint64_t seed,
                     long long ray_base, float* z, hipStream_t stream, const float* orig, const float* dirs,
                     const SceneBox* box, const float* bounds, const int* state) {
    if (N <= 0) return;
    using Kernel = void (*)(const DepthRays, DepthConsts, long long, int, const float*, uint64_t, long long, float*);
    static const Kernel kernels[3][2] = {{z_values_kernel<false, kDepthHost>, z_values_kernel<true, kDepthHost>},
                                         {z_values_kernel<false, kDepthBox>, z_values_kernel<true, kDepthBox>},
                                         {z_values_kernel<false, kDepthBounds>, z_values_kernel<true, kDepthBounds>}};
    const DepthSrc src = bounds && state ? kDepthBounds : box && orig && dirs ? kDepthBox : kDepthHost;
    DepthRays rays = {};
    if (src == kDepthBox) { rays.bx = box_args(*box, near_b, far_b); rays.orig = orig; rays.dirs = dirs; }
    if (src == kDepthBounds) { rays.bounds = bounds; rays.state = state; }
    hipLaunchKernelGGL(kernels[src][lindisp ? 1 : 0], dim3(blocks_for(N * S)), dim3(kBs), 0, stream, rays,
                       depth_consts_host(near_b, far_b, lindisp, S), N, S, u, seed, ray_base, z);
}

// ------------------------------------------------------------------------------------------------
// sample_pdf: one ray per wavefront.  LDS per wave: cdf[S], zc[S], znew[Sf], zall[S+Sf].  The arithmetic is
// sampling_device.h's; the backward (train_kernels.hip: sample_pdf_bwd_kernel) recomputes it through the same functions:
//   1. ray_cdf: w, z -> cdf in the canonical order
//   2. each lane: fine draws k = lane, lane+64, ...: inverse_cdf_draw
//   3. stable_rank sort of the Sf new depths, then a binary-search merge with the (already increasing) coarse
//      depths for the fine pass
// ------------------------------------------------------------------------------------------------
constexpr int kPdfWaves = 4;   // rays per workgroup

__global__ __launch_bounds__(64 * kPdfWaves) void sample_pdf_kernel(
    const float* __restrict__ weights, const float* __restrict__ zin, long long N, int S, int Sf,
    const float* __restrict__ u, uint64_t seed, long long ray_base, float* __restrict__ z_new,
    float* __restrict__ z_merged) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const long long ray = (long long)blockIdx.x * kPdfWaves + wave;
    if (ray >= N) return;   // whole wave exits; no block-level barrier is used below
    // per-wave LDS arrays, each padded to a multiple of 4 floats so the rank sorts can read float4
    const int S4 = (S + 3) & ~3, Sf4 = (Sf + 3) & ~3, T = S + Sf, T4 = (T + 3) & ~3;
    const int per_wave = S4 + S4 + Sf4 + T4;
    float* cdf = lds + wave * per_wave;   // first holds w, then pdf, then cdf
    float* zc = cdf + S4;
    float* zn = zc + S4;
    float* za = zn + Sf4;
    const float* wr = weights + ray * S;
    const float* zr = zin + ray * S;
    ray_cdf(wr, zr, S, lane, cdf, zc, nullptr);
    const float kInf = __builtin_huge_valf();
    for (int k = lane; k < Sf4; k += 64) {
        if (k >= Sf) { zn[k] = kInf; continue; }   // padding never ranks below a real sample
        const float uu = u ? u[ray * Sf + k] : philox_uniform(seed, (uint64_t)(ray_base + ray), k, 1u);
        zn[k] = inverse_cdf_draw(cdf, zc, S, uu).z;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // rank sort of the draws
    for (int k = lane; k < Sf; k += 64) {
        const float v = zn[k];
        const int rank = stable_rank(zn, Sf4, v, k);
        if (z_new) z_new[ray * Sf + rank] = v;
        za[rank] = v;                                   // za[0..Sf) = the new depths, sorted
    }
    if (z_merged) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // The stratified coarse depths are increasing by construction (UtilsCV.py:578-580); a caller of
        // the stand-alone entry point may pass anything, so check before relying on it.
        bool bad = false;
        for (int s = lane; s + 1 < S; s += 64) bad |= zc[s + 1] < zc[s];
        if (!__any(bad)) {
            // sort(concat(new, coarse)) = merge of two sorted runs: output slot = own index + number of
            // elements of the OTHER run that precede it, by binary search instead of an O(n^2) sweep
            for (int k = lane; k < Sf; k += 64) {
                const float v = za[k];
                z_merged[ray * T + k + count_below(zc, S, v)] = v;
            }
            for (int j = lane; j < S; j += 64) {
                const float v = zc[j];
                z_merged[ray * T + j + count_not_above(za, Sf, v)] = v;
            }
        } else {
            // general case: rank sort of the concatenation
            for (int k = lane; k < T4; k += 64) if (k >= Sf) za[k] = k < T ? zc[k - Sf] : kInf;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            for (int k = lane; k < T; k += 64) {
                const float v = za[k];
                z_merged[ray * T + stable_rank(za, T4, v, k)] = v;
            }
        }
    }
}

size_t sample_pdf_lds_bytes(int S, int Sf) {
    const int S4 = (S + 3) & ~3, Sf4 = (Sf + 3) & ~3, T4 = (S + Sf + 3) & ~3;
    return (size_t)kPdfWaves * (S4 + S4 + Sf4 + T4) * sizeof(float);
}

void launch_sample_pdf(const float* weights, const float* z, long long N, int S, int Sf, const float* u,
                       uint64_t seed, long long ray_base, float* z_new, float* z_merged, hipStream_t stream) {
    if (N <= 0) return;
    const size_t lds = sample_pdf_lds_bytes(S, Sf);
    hipLaunchKernelGGL(sample_pdf_kernel, dim3((unsigned)((N + kPdfWaves - 1) / kPdfWaves)), dim3(64 * kPdfWaves),
                       lds, stream, weights, z, N, S, Sf, u, seed, ray_base, z_new, z_merged);
}

// ------------------------------------------------------------------------------------------------
// composite (ray_marching, src/UtilsNeuralRadianceField.py:88-115): ONE RAY PER WAVEFRONT.  The 64 lanes take 64
// consecutive samples (one coalesced 1 KiB read of the raw rows), alpha / sigmoid -- the expensive part -- are evaluated
// in parallel, the exclusive transmittance travels through the lanes in the canonical left-to-right order (below),
// carried from one 64-sample chunk to the next, and the rgb / depth sums are per-lane partial sums closed by a
// butterfly (same terms as a left-to-right loop, another association: a few ulps).  Same result on every run and
// for every batching of the rays.  The first version walked one ray per LANE: 64 wavefronts for a 4096-ray batch and
// a 3 KiB stride between the lanes of a load.
// SIGMA_ONLY (the coarse pass of a render, whose only output is the weights): raw is the compact (N*S,) sigma vector of
// mlp_f16x3_sig_kernel, only `weights` is written, and the weights are the same bits as the full kernel's.
// ------------------------------------------------------------------------------------------------
template <bool SIGMA_ONLY>
__global__ __launch_bounds__(256) void composite_kernel(const float* __restrict__ raw, const float* __restrict__ z,
                                                        long long N, int S, float* __restrict__ rgb,
                                                        float* __restrict__ weights, float* __restrict__ cumprod,
                                                        float* __restrict__ alpha_out, float* __restrict__ rgb_samples,
                                                        float* __restrict__ depth) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;                                        // uniform per wavefront
    const float4* rw = reinterpret_cast<const float4*>(raw) + r * S;
    const float* zr = z + r * S;
    float carry = 1.0f, c0 = 0.f, c1 = 0.f, c2 = 0.f, dep = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool in = s < S;
        const float4 o = SIGMA_ONLY ? make_float4(0.f, 0.f, 0.f, in ? raw[r * S + s] : 0.f)
                                    : in ? rw[s] : make_float4(0.f, 0.f, 0.f, 0.f);
        const float zc = in ? zr[s] : 0.f;
        const CompositeTerms ct = composite_terms(o, zr, s, S);
        const float a = ct.alpha, r0 = ct.r0, r1 = ct.r1, r2 = ct.r2;
        // Exclusive transmittance in the canonical order T_l = fl(T_(l-1) * (1 - alpha_(l-1))): lane l reads its left
        // neighbour through a one-lane wavefront shift (DPP wave_shr:1; lane 0 keeps the carry) and multiplies; after k
        // rounds lanes 0..k are final and recomputing them changes nothing, so 63 rounds of one shift + one multiply
        // finish the chunk.  (A tree-shaped prefix product is six steps, but neighbouring T then differ from the
        // ratio 1 - alpha by a few ulps -- the inverse-CDF sampler amplifies exactly that, by up to 1e5.)
        const float om = 1.0f - a;
        const float oms = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(1.0f), __float_as_int(om), 0x138, 0xf, 0xf, false));
        float T = lane == 0 ? carry : 1.0f;
        const int rounds = S - s0 < 64 ? S - s0 - 1 : 63;
        for (int k = 0; k < rounds; ++k) {
            const float Ts = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(T), __float_as_int(T), 0x138, 0xf, 0xf, false));
            T = Ts * (lane == 0 ? 1.0f : oms);
        }
        const float w = a * T;
        if constexpr (SIGMA_ONLY) {
            if (in) weights[r * S + s] = w;
            carry = __shfl(T * om, 63);
            continue;
        }
        c0 += w * r0; c1 += w * r1; c2 += w * r2; dep += w * zc;
        if (in) {
            const long long m = r * S + s;
            if (weights) weights[m] = w;
            if (cumprod) cumprod[m] = T;
            if (alpha_out) alpha_out[m] = a;
            if (rgb_samples) { rgb_samples[m * 3 + 0] = r0; rgb_samples[m * 3 + 1] = r1; rgb_samples[m * 3 + 2] = r2; }
        }
        carry = __shfl(T * om, 63);
    }
    if constexpr (SIGMA_ONLY) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); dep += __shfl_xor(dep, o);
    }
    if (lane == 0) {
        if (rgb) { rgb[r * 3 + 0] = c0; rgb[r * 3 + 1] = c1; rgb[r * 3 + 2] = c2; }
        if (depth) depth[r] = dep;
    }
}

void launch_composite(const float* raw, const float* z, long long N, int S, float* rgb, float* weights,
                      float* cumprod, float* alpha, float* rgb_samples, float* depth, hipStream_t stream) {
    if (N <= 0) return;
    hipLaunchKernelGGL(composite_kernel<false>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, raw, z, N, S,
                       rgb, weights, cumprod, alpha, rgb_samples, depth);
}

void launch_composite_weights(const float* sigma, const float* z, long long N, int S, float* weights, hipStream_t stream) {
    if (N <= 0) return;
    hipLaunchKernelGGL(composite_kernel<true>, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, stream, sigma, z, N, S,
                       nullptr, weights, nullptr, nullptr, nullptr, nullptr);
}

// ------------------------------------------------------------------------------------------------
// posenc (standalone): x (M,3) -> [x, sin0,cos0,...]*3 (passthrough) or [sin0,cos0,...]*3
// ------------------------------------------------------------------------------------------------
__global__ void posenc_kernel(const float* __restrict__ x, long long M, int n_enc, int passthrough,
                              float* __restrict__ out) {
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const int per = (passthrough ? 1 : 0) + 2 * n_enc;
    const float kPi = 3.1415927410125732f;
    for (int c = 0; c < 3; ++c) {
        const float v = x[m * 3 + c];
        float* o = out + m * (3 * per) + c * per;
        if (passthrough) *o++ = v;
        for (int k = 0; k < n_enc; ++k) {
            const float th = __fmul_rn(v, kPi * (float)(1 << k));
            o[2 * k] = sin_shifted(th, 0);
            o[2 * k + 1] = sin_shifted(th, 1);
        }
    }
}

void launch_posenc(const float* x, long long M, int n_enc, int passthrough, float* out, hipStream_t stream) {
    if (M <= 0) return;
    hipLaunchKernelGGL(posenc_kernel, dim3(blocks_for(M)), dim3(kBs), 0, stream, x, M, n_enc,
                       passthrough, out);
}

// ------------------------------------------------------------------------------------------------
// repack: weight blob -> one operand stream (and its constant block) through a gather table (nerf_kernels.h: launch_repack).
// E = _Float16 / __bf16: entry 2 * (src + 1) + is_lo -> the weight rounded to E (RNE), or what rounding left, rounded again;
// E = float: entry src + 1 -> the weight.  Entry 0: padding.  With a scale table (the encoding window: one float per blob
// element, build_scale_table) "the weight" is fl32(blob[src] * scale[src]): the product is rounded on its own, never fused
// into the hi / lo split.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float repack_weight(const float* __restrict__ blob, const float* __restrict__ scale, int32_t src) {
    const float w = blob[src];
    return scale ? __fmul_rn(w, scale[src]) : w;
}

template <class E>
__global__ void repack_kernel(const float* __restrict__ blob, const float* __restrict__ scale, const int32_t* __restrict__ idx,
                              E* __restrict__ out, size_t n, const int32_t* __restrict__ const_idx, float* __restrict__ cst) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int32_t t = idx[i];
        E v = (E)0.f;
        if constexpr (sizeof(E) == sizeof(float)) {
            if (t != 0) v = repack_weight(blob, scale, t - 1);
        } else if (t != 0) {
            const float w = repack_weight(blob, scale, (t >> 1) - 1);
            const E hi = (E)w;
            v = (t & 1) ? (E)(w - (float)hi) : hi;
        }
        out[i] = v;
    }
    if (const_idx && i < (size_t)kConstFloats) {
        const int32_t t = const_idx[i];
        cst[i] = t ? repack_weight(blob, scale, t - 1) : 0.f;
    }
}

void launch_repack(StreamElem elem, const float* blob, const float* scale, const int32_t* idx, void* out, size_t n,
                   const int32_t* const_idx, float* cst, hipStream_t s) {
    const dim3 grid((unsigned)((std::max(n, (size_t)kConstFloats) + 255) / 256)), block(256);
    if (elem == kElemF32) hipLaunchKernelGGL(repack_kernel<float>, grid, block, 0, s, blob, scale, idx, (float*)out, n, const_idx, cst);
    else if (elem == kElemBf16) hipLaunchKernelGGL(repack_kernel<__bf16>, grid, block, 0, s, blob, scale, idx, (__bf16*)out, n, const_idx, cst);
    else hipLaunchKernelGGL(repack_kernel<_Float16>, grid, block, 0, s, blob, scale, idx, (_Float16*)out, n, const_idx, cst);
}

}  // namespace nerf
