// volume_kernels.hip -- the radiance volume: an (n, n, n, 4) float32 lattice of (r, g, b, sigma) over a box, indexed
// [iz, iy, ix, channel], colour after the sigmoid and density after the ReLU (include/nerf_mi355.h: nerf_radiance_lattice has
// the format, nerf_volume_sample the trilinear rule, nerf_volume_march the march).  Here: the trilinear sampler, the march and
// their entry points.  The bake (nerf_radiance_lattice) is a field query: field_api.hip.
//
// Everything is float32 with every operation rounded on its own (the __f*_rn idiom of aux_kernels.hip), so the numpy
// restatement of tests/volume_ref.py matches the sampler bit for bit and the march up to expf.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "field_device.h"
#include "nerf_ctx.h"
#include "ray_box_device.h"

namespace nerf {
namespace {

// ---- trilinear sampling ----
// the volume's texels and the lattice they sit on: field_device.h's, so the sampler's step is the bake's by construction
struct VolumeArgs { const float4* texels; Lattice l; };

VolumeArgs volume_args(const float* volume, int n, const float* lo3, const float* hi3) {
    return {reinterpret_cast<const float4*>(volume), make_lattice(lo3, hi3, n)};
}

// One axis: the cell of coordinate p and the weight of the cell's upper vertex.  The cell is in [0, n - 2] for every input: a
// NaN compares false twice and lands in cell 0 (its weight stays NaN), +-Inf land in the last / first cell with weight 1 / 0.
__device__ __forceinline__ int volume_cell(float p, float lo, float step, int n, float* f) {
    const float g = __fdiv_rn(__fsub_rn(p, lo), step);
    const int i = g >= 0.0f ? (g < (float)(n - 1) ? (int)floorf(g) : n - 2) : 0;
    const float w = __fsub_rn(g, (float)i);
    *f = w < 0.0f ? 0.0f : (w > 1.0f ? 1.0f : w);
    return i;
}

// the eight texels of one cell, index = dx + 2 dy + 4 dz, and the three weights
struct CellFetch {
    float4 v[8];
    float f[3];
};

__device__ __forceinline__ void volume_fetch(const VolumeArgs& g, float px, float py, float pz, CellFetch* c) {
    const int n = g.l.n;
    const int ix = volume_cell(px, g.l.lo[0], g.l.step[0], n, &c->f[0]);
    const int iy = volume_cell(py, g.l.lo[1], g.l.step[1], n, &c->f[1]);
    const int iz = volume_cell(pz, g.l.lo[2], g.l.step[2], n, &c->f[2]);
    const float4* row = g.texels + ((size_t)iz * n + iy) * n + ix;     // ix + 1, iy + 1, iz + 1 <= n - 1
    const size_t sy = (size_t)n, sz = (size_t)n * n;
    c->v[0] = row[0];       c->v[1] = row[1];
    c->v[2] = row[sy];      c->v[3] = row[sy + 1];
    c->v[4] = row[sz];      c->v[5] = row[sz + 1];
    c->v[6] = row[sz + sy]; c->v[7] = row[sz + sy + 1];
}

__device__ __forceinline__ float lerp_rn(float a, float b, float f) { return __fadd_rn(a, __fmul_rn(f, __fsub_rn(b, a))); }

// along x, then y, then z
__device__ __forceinline__ float trilinear(float v0, float v1, float v2, float v3, float v4, float v5, float v6, float v7,
                                           const float f[3]) {
    const float v00 = lerp_rn(v0, v1, f[0]), v10 = lerp_rn(v2, v3, f[0]);
    const float v01 = lerp_rn(v4, v5, f[0]), v11 = lerp_rn(v6, v7, f[0]);
    return lerp_rn(lerp_rn(v00, v10, f[1]), lerp_rn(v01, v11, f[1]), f[2]);
}

__device__ __forceinline__ float4 volume_value(const CellFetch& c) {
    const float4* v = c.v;
    return make_float4(trilinear(v[0].x, v[1].x, v[2].x, v[3].x, v[4].x, v[5].x, v[6].x, v[7].x, c.f),
                       trilinear(v[0].y, v[1].y, v[2].y, v[3].y, v[4].y, v[5].y, v[6].y, v[7].y, c.f),
                       trilinear(v[0].z, v[1].z, v[2].z, v[3].z, v[4].z, v[5].z, v[6].z, v[7].z, c.f),
                       trilinear(v[0].w, v[1].w, v[2].w, v[3].w, v[4].w, v[5].w, v[6].w, v[7].w, c.f));
}

// one thread per point
__global__ void volume_sample_kernel(const VolumeArgs g, const float* __restrict__ points, long long M, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    CellFetch c;
    volume_fetch(g, points[3 * t + 0], points[3 * t + 1], points[3 * t + 2], &c);
    reinterpret_cast<float4*>(out)[t] = volume_value(c);
}

// ---- the march ----
// One thread per ray, 64 consecutive rays per wavefront, one wavefront per workgroup: a 256 x 256 frame is 1024 wavefronts,
// one per SIMD of the chip, so what hides the gathers' latency is the work one ray keeps in flight, not other wavefronts.  The
// sample positions do not depend on the transmittance: the ray fetches the cells of kAhead steps (8 x kAhead 16-byte gathers)
// and only then composites them, in order.  A ray under t_min stops fetching at the next group of steps; the steps of its
// last group past the stop, and a last group's steps past n_steps, are fetched (their cells are in the volume like any
// other) and not composited.  kAhead = 4 (161 VGPRs) against 2 and 8 (72, 300): 0.317 ms against 0.357 and 0.314 for the 256 x 256
// frame through n = 256 at 512 steps, 2.80 ms against 2.60 and 4.26 for 1024 x 1024 (profiles/volume_ahead_ab.json).
constexpr int kAhead = 4;

__global__ __launch_bounds__(64) void volume_march_kernel(const VolumeArgs g, const BoxArgs bx, const float* __restrict__ orig,
                                                          const float* __restrict__ dirs, long long N, int n_steps, float t_min,
                                                          float* __restrict__ rgb, float* __restrict__ depth,
                                                          float* __restrict__ opacity) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float4 o = reinterpret_cast<const float4*>(orig)[r], d = reinterpret_cast<const float4*>(dirs)[r];
    float a, b;
    bool hit = ray_box_hit(bx, o, d, &a, &b);
    // a ray with a non-finite component is a miss (ray_box_hit does not guard them: a NaN ray would "hit" on [near, far])
    hit = hit && finite_f(o.x) && finite_f(o.y) && finite_f(o.z) && finite_f(d.x) && finite_f(d.y) && finite_f(d.z);
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, cd = 0.0f, T = 1.0f;
    if (hit) {
        const float delta = __fdiv_rn(__fsub_rn(b, a), (float)n_steps);
        bool alive = true;
        for (int k0 = 0; k0 < n_steps && alive; k0 += kAhead) {
            CellFetch c[kAhead];
            float z[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                z[u] = __fadd_rn(a, __fmul_rn(__fadd_rn((float)(k0 + u), 0.5f), delta));
                volume_fetch(g, __fadd_rn(o.x, __fmul_rn(d.x, z[u])), __fadd_rn(o.y, __fmul_rn(d.y, z[u])),
                             __fadd_rn(o.z, __fmul_rn(d.z, z[u])), &c[u]);
            }
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const float4 v = volume_value(c[u]);
                const float e = expf(-__fmul_rn(v.w, delta));
                const float alpha = __fsub_rn(1.0f, e);
                const float w = __fmul_rn(alpha, T);
                const bool on = alive && k0 + u < n_steps;          // predicated, not branched: the body is a few selects
                cr = on ? __fadd_rn(cr, __fmul_rn(w, v.x)) : cr;
                cg = on ? __fadd_rn(cg, __fmul_rn(w, v.y)) : cg;
                cb = on ? __fadd_rn(cb, __fmul_rn(w, v.z)) : cb;
                cd = on ? __fadd_rn(cd, __fmul_rn(w, z[u])) : cd;
                T = on ? __fmul_rn(T, __fsub_rn(1.0f, alpha)) : T;
                alive = alive && !(on && T < t_min);
            }
        }
    }
    if (rgb) { rgb[3 * r + 0] = cr; rgb[3 * r + 1] = cg; rgb[3 * r + 2] = cb; }
    if (depth) depth[r] = cd;
    if (opacity) opacity[r] = __fsub_rn(1.0f, T);
}

// The trilinear sampler at points (M, 3) -> out (M, 4), and the march of N rays (any of rgb (N, 3), depth (N), opacity (N)
// nullable) through an (n, n, n, 4) volume over (lo3, hi3); the cell index is held in [0, n - 2] wherever the volume is read.
void launch_volume_sample(const float* volume, int n, const float* lo3, const float* hi3, const float* points, long long M,
                          float* out, hipStream_t stream) {
    if (M <= 0) return;
    hipLaunchKernelGGL(volume_sample_kernel, dim3(blocks_for(M)), dim3(kBs), 0, stream, volume_args(volume, n, lo3, hi3), points,
                       M, out);
}

void launch_volume_march(const float* volume, int n, const float* lo3, const float* hi3, float near_b, float far_b,
                         const float* orig, const float* dirs, long long N, int n_steps, float t_min, float* rgb, float* depth,
                         float* opacity, hipStream_t stream) {
    if (N <= 0) return;
    SceneBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo3[a]; box.hi[a] = hi3[a]; }
    hipLaunchKernelGGL(volume_march_kernel, dim3(blocks_for(N, 64)), dim3(64), 0, stream, volume_args(volume, n, lo3, hi3),
                       box_args(box, near_b, far_b), orig, dirs, N, n_steps, t_min, rgb, depth, opacity);
}

}  // namespace
}  // namespace nerf

using namespace nerf;

// the arguments every volume call shares
static int volume_ok(const char* what, const float* volume, int32_t n, const float* lo3, const float* hi3) {
    if (!volume || !lo3 || !hi3) return fail("NULL argument");
    if (int r = lattice_n_ok(what, n)) return r;
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(lo3[a]) || !std::isfinite(hi3[a]) || !(lo3[a] < hi3[a]))
            return fail("%s needs finite lo < hi on every axis (axis %d: lo %g, hi %g)", what, a, lo3[a], hi3[a]);
    return 0;
}

static int march_ok(int32_t n_steps, float t_min, const float* rgb, const float* depth, const float* opacity) {
    if (n_steps < 1) return fail("volume march: n_steps must be >= 1 (got %d)", n_steps);
    if (!(t_min >= 0.f && t_min < 1.f)) return fail("volume march: t_min must be in [0, 1) (got %g)", t_min);
    if (!rgb && !depth && !opacity) return fail("volume march: rgb, depth and opacity are all NULL");
    return 0;
}

extern "C" {

int nerf_volume_sample(nerf_ctx* c, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* points,
                       int64_t M, float* out, int mem) {
    ENTER(c);
    if (int r = volume_ok("volume sample", volume, n, lo3, hi3)) return r;
    if (M < 0) return fail("bad shape M=%lld", (long long)M);
    if (M == 0) return 0;
    if (!points || !out) return fail("NULL argument");
    Staging st(c, mem);
    const float* vol = st.in(c->b_lattice, volume, (size_t)n * n * n * 16);
    const float* p = st.in(c->b_in0, points, (size_t)M * 12);
    float* o = st.out(c->b_raw, out, (size_t)M * 16);
    if (st.err) return st.err;
    launch_volume_sample(vol, n, lo3, hi3, p, M, o, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_volume_march(nerf_ctx* c, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* rays_orig,
                      const float* rays_dirs, int64_t N, int32_t n_steps, float t_min, float* rgb, float* depth, float* opacity,
                      int mem) {
    ENTER(c);
    if (int r = volume_ok("volume march", volume, n, lo3, hi3)) return r;
    if (int r = march_ok(n_steps, t_min, rgb, depth, opacity)) return r;
    if (N < 0) return fail("bad shape N=%lld", (long long)N);
    if (N == 0) return 0;
    if (!rays_orig || !rays_dirs) return fail("NULL argument");
    Staging st(c, mem);
    const float* vol = st.in(c->b_lattice, volume, (size_t)n * n * n * 16);
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    float* drgb = st.out(c->b_out[0], rgb, (size_t)N * 12);
    float* ddepth = st.out(c->b_out[1], depth, (size_t)N * 4);
    float* dopac = st.out(c->b_out[2], opacity, (size_t)N * 4);
    if (st.err) return st.err;
    launch_volume_march(vol, n, lo3, hi3, c->cfg.near_boundary, c->cfg.far_boundary, o, d, N, n_steps, t_min, drgb, ddepth, dopac,
                        c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

int nerf_volume_render_image(nerf_ctx* c, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* c2w,
                             float fov, int32_t H, int32_t W, int64_t ray_begin, int64_t ray_count, int32_t n_steps, float t_min,
                             float* rgb, float* depth, float* opacity, int mem) {
    ENTER(c);
    if (int r = volume_ok("volume render", volume, n, lo3, hi3)) return r;
    if (int r = march_ok(n_steps, t_min, rgb, depth, opacity)) return r;
    if (!c2w) return fail("NULL argument");
    if (H <= 0 || W <= 0) return fail("bad image size %dx%d", H, W);
    const long long total = (long long)H * W;
    if (ray_count <= 0) { ray_begin = 0; ray_count = total; }
    if (ray_begin < 0 || ray_begin + ray_count > total) return fail("ray slab [%lld,+%lld) outside %lld rays",
                                                                    (long long)ray_begin, (long long)ray_count, total);
    const long long N = ray_count, batch = std::min<long long>(N, 1 << 18);
    if (int r = ensure(c, c->b_orig, (size_t)batch * 16)) return r;
    if (int r = ensure(c, c->b_dirs, (size_t)batch * 16)) return r;
    Staging st(c, mem);
    const float* vol = st.in(c->b_lattice, volume, (size_t)n * n * n * 16);
    float* drgb = st.out(c->b_out[0], rgb, (size_t)N * 12);
    float* ddepth = st.out(c->b_out[1], depth, (size_t)N * 4);
    float* dopac = st.out(c->b_out[2], opacity, (size_t)N * 4);
    if (st.err) return st.err;
    float *o = (float*)c->b_orig.p, *d = (float*)c->b_dirs.p;
    for (long long off = 0; off < N; off += batch) {      // the rays of nerf_render_image, batch by batch on the stream
        const long long m = std::min(batch, N - off);
        launch_raygen(c2w, fov, H, W, ray_begin + off, m, o, d, c->stream);
        if (c->ray_space == NERF_RAYS_NDC) launch_rays_to_ndc(o, d, m, fov, c->ndc_near_plane, o, d, c->stream);
        launch_volume_march(vol, n, lo3, hi3, c->cfg.near_boundary, c->cfg.far_boundary, o, d, m, n_steps, t_min,
                            drgb ? drgb + 3 * off : nullptr, ddepth ? ddepth + off : nullptr, dopac ? dopac + off : nullptr,
                            c->stream);
    }
    HIP_OK(hipGetLastError());
    return st.finish();
}

}  // extern "C"
