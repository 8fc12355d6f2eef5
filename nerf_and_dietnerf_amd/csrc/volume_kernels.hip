// volume_kernels.hip -- the radiance volume: an (n, n, n, 4) float32 lattice of (r, g, b, sigma) over a box, indexed
// [iz, iy, ix, channel], colour after the sigmoid and density after the ReLU (include/nerf_mi355.h: nerf_radiance_lattice has
// the format, nerf_volume_sample the trilinear rule, nerf_volume_march the march), and the SH volume -- K spherical-harmonic
// coefficients per colour and vertex in place of one colour (nerf_sh_radiance_lattice has the format).  Here: the trilinear
// sampler and the march, each written once over the two formats, and their entry points.  The bakes (nerf_radiance_lattice,
// nerf_sh_radiance_lattice) are field queries: field_api.hip.
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
// the volume's texels and the lattice they sit on: field_device.h's, so the sampler's step is the bake's by construction.  A
// texel is Q float4: 1 in the plain format, C(L) / 4 in the SH format of degree L.
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

// ---- view-dependent colour: spherical harmonics per vertex (include/nerf_mi355.h: nerf_sh_radiance_lattice has the format, the
// basis and the direction rule, nerf_sh_volume_sample the per-point rule) ----
// A texel is Q = C(L) / 4 float4: channel 3 k + c the coefficient of basis function k for colour c, channel 3 K sigma.

// u = d / |d|, (0, 0, 1) where |d|^2 is 0 or not finite
__device__ __forceinline__ void sh_unit(float dx, float dy, float dz, float u[3]) {
    const float s = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
    const bool ok = s != 0.0f && finite_f(s);
    const float r = sqrtf(s);      // correctly rounded (hipcc's default for fp32 sqrt); HIP's __fsqrt_rn is the native approximation
    u[0] = ok ? __fdiv_rn(dx, r) : 0.0f;
    u[1] = ok ? __fdiv_rn(dy, r) : 0.0f;
    u[2] = ok ? __fdiv_rn(dz, r) : 1.0f;
}

// Y_0 .. Y_{K-1} at u, in the header's operation order
template <int L>
__device__ __forceinline__ void sh_basis(const float u[3], float* Y) {
    const float x = u[0], y = u[1], z = u[2];
    Y[0] = 0.28209479177387814f;
    if constexpr (L >= 1) {
        Y[1] = __fmul_rn(0.4886025119029199f, y);
        Y[2] = __fmul_rn(0.4886025119029199f, z);
        Y[3] = __fmul_rn(0.4886025119029199f, x);
    }
    if constexpr (L >= 2) {
        const float xx = __fmul_rn(x, x), yy = __fmul_rn(y, y), zz = __fmul_rn(z, z);
        const float xy = __fmul_rn(x, y), yz = __fmul_rn(y, z), xz = __fmul_rn(x, z);
        Y[4] = __fmul_rn(1.0925484305920792f, xy);
        Y[5] = __fmul_rn(1.0925484305920792f, yz);
        Y[6] = __fmul_rn(0.31539156525252005f, __fsub_rn(__fmul_rn(3.0f, zz), 1.0f));
        Y[7] = __fmul_rn(1.0925484305920792f, xz);
        Y[8] = __fmul_rn(0.5462742152960396f, __fsub_rn(xx, yy));
        if constexpr (L >= 3) {
            const float zz5 = __fmul_rn(5.0f, zz);
            Y[9] = __fmul_rn(0.5900435899266435f, __fmul_rn(y, __fsub_rn(__fmul_rn(3.0f, xx), yy)));
            Y[10] = __fmul_rn(2.890611442640554f, __fmul_rn(xy, z));
            Y[11] = __fmul_rn(0.4570457994644658f, __fmul_rn(y, __fsub_rn(zz5, 1.0f)));
            Y[12] = __fmul_rn(0.3731763325901154f, __fmul_rn(z, __fsub_rn(zz5, 3.0f)));
            Y[13] = __fmul_rn(0.4570457994644658f, __fmul_rn(x, __fsub_rn(zz5, 1.0f)));
            Y[14] = __fmul_rn(1.445305721320277f, __fmul_rn(z, __fsub_rn(xx, yy)));
            Y[15] = __fmul_rn(0.5900435899266435f, __fmul_rn(x, __fsub_rn(xx, __fmul_rn(3.0f, yy))));
        }
    }
}

// One vertex towards Y -> (r, g, b, sigma), the colour not yet clamped.  The texel streams through as Q 16-byte loads, every
// value used as it arrives: the index arithmetic below is all compile-time once the loops are unrolled.
template <int L>
__device__ __forceinline__ float4 sh_vertex(const float4* __restrict__ texel, const float* Y) {
    constexpr int K = sh_basis_count(L), Q = sh_texel_floats(L) / 4;
    float acc[3] = {0.0f, 0.0f, 0.0f}, sigma = 0.0f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const float4 v = texel[q];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int ch = 4 * q + i;
            if (ch < 3 * K) {
                const float term = __fmul_rn(Y[ch / 3], e[i]);
                acc[ch % 3] = ch < 3 ? term : __fadd_rn(acc[ch % 3], term);
            } else if (ch == 3 * K) {
                sigma = e[i];
            }
        }
    }
    return make_float4(acc[0], acc[1], acc[2], sigma);
}

__device__ __forceinline__ float clamp01(float x) { return x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x); }      // a NaN stays
__device__ __forceinline__ float4 clamp_colour(float4 v) { return make_float4(clamp01(v.x), clamp01(v.y), clamp01(v.z), v.w); }

// the cell of a point: the texel of its lowest vertex and the three weights
template <int L>
__device__ __forceinline__ const float4* sh_cell(const VolumeArgs& g, float px, float py, float pz, float f[3]) {
    const int n = g.l.n;
    const int ix = volume_cell(px, g.l.lo[0], g.l.step[0], n, &f[0]);
    const int iy = volume_cell(py, g.l.lo[1], g.l.step[1], n, &f[1]);
    const int iz = volume_cell(pz, g.l.lo[2], g.l.step[2], n, &f[2]);
    return g.texels + (((size_t)iz * n + iy) * n + ix) * (sh_texel_floats(L) / 4);      // ix + 1, iy + 1, iz + 1 <= n - 1
}

// all eight vertices of a cell by one lane -> the interpolated, clamped value
template <int L>
__device__ __forceinline__ float4 sh_value(const VolumeArgs& g, float px, float py, float pz, const float* Y) {
    constexpr size_t Q = sh_texel_floats(L) / 4;
    float f[3];
    const float4* row = sh_cell<L>(g, px, py, pz, f);
    const size_t sy = (size_t)g.l.n * Q, sz = (size_t)g.l.n * g.l.n * Q;
    CellFetch c;
    c.f[0] = f[0]; c.f[1] = f[1]; c.f[2] = f[2];
    c.v[0] = sh_vertex<L>(row, Y);           c.v[1] = sh_vertex<L>(row + Q, Y);
    c.v[2] = sh_vertex<L>(row + sy, Y);      c.v[3] = sh_vertex<L>(row + sy + Q, Y);
    c.v[4] = sh_vertex<L>(row + sz, Y);      c.v[5] = sh_vertex<L>(row + sz + Q, Y);
    c.v[6] = sh_vertex<L>(row + sz + sy, Y); c.v[7] = sh_vertex<L>(row + sz + sy + Q, Y);
    return clamp_colour(volume_value(c));
}

// ---- the two formats, as the sampler and the march see them ----
// Either type gives "the value of the volume at a point, seen along a direction" to the thread that asks: towards() makes what
// depends on the direction alone, K floats Y that the asking kernel keeps in a local array (as a member of a value of the
// type, Y changed the register allocation of the SH marches of degree 1 to 3); fetch() starts the value at a point and leaves
// an InFlight behind, value() finishes it, so that a march can start Ahead steps before it finishes the first.
//
// The plain format.  Only the sampler asks it: its march is spelled out (volume_march_kernel<PlainVolume>), so it has neither
// towards() nor Ahead.
struct PlainVolume {
    static constexpr int K = 1;
    static constexpr bool ViewDependent = false;                      // the same along every direction: Y stays unused
    using InFlight = CellFetch;                                       // the eight texels, not yet interpolated
    static __device__ __forceinline__ void fetch(const VolumeArgs& g, float px, float py, float pz, const float*, InFlight* c) {
        volume_fetch(g, px, py, pz, c);
    }
    static __device__ __forceinline__ float4 value(const InFlight& c) { return volume_value(c); }
};

// The SH format of degree L.  A step gathers 8 x Q float4 per ray -- 8 / 32 / 56 / 104 -- where the plain format gathers 8, so
// holding the cells of the steps in flight does not carry over: sh_vertex consumes a vertex's loads as they arrive, a step leaves
// 4 values behind, and kShAhead[L] steps are in flight.  u and Y are made once, with the value: once per ray in the march.
constexpr int kShAhead[kShMaxDegree + 1] = {4, 2, 1, 1};      // one lane per ray: steps in flight

template <int L>
struct ShVolume {
    static constexpr int Degree = L, Ahead = kShAhead[L], K = sh_basis_count(L);
    static constexpr bool ViewDependent = true;
    using InFlight = float4;                                          // the value itself
    static __device__ __forceinline__ void towards(float dx, float dy, float dz, float* Y) {
        float u[3];
        sh_unit(dx, dy, dz, u);
        sh_basis<L>(u, Y);
    }
    static __device__ __forceinline__ void fetch(const VolumeArgs& g, float px, float py, float pz, const float* Y, InFlight* c) {
        *c = sh_value<L>(g, px, py, pz, Y);
    }
    static __device__ __forceinline__ float4 value(const InFlight& c) { return c; }
};

// one thread per point; dirs (M, 3) is read by the SH formats alone (NULL for the plain one)
template <class Format>
__global__ void volume_sample_kernel(const VolumeArgs g, const float* __restrict__ points, const float* __restrict__ dirs,
                                     long long M, float* __restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= M) return;
    float Y[Format::K];
    if constexpr (Format::ViewDependent) Format::towards(dirs[3 * t + 0], dirs[3 * t + 1], dirs[3 * t + 2], Y);
    typename Format::InFlight c;
    Format::fetch(g, points[3 * t + 0], points[3 * t + 1], points[3 * t + 2], Y, &c);
    reinterpret_cast<float4*>(out)[t] = Format::value(c);
}

// ---- the march ----
// One lane per ray over either format; a ray under t_min stops fetching at the next group of steps; the steps of its last group
// past the stop, and a last group's steps past n_steps, are fetched (their cells are in the volume like any other) and not
// composited.  For the SH format there is a second mapping, the same arithmetic in the same order, hence the same bits
// (profiles/sh_volume_measure.json has both):
//   one lane per ray     volume_march_kernel<ShVolume<L>>.
//   eight lanes per ray  one cell vertex each: a lane streams its own texel (Q contiguous 16-byte loads; the two x-neighbours
//                        are 2 Q contiguous float4), the three lerps run across lanes -- x between lanes 1 apart, y 2 apart,
//                        z 4 apart, each lane picking lower and upper by its own bit, so all eight end with the step's value
//                        and composite it alike.  A 256 x 256 frame is 8 wavefronts per SIMD: other wavefronts hide the
//                        latency, and two steps are in flight per lane.
// Neither wins everywhere (kShEightLanes has the times and the choice): at degrees 0 and 1 a lane's own 8 or 32 gathers
// keep it busy and the eight-lane form pays its eightfold address and compositing arithmetic for nothing; at degree 3 one
// lane's 104 gathers a step need 256 VGPRs and leave one wavefront per SIMD with nothing to switch to.

// per ray: the box interval and, for a hit, the step
struct MarchRay { float4 o, d; float a, delta; bool hit; };

__device__ __forceinline__ MarchRay march_ray(const BoxArgs& bx, const float* orig, const float* dirs, long long r, int n_steps) {
    MarchRay m;
    m.o = reinterpret_cast<const float4*>(orig)[r];
    m.d = reinterpret_cast<const float4*>(dirs)[r];
    float b;
    m.hit = ray_box_hit(bx, m.o, m.d, &m.a, &b);
    // a ray with a non-finite component is a miss (ray_box_hit does not guard them: a NaN ray would "hit" on [near, far])
    m.hit = m.hit && finite_f(m.o.x) && finite_f(m.o.y) && finite_f(m.o.z) && finite_f(m.d.x) && finite_f(m.d.y) && finite_f(m.d.z);
    m.delta = __fdiv_rn(__fsub_rn(b, m.a), (float)n_steps);
    return m;
}

// steps 4 and 5 of nerf_volume_march for one sample
struct MarchSums { float cr = 0.0f, cg = 0.0f, cb = 0.0f, cd = 0.0f, T = 1.0f; bool alive = true; };

__device__ __forceinline__ void march_step(MarchSums& s, float4 v, float z, float delta, bool in_range, float t_min) {
    const float e = expf(-__fmul_rn(v.w, delta));
    const float alpha = __fsub_rn(1.0f, e);
    const float w = __fmul_rn(alpha, s.T);
    const bool on = s.alive && in_range;                  // predicated, not branched: the body is a few selects
    s.cr = on ? __fadd_rn(s.cr, __fmul_rn(w, v.x)) : s.cr;
    s.cg = on ? __fadd_rn(s.cg, __fmul_rn(w, v.y)) : s.cg;
    s.cb = on ? __fadd_rn(s.cb, __fmul_rn(w, v.z)) : s.cb;
    s.cd = on ? __fadd_rn(s.cd, __fmul_rn(w, z)) : s.cd;
    s.T = on ? __fmul_rn(s.T, __fsub_rn(1.0f, alpha)) : s.T;
    s.alive = s.alive && !(on && s.T < t_min);
}

__device__ __forceinline__ void march_store(const MarchSums& s, long long r, float* rgb, float* depth, float* opacity) {
    if (rgb) { rgb[3 * r + 0] = s.cr; rgb[3 * r + 1] = s.cg; rgb[3 * r + 2] = s.cb; }
    if (depth) depth[r] = s.cd;
    if (opacity) opacity[r] = __fsub_rn(1.0f, s.T);
}

__device__ __forceinline__ float step_depth(float a, float delta, int k) {
    return __fadd_rn(a, __fmul_rn(__fadd_rn((float)k, 0.5f), delta));
}

template <class Format>
__global__ __launch_bounds__(64) void volume_march_kernel(const VolumeArgs g, const BoxArgs bx, const float* __restrict__ orig,
                                                          const float* __restrict__ dirs, long long N, int n_steps, float t_min,
                                                          float* __restrict__ rgb, float* __restrict__ depth,
                                                          float* __restrict__ opacity) {
    constexpr int A = Format::Ahead;
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const MarchRay m = march_ray(bx, orig, dirs, r, n_steps);
    MarchSums s;
    if (m.hit) {
        float Y[Format::K];
        Format::towards(m.d.x, m.d.y, m.d.z, Y);
        for (int k0 = 0; k0 < n_steps && s.alive; k0 += A) {
            typename Format::InFlight c[A];
            float z[A];
#pragma unroll
            for (int i = 0; i < A; ++i) {
                z[i] = step_depth(m.a, m.delta, k0 + i);
                Format::fetch(g, __fadd_rn(m.o.x, __fmul_rn(m.d.x, z[i])), __fadd_rn(m.o.y, __fmul_rn(m.d.y, z[i])),
                              __fadd_rn(m.o.z, __fmul_rn(m.d.z, z[i])), Y, &c[i]);
            }
#pragma unroll
            for (int i = 0; i < A; ++i) march_step(s, Format::value(c[i]), z[i], m.delta, k0 + i < n_steps, t_min);
        }
    }
    march_store(s, r, rgb, depth, opacity);
}

// The plain format's march.  One thread per ray, 64 consecutive rays per wavefront, one wavefront per workgroup: a 256 x 256
// frame is 1024 wavefronts, one per SIMD of the chip, so what hides the gathers' latency is the work one ray keeps in flight, not
// other wavefronts.  The sample positions do not depend on the transmittance: the ray fetches the cells of kAhead steps
// (8 x kAhead 16-byte gathers) and only then composites them, in order.  kAhead = 4 (161 VGPRs) against 2 and 8 (72, 300):
// 0.317 ms against 0.357 and 0.314 for the 256 x 256 frame through n = 256 at 512 steps, 2.80 ms against 2.60 and 4.26 for
// 1024 x 1024 (profiles/volume_ahead_ab.json).
// It is the body above with InFlight = CellFetch, spelled out as it was before that body was shared: the same operations in the
// same order, so the same bits, but the shared body compiles to 16 instructions fewer in another schedule and measured 0.7 %
// slower on that frame with t_min = 1 / 512 (0.3149 against 0.3127 ms, medians of three fresh processes each whose own medians
// lie within 0.0003 and 0.0002 ms; equal at t_min = 0; profiles/volume_refactor_ab_shared_body.json).  That is over the bar set
// for the change, the parent's own range; processes of identical code differed by as much in a later call
// (profiles/volume_refactor_ab.json), so a slower kernel is not established.  Both bodies are held to tests/volume_ref.py's
// march by tests/test_gpu_volume.py and tests/test_gpu_sh_volume.py.
constexpr int kAhead = 4;

template <>
__global__ __launch_bounds__(64) void volume_march_kernel<PlainVolume>(const VolumeArgs g, const BoxArgs bx,
                                                                       const float* __restrict__ orig,
                                                                       const float* __restrict__ dirs, long long N, int n_steps,
                                                                       float t_min, float* __restrict__ rgb,
                                                                       float* __restrict__ depth, float* __restrict__ opacity) {
    const long long r = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float4 o = reinterpret_cast<const float4*>(orig)[r], d = reinterpret_cast<const float4*>(dirs)[r];
    float a, b;
    bool hit = ray_box_hit(bx, o, d, &a, &b);
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
                const bool on = alive && k0 + u < n_steps;
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

constexpr int kShCornerAhead = 2;                            // eight lanes per ray: steps in flight

// the value of the lane `Mask` away (1, 2: inside the quad, a DPP move; 4: a swizzle of the 32-lane half)
template <int Mask>
__device__ __forceinline__ float lane_xor(float v) {
    const int x = __float_as_int(v);
    if constexpr (Mask == 1) return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false));      // quad_perm:[1,0,3,2]
    else if constexpr (Mask == 2) return __int_as_float(__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false)); // quad_perm:[2,3,0,1]
    else return __int_as_float(__builtin_amdgcn_ds_swizzle(x, 0x101F));                     // bit mode: and 0x1f, or 0, xor 4
}

// lerp_rn between this lane's value and that of the lane Mask away: the lane whose bit is clear holds the lower vertex
template <int Mask>
__device__ __forceinline__ float4 lerp_lanes(float4 mine, float f, bool upper) {
    const float4 other = make_float4(lane_xor<Mask>(mine.x), lane_xor<Mask>(mine.y), lane_xor<Mask>(mine.z), lane_xor<Mask>(mine.w));
    const float4 lo = upper ? other : mine, hi = upper ? mine : other;
    return make_float4(lerp_rn(lo.x, hi.x, f), lerp_rn(lo.y, hi.y, f), lerp_rn(lo.z, hi.z, f), lerp_rn(lo.w, hi.w, f));
}

// ray = thread / 8, vertex = thread % 8 = dx + 2 dy + 4 dz; the eight lanes of a ray share every branch
template <int L>
__global__ __launch_bounds__(256) void sh_march_corner_kernel(const VolumeArgs g, const BoxArgs bx, const float* __restrict__ orig,
                                                              const float* __restrict__ dirs, long long N, int n_steps,
                                                              float t_min, float* __restrict__ rgb, float* __restrict__ depth,
                                                              float* __restrict__ opacity) {
    constexpr int A = kShCornerAhead;
    constexpr size_t Q = sh_texel_floats(L) / 4;
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long r = t >> 3;
    if (r >= N) return;
    const int corner = (int)(threadIdx.x & 7);
    const bool ux = corner & 1, uy = corner & 2, uz = corner & 4;
    const size_t mine = (ux ? Q : 0) + (uy ? (size_t)g.l.n * Q : 0) + (uz ? (size_t)g.l.n * g.l.n * Q : 0);
    const MarchRay m = march_ray(bx, orig, dirs, r, n_steps);
    MarchSums s;
    if (m.hit) {
        float Y[ShVolume<L>::K];
        ShVolume<L>::towards(m.d.x, m.d.y, m.d.z, Y);
        for (int k0 = 0; k0 < n_steps && s.alive; k0 += A) {
            float4 v[A];
            float z[A], f[A][3];
#pragma unroll
            for (int i = 0; i < A; ++i) {
                z[i] = step_depth(m.a, m.delta, k0 + i);
                const float4* row = sh_cell<L>(g, __fadd_rn(m.o.x, __fmul_rn(m.d.x, z[i])), __fadd_rn(m.o.y, __fmul_rn(m.d.y, z[i])),
                                               __fadd_rn(m.o.z, __fmul_rn(m.d.z, z[i])), f[i]);
                v[i] = sh_vertex<L>(row + mine, Y);
            }
#pragma unroll
            for (int i = 0; i < A; ++i) {
                const float4 along_x = lerp_lanes<1>(v[i], f[i][0], ux);
                const float4 along_y = lerp_lanes<2>(along_x, f[i][1], uy);
                march_step(s, clamp_colour(lerp_lanes<4>(along_y, f[i][2], uz)), z[i], m.delta, k0 + i < n_steps, t_min);
            }
        }
    }
    if (corner == 0) march_store(s, r, rgb, depth, opacity);
}

// ---- launches ----
// a stored format on the host: plain, or SH of a degree in 0..3 (volume_ok's check)
struct VolumeFormat {
    bool sh;
    int degree;
    size_t texel_bytes() const { return sh ? (size_t)sh_texel_floats(degree) * 4 : 16; }
};

// fn(Format{}) for the format's type
template <class Fn>
void with_format(VolumeFormat f, Fn&& fn) {
    if (!f.sh) return fn(PlainVolume{});
    switch (f.degree) {
        case 0: return fn(ShVolume<0>{});
        case 1: return fn(ShVolume<1>{});
        case 2: return fn(ShVolume<2>{});
        default: return fn(ShVolume<3>{});
    }
}

// The SH march's mapping is chosen per degree by the time of a 256 x 256 frame through n = 256 at 512 steps
// (profiles/sh_volume_measure.json), one lane against eight lanes per ray: 0.42 / 1.28 ms at degree 0, 1.04 / 1.41 at 1,
// 1.92 / 1.85 at 2, 9.02 / 3.46 at 3 (256 VGPRs, one wavefront per SIMD).
// -DNERF_SH_MARCH_LANES=1 or 8 forces one mapping for every degree: the A/B builds of tools/sh_volume_measure.py.
#ifdef NERF_SH_MARCH_LANES
constexpr bool kShEightLanes[kShMaxDegree + 1] = {NERF_SH_MARCH_LANES == 8, NERF_SH_MARCH_LANES == 8, NERF_SH_MARCH_LANES == 8,
                                                  NERF_SH_MARCH_LANES == 8};
#else
constexpr bool kShEightLanes[kShMaxDegree + 1] = {false, false, true, true};
#endif

// The trilinear sampler at points (M, 3), seen along dirs (M, 3; the SH formats alone) -> out (M, 4), and the march of N rays
// (any of rgb (N, 3), depth (N), opacity (N) nullable) through a volume over (lo3, hi3); the cell index is held in [0, n - 2]
// wherever the volume is read.
void launch_volume_sample(VolumeFormat f, const float* volume, int n, const float* lo3, const float* hi3, const float* points,
                          const float* dirs, long long M, float* out, hipStream_t stream) {
    if (M <= 0) return;
    const VolumeArgs g = volume_args(volume, n, lo3, hi3);
    with_format(f, [&](auto format) {
        hipLaunchKernelGGL(volume_sample_kernel<decltype(format)>, dim3(blocks_for(M)), dim3(kBs), 0, stream, g, points, dirs, M, out);
    });
}

void launch_volume_march(VolumeFormat f, const float* volume, int n, const float* lo3, const float* hi3, float near_b, float far_b,
                         const float* orig, const float* dirs, long long N, int n_steps, float t_min, float* rgb, float* depth,
                         float* opacity, hipStream_t stream) {
    if (N <= 0) return;
    SceneBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = lo3[a]; box.hi[a] = hi3[a]; }
    const VolumeArgs g = volume_args(volume, n, lo3, hi3);
    const BoxArgs bx = box_args(box, near_b, far_b);
    with_format(f, [&](auto format) {
        using Format = decltype(format);
        if constexpr (Format::ViewDependent) {
            if (kShEightLanes[Format::Degree]) {
                hipLaunchKernelGGL(sh_march_corner_kernel<Format::Degree>, dim3(blocks_for(8 * N)), dim3(kBs), 0, stream, g, bx, orig,
                                   dirs, N, n_steps, t_min, rgb, depth, opacity);
                return;
            }
        }
        hipLaunchKernelGGL(volume_march_kernel<Format>, dim3(blocks_for(N, 64)), dim3(64), 0, stream, g, bx, orig, dirs, N, n_steps,
                           t_min, rgb, depth, opacity);
    });
}

}  // namespace
}  // namespace nerf

using namespace nerf;

// ---- entry points: one body each for sample, march and render-image, over the format ----
// the `what` of a refusal
enum VolumeCall { kSample, kMarch, kRender };
static const char* what_of(VolumeFormat f, VolumeCall call) {
    static const char* const names[2][3] = {{"volume sample", "volume march", "volume render"},
                                            {"SH volume sample", "SH volume march", "SH volume render"}};
    return names[f.sh][call];
}

// the arguments every volume call shares
static int volume_ok(const char* what, const float* volume, int32_t n, VolumeFormat f, const float* lo3, const float* hi3) {
    if (!volume || !lo3 || !hi3) return fail("NULL argument");
    if (int r = lattice_n_ok(what, n)) return r;
    if (f.sh && (f.degree < 0 || f.degree > kShMaxDegree))
        return fail("%s: degree must be in 0..%d (got %d)", what, kShMaxDegree, f.degree);
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

static int volume_sample(nerf_ctx* c, VolumeFormat f, const float* volume, int32_t n, const float* lo3, const float* hi3,
                         const float* points, const float* dirs, int64_t M, float* out, int mem) {
    ENTER(c);
    if (int r = volume_ok(what_of(f, kSample), volume, n, f, lo3, hi3)) return r;
    if (M < 0) return fail("bad shape M=%lld", (long long)M);
    if (M == 0) return 0;
    if (!points || (f.sh && !dirs) || !out) return fail("NULL argument");
    Staging st(c, mem);
    const float* vol = st.in(c->b_lattice, volume, (size_t)n * n * n * f.texel_bytes());
    const float* p = st.in(c->b_in0, points, (size_t)M * 12);
    const float* d = f.sh ? st.in(c->b_in1, dirs, (size_t)M * 12) : nullptr;
    float* o = st.out(c->b_raw, out, (size_t)M * 16);
    if (st.err) return st.err;
    launch_volume_sample(f, vol, n, lo3, hi3, p, d, M, o, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

static int volume_march(nerf_ctx* c, VolumeFormat f, const float* volume, int32_t n, const float* lo3, const float* hi3,
                        const float* rays_orig, const float* rays_dirs, int64_t N, int32_t n_steps, float t_min, float* rgb,
                        float* depth, float* opacity, int mem) {
    ENTER(c);
    if (int r = volume_ok(what_of(f, kMarch), volume, n, f, lo3, hi3)) return r;
    if (int r = march_ok(n_steps, t_min, rgb, depth, opacity)) return r;
    if (N < 0) return fail("bad shape N=%lld", (long long)N);
    if (N == 0) return 0;
    if (!rays_orig || !rays_dirs) return fail("NULL argument");
    Staging st(c, mem);
    const float* vol = st.in(c->b_lattice, volume, (size_t)n * n * n * f.texel_bytes());
    const float* o = st.in(c->b_orig, rays_orig, (size_t)N * 16);
    const float* d = st.in(c->b_dirs, rays_dirs, (size_t)N * 16);
    float* drgb = st.out(c->b_out[0], rgb, (size_t)N * 12);
    float* ddepth = st.out(c->b_out[1], depth, (size_t)N * 4);
    float* dopac = st.out(c->b_out[2], opacity, (size_t)N * 4);
    if (st.err) return st.err;
    launch_volume_march(f, vol, n, lo3, hi3, c->cfg.near_boundary, c->cfg.far_boundary, o, d, N, n_steps, t_min, drgb, ddepth,
                        dopac, c->stream);
    HIP_OK(hipGetLastError());
    return st.finish();
}

static int volume_render_image(nerf_ctx* c, VolumeFormat f, const float* volume, int32_t n, const float* lo3, const float* hi3,
                               const float* c2w, float fov, int32_t H, int32_t W, int64_t ray_begin, int64_t ray_count,
                               int32_t n_steps, float t_min, float* rgb, float* depth, float* opacity, int mem) {
    ENTER(c);
    if (int r = volume_ok(what_of(f, kRender), volume, n, f, lo3, hi3)) return r;
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
    const float* vol = st.in(c->b_lattice, volume, (size_t)n * n * n * f.texel_bytes());
    float* drgb = st.out(c->b_out[0], rgb, (size_t)N * 12);
    float* ddepth = st.out(c->b_out[1], depth, (size_t)N * 4);
    float* dopac = st.out(c->b_out[2], opacity, (size_t)N * 4);
    if (st.err) return st.err;
    float *o = (float*)c->b_orig.p, *d = (float*)c->b_dirs.p;
    for (long long off = 0; off < N; off += batch) {      // the rays of nerf_render_image, batch by batch on the stream
        const long long m = std::min(batch, N - off);
        launch_raygen(c2w, fov, H, W, ray_begin + off, m, o, d, c->stream);
        if (c->ray_space == NERF_RAYS_NDC) launch_rays_to_ndc(o, d, m, fov, c->ndc_near_plane, o, d, c->stream);
        launch_volume_march(f, vol, n, lo3, hi3, c->cfg.near_boundary, c->cfg.far_boundary, o, d, m, n_steps, t_min,
                            drgb ? drgb + 3 * off : nullptr, ddepth ? ddepth + off : nullptr, dopac ? dopac + off : nullptr,
                            c->stream);
    }
    HIP_OK(hipGetLastError());
    return st.finish();
}

extern "C" {

int nerf_volume_sample(nerf_ctx* c, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* points,
                       int64_t M, float* out, int mem) {
    return volume_sample(c, {false, 0}, volume, n, lo3, hi3, points, nullptr, M, out, mem);
}

int nerf_volume_march(nerf_ctx* c, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* rays_orig,
                      const float* rays_dirs, int64_t N, int32_t n_steps, float t_min, float* rgb, float* depth, float* opacity,
                      int mem) {
    return volume_march(c, {false, 0}, volume, n, lo3, hi3, rays_orig, rays_dirs, N, n_steps, t_min, rgb, depth, opacity, mem);
}

int nerf_volume_render_image(nerf_ctx* c, const float* volume, int32_t n, const float* lo3, const float* hi3, const float* c2w,
                             float fov, int32_t H, int32_t W, int64_t ray_begin, int64_t ray_count, int32_t n_steps, float t_min,
                             float* rgb, float* depth, float* opacity, int mem) {
    return volume_render_image(c, {false, 0}, volume, n, lo3, hi3, c2w, fov, H, W, ray_begin, ray_count, n_steps, t_min, rgb, depth,
                               opacity, mem);
}

int nerf_sh_volume_sample(nerf_ctx* c, const float* volume, int32_t n, int32_t degree, const float* lo3, const float* hi3,
                          const float* points, const float* dirs, int64_t M, float* out, int mem) {
    return volume_sample(c, {true, degree}, volume, n, lo3, hi3, points, dirs, M, out, mem);
}

int nerf_sh_volume_march(nerf_ctx* c, const float* volume, int32_t n, int32_t degree, const float* lo3, const float* hi3,
                         const float* rays_orig, const float* rays_dirs, int64_t N, int32_t n_steps, float t_min, float* rgb,
                         float* depth, float* opacity, int mem) {
    return volume_march(c, {true, degree}, volume, n, lo3, hi3, rays_orig, rays_dirs, N, n_steps, t_min, rgb, depth, opacity, mem);
}

int nerf_sh_volume_render_image(nerf_ctx* c, const float* volume, int32_t n, int32_t degree, const float* lo3, const float* hi3,
                                const float* c2w, float fov, int32_t H, int32_t W, int64_t ray_begin, int64_t ray_count,
                                int32_t n_steps, float t_min, float* rgb, float* depth, float* opacity, int mem) {
    return volume_render_image(c, {true, degree}, volume, n, lo3, hi3, c2w, fov, H, W, ray_begin, ray_count, n_steps, t_min, rgb,
                               depth, opacity, mem);
}

}  // extern "C"
