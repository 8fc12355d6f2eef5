// sampling_device.h -- the arithmetic of the per-ray stage (stratified depths, inverse-CDF sampler, compositing), each
// formula stated once for the forward kernels (aux_kernels.hip) and the backward kernels that must recompute the forward's
// bits (train_kernels.hip).  __device__ __forceinline__ functions only: device functions do not cross translation units in
// this build.  Every float32 operation is rounded on its own (explicit __f*_rn, or plain operators under -ffp-contract=off);
// sums and cumulative sums run left to right along the sample axis (oracle/nerf_oracle.py's canonical order).
#pragma once
#include "nerf_device.h"

namespace nerf {

// ------------------------------------------------------------------------------------------------
// Stratified depths.  The four constants of a depth range [near, far] --
//   linear:  c0 = start, c1 = stop, c2 = delta = span / (S - 1) (0 for S == 1), c3 = span
//   lindisp: c0 = near, c1 = the float below far, c2 = 1 / near, c3 = 1 / far - 1 / near      (near > 0)
// -- come from the host for the context's (near, far) (aux_kernels.hip: depth_consts_host, in double, rounded once) and from
// depth_consts_of_interval for a ray that a scene box or an occupancy grid narrows to its own (a, b), in float32.
// ------------------------------------------------------------------------------------------------
struct DepthConsts { float c0, c1, c2, c3; };

template <bool LINDISP>
__device__ __forceinline__ DepthConsts depth_consts_of_interval(float a, float b, int S) {
    DepthConsts k;
    k.c0 = a;
    if constexpr (LINDISP) {
        k.c1 = __int_as_float(__float_as_int(b) - 1);           // b > a > 0
        k.c2 = __fdiv_rn(1.0f, a);
        k.c3 = __fsub_rn(__fdiv_rn(1.0f, b), k.c2);
    } else {
        k.c1 = b;
        k.c3 = __fsub_rn(b, a);                                 // the last stratum may pass b by span / S
        k.c2 = S > 1 ? __fdiv_rn(k.c3, (float)(S - 1)) : 0.f;
    }
    return k;
}

// Depth s of S with the draw u in [0, 1).
//   linear:  linspace(start, stop, S)[s] + (u * span) / S; tf.linspace: first = start, last = stop exactly, interior =
//            start + delta * s
//   lindisp: the strata are uniform in 1/z.  t = (s + u) / S,  z = 1 / (inv_near + dinv t).  s + u can round up to s + 1
//            (u = 1 - 2^-24): it is held at the largest float below, so t stays inside its stratum and t < 1; the result is
//            held in [near, far), which the roundings of the last stratum could otherwise touch.
template <bool LINDISP>
__device__ __forceinline__ float stratified_depth(const DepthConsts& k, int s, int S, float u) {
    if constexpr (LINDISP) {
        const float top = (float)(s + 1);
        float v = __fadd_rn((float)s, u);
        if (v >= top) v = __int_as_float(__float_as_int(top) - 1);
        const float t = __fdiv_rn(v, (float)S);
        const float zz = __fdiv_rn(1.0f, __fadd_rn(k.c2, __fmul_rn(k.c3, t)));
        return fminf(fmaxf(zz, k.c0), k.c1);
    } else {
        float lin = __fadd_rn(k.c0, __fmul_rn(k.c2, (float)s));
        if (s == 0) lin = k.c0;
        if (s == S - 1 && S > 1) lin = k.c1;
        return __fadd_rn(lin, __fdiv_rn(__fmul_rn(u, k.c3), (float)S));
    }
}

// ------------------------------------------------------------------------------------------------
// Inverse-CDF sampler (get_z_vals_from_prob_dist_func, src/UtilsCV.py:502-539), one ray per wavefront.
// ------------------------------------------------------------------------------------------------
// #{i < n : arr[i] < v} and #{i < n : arr[i] <= v} of an increasing array: searchsorted left / right
__device__ __forceinline__ int count_below(const float* arr, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (arr[mid] < v) lo = mid + 1; else hi = mid; }
    return lo;
}

__device__ __forceinline__ int count_not_above(const float* arr, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (arr[mid] <= v) lo = mid + 1; else hi = mid; }
    return lo;
}

// Stable rank of v = arr[k] among the n4 (a multiple of 4; padding = +inf) entries of a 16-byte-aligned array: ties broken
// by index, so the ranks are a permutation.  Every lane sweeps the array as float4 broadcasts.
__device__ __forceinline__ int stable_rank(const float* arr, int n4, float v, int k) {
    int rank = 0;
    for (int i = 0; i < n4; i += 4) {
        const float4 o = *reinterpret_cast<const float4*>(arr + i);
        rank += (o.x < v || (o.x == v && i + 0 < k)) ? 1 : 0;
        rank += (o.y < v || (o.y == v && i + 1 < k)) ? 1 : 0;
        rank += (o.z < v || (o.z == v && i + 2 < k)) ? 1 : 0;
        rank += (o.w < v || (o.w == v && i + 3 < k)) ? 1 : 0;
    }
    return rank;
}

// The ray's coarse row into the wave's LDS: zc[s] = zr[s], wv[s] = wr[s] (wv nullable), cdf[s] = the canonical
// left-to-right cumsum of w / (sum + 1e-7), sum itself left to right.  -> sum + 1e-7, in every lane.
// The order is sequential by definition, but only the additions are: up to 64 * kCdfChunks samples every lane keeps its
// samples in registers, the running value is formed redundantly in all lanes from v_readlane broadcasts (no LDS round
// trip, no single-lane loop) and the divisions run 64 wide; longer rays fall back to a one-lane loop over LDS -- the same
// additions and divisions in the same order, so the same bits.  Ends with the wave's fence: the arrays may be read on return.
constexpr int kCdfChunks = 4;

__device__ __forceinline__ float ray_cdf(const float* __restrict__ wr, const float* __restrict__ zr, int S, int lane,
                                         float* cdf, float* zc, float* wv) {
    float den = 0.f;
    if (S <= 64 * kCdfChunks) {
        float wreg[kCdfChunks], creg[kCdfChunks];
#pragma unroll
        for (int c = 0; c < kCdfChunks; ++c) {
            const int s = lane + 64 * c;
            wreg[c] = s < S ? wr[s] : 0.f;
            if (s < S) { zc[s] = zr[s]; if (wv) wv[s] = wreg[c]; }
        }
        float sum = 0.f;
#pragma unroll
        for (int c = 0; c < kCdfChunks; ++c) {
            const int n = min(64, S - 64 * c);
            for (int i = 0; i < n; ++i) sum = __fadd_rn(sum, __shfl(wreg[c], i));
        }
        den = __fadd_rn(sum, 1e-7f);
        float acc = 0.f;
#pragma unroll
        for (int c = 0; c < kCdfChunks; ++c) {
            const float pdf = __fdiv_rn(wreg[c], den);
            const int n = min(64, S - 64 * c);
            creg[c] = 0.f;
            for (int i = 0; i < n; ++i) {
                acc = __fadd_rn(acc, __shfl(pdf, i));
                if (lane == i) creg[c] = acc;
            }
        }
#pragma unroll
        for (int c = 0; c < kCdfChunks; ++c) {
            const int s = lane + 64 * c;
            if (s < S) cdf[s] = creg[c];
        }
    } else {
        for (int s = lane; s < S; s += 64) {
            const float w = wr[s];
            cdf[s] = w; zc[s] = zr[s];
            if (wv) wv[s] = w;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (lane == 0) {
            float sum = 0.f;
            for (int s = 0; s < S; ++s) sum = __fadd_rn(sum, cdf[s]);
            den = __fadd_rn(sum, 1e-7f);
            float acc = 0.f;
            for (int s = 0; s < S; ++s) {
                acc = __fadd_rn(acc, __fdiv_rn(cdf[s], den));
                cdf[s] = acc;
            }
        }
        den = __shfl(den, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    return den;
}

// One fine draw u against the ray's cdf and coarse depths zc (S >= 2 of each): the bin by searchsorted(cdf, u, 'left') --
// count_below, i.e. the search on "cdf[mid] < uu" -- clipped to [0, S - 1] on either side, a 1e-5 floor under the bin's
// probability, and the lerp between the bin's midpoints.  z is the draw; the rest is what the backward differentiates:
// z = z_lo + t * span, t = (u - cdf[b]) / den, den = max(cdf[t_bin] - cdf[b], 1e-5).  A forward that reads .z alone pays
// for nothing else.
struct CdfDraw {
    float z, span, t, den;
    int b, t_bin;
    bool clamped;        // den is the 1e-5 floor: no gradient reaches the cdf through it
};

__device__ __forceinline__ CdfDraw inverse_cdf_draw(const float* cdf, const float* zc, int S, float u) {
    CdfDraw d;
    const int idx = count_below(cdf, S, u);      // first i with cdf[i] >= u, in [0, S]
    d.b = max(0, idx - 1);
    d.t_bin = min(S - 1, idx);
    const float c_lo = cdf[d.b], c_hi = cdf[d.t_bin];
    const int bz = min(max(d.b, 0), S - 2), tz = min(max(d.t_bin, 0), S - 2);
    const float z_lo = __fmul_rn(0.5f, __fadd_rn(zc[bz + 1], zc[bz]));
    const float z_hi = __fmul_rn(0.5f, __fadd_rn(zc[tz + 1], zc[tz]));
    d.den = __fsub_rn(c_hi, c_lo);
    d.clamped = d.den < 1e-5f;
    d.den = d.clamped ? 1e-5f : d.den;
    d.t = __fdiv_rn(__fsub_rn(u, c_lo), d.den);
    d.span = __fsub_rn(z_hi, z_lo);
    d.z = __fadd_rn(z_lo, __fmul_rn(d.t, d.span));
    return d;
}

// ------------------------------------------------------------------------------------------------
// Compositing (ray_marching, src/UtilsNeuralRadianceField.py:88-115): what sample s of an S-sample ray contributes, from its
// raw row o = (r, g, b, sigma) and the depths zr[s], zr[s + 1].  The last interval is 1e9.  e = exp(-sigma delta) is the
// 1 - alpha of the formulas; alpha = fl(1 - e).  A lane past the ray's end (s >= S) gets alpha = 0, e = 1.
// ------------------------------------------------------------------------------------------------
struct CompositeTerms { float delta, sigma, e, alpha, r0, r1, r2; };

// a raw colour column -> the colour: the one sigmoid of the compositing, the vertex colours and the radiance volume's texels
__device__ __forceinline__ float raw_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

__device__ __forceinline__ CompositeTerms composite_terms(const float4 o, const float* __restrict__ zr, int s, int S) {
    CompositeTerms c;
    c.delta = s + 1 < S ? zr[s + 1] - zr[s] : 1e9f;
    c.sigma = fmaxf(o.w, 0.f);
    c.e = s < S ? expf(-(c.sigma * c.delta)) : 1.0f;
    c.alpha = 1.0f - c.e;
    c.r0 = raw_sigmoid(o.x);
    c.r1 = raw_sigmoid(o.y);
    c.r2 = raw_sigmoid(o.z);
    return c;
}

}  // namespace nerf
