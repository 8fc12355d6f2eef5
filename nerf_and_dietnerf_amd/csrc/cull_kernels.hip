// cull_kernels.hip -- sample culling under an occupancy grid (include/nerf_mi355.h: nerf_ctx_set_sample_culling has the
// rule): the samples of a render pass that lie in empty cells of the grid never reach the network.  sample_kept decides per
// sample, sample_keep_kernel packs the verdicts into a bit mask, mesh_kernels.hip's scan turns the mask into a slot per kept
// sample and the row count M, sample_gather_kernel writes the kept samples' points as the M rows of a point-mode (mode 1)
// network pass, and raw_expand_kernel spreads the M raw rows back over all N * S samples with zeros for the culled ones.
//
// The trainer under nerf_ctx_set_train_sample_culling (train_api.hip) uses the same kernels for its forward half; its backward
// half adds graw_gather_kernel (the kept rows of dL/d(raw), padded to whole 128-row tiles with zero rows) and
// pe_bwd_compact_kernel (train_kernels.hip's pe_bwd_kernel reading the encoding gradient of sample t at its compact row).
//
// Canonical like the mesh: no atomics, the rows are in ascending sample index.  The fused MLP kernels are not touched: they
// take M by value, so the host reads it (nerf_api.hip: culled_mlp).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "frag_layout.h"
#include "nerf_device.h"
#include "nerf_kernels.h"
#include "train_kernels.h"

namespace nerf {
namespace {

constexpr int kBs = 256;

struct CullArgs {
    float lo[3], hi[3], cell[3];   // cell_a = (hi_a - lo_a) / R, float32
    const uint32_t* bits;          // R^3 / 32 words, cell (ix, iy, iz) = bit ix + R (iy + R iz)
    int R;
};

CullArgs cull_args(const SceneBox& box, const uint32_t* bits, int R) {
    CullArgs g;
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = box.lo[a]; g.hi[a] = box.hi[a];
        g.cell[a] = (box.hi[a] - box.lo[a]) / (float)R;
    }
    g.bits = bits; g.R = R;
    return g;
}

unsigned blocks_for(long long items) { return (unsigned)((items + kBs - 1) / kBs); }

// The verdict of one sample: float32, every operation rounded on its own, comparisons instead of fminf / fmaxf.
//   1. p_a = o_a + d_a z, multiply then add: the point the MLP kernels form in mode 0, bit for bit
//   2. inside = lo_a <= p_a <= hi_a on all three axes (a NaN compares false: not inside)
//   3. i_a = clamp(floor((p_a - lo_a) / cell_a), 0, R - 1), grid_cell_index (nerf_device.h), which ray_grid_interval calls too:
//      the hi face belongs to cell R - 1, an interior cell face to the upper cell
//   4. culled iff inside and the cell's bit is 0.  A sample outside the box is kept: the grid knows nothing there.
// -> kept.  p: the point of step 1.
__device__ __forceinline__ bool sample_kept(const CullArgs& g, const float4 o, const float4 d, float z, float p[3]) {
    const float oo[3] = {o.x, o.y, o.z}, dd[3] = {d.x, d.y, d.z};
    const int R = g.R;
    bool inside = true;
    int idx[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        p[ax] = __fadd_rn(oo[ax], __fmul_rn(dd[ax], z));
        if (!(g.lo[ax] <= p[ax] && p[ax] <= g.hi[ax])) inside = false;
        idx[ax] = grid_cell_index(p[ax], g.lo[ax], g.cell[ax], R);    // NaN -> 0: the index is in [0, R) whatever p is
    }
    if (!inside) return true;
    const int bit = idx[0] + R * (idx[1] + R * idx[2]);           // < R^3 <= 2^24
    return ((g.bits[bit >> 5] >> (bit & 31)) & 1u) != 0;
}

// One thread per sample; a wave's 64 verdicts are one ballot, stored by its first lane.  Tail lanes vote 0, so the mask's
// last word is whole.  mask: ceil(total / 64) words (nullable); verdict: (total,) int32 1 kept / 0 culled (nullable).
__global__ __launch_bounds__(kBs) void sample_keep_kernel(const CullArgs g, const float* __restrict__ orig,
                                                          const float* __restrict__ dirs, const float* __restrict__ z,
                                                          long long total, int S, unsigned long long* __restrict__ mask,
                                                          int* __restrict__ verdict) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    bool keep = false;
    if (t < total) {
        const long long r = t / S;
        float p[3];
        keep = sample_kept(g, reinterpret_cast<const float4*>(orig)[r], reinterpret_cast<const float4*>(dirs)[r], z[t], p);
        if (verdict) verdict[t] = keep ? 1 : 0;
    }
    const unsigned long long m = __ballot(keep);
    if (mask && (threadIdx.x & 63) == 0 && t < total) mask[t >> 6] = m;
}

// slot of kept sample t among the kept samples: the scan's offset of its mask byte + the kept samples before it in the byte
__device__ __forceinline__ bool sample_slot(const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first, long long t,
                                            size_t* slot) {
    const unsigned byte = mask[t >> 3], k = (unsigned)(t & 7);
    if (!((byte >> k) & 1u)) return false;
    *slot = (size_t)first[t >> 3] + __popc(byte & ((1u << k) - 1u));
    return true;
}

// One thread per sample: a kept sample writes its point (step 1's operations) and its ray's direction to its slot.
__global__ __launch_bounds__(kBs) void sample_gather_kernel(const float* __restrict__ orig, const float* __restrict__ dirs,
                                                            const float* __restrict__ z, long long total, int S,
                                                            const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                            float* __restrict__ xyz, float* __restrict__ view) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t >= total) return;
    size_t slot;
    if (!sample_slot(mask, first, t, &slot)) return;
    const long long r = t / S;
    const float4 o = reinterpret_cast<const float4*>(orig)[r], d = reinterpret_cast<const float4*>(dirs)[r];
    const float zz = z[t];
    xyz[3 * slot + 0] = __fadd_rn(o.x, __fmul_rn(d.x, zz));
    xyz[3 * slot + 1] = __fadd_rn(o.y, __fmul_rn(d.y, zz));
    xyz[3 * slot + 2] = __fadd_rn(o.z, __fmul_rn(d.z, zz));
    if (view) { view[3 * slot + 0] = d.x; view[3 * slot + 1] = d.y; view[3 * slot + 2] = d.z; }
}

// One thread per sample: the full raw buffer from the compact rows, zeros for a culled sample.  SIGMA: (total,) sigma from
// (M,) sigma (the sigma-only coarse pass); otherwise (total, 4) from (M, 4).
template <bool SIGMA>
__global__ __launch_bounds__(kBs) void raw_expand_kernel(const float* __restrict__ compact, long long total,
                                                         const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                         float* __restrict__ raw) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t >= total) return;
    size_t slot;
    const bool kept = sample_slot(mask, first, t, &slot);
    if constexpr (SIGMA) raw[t] = kept ? compact[slot] : 0.f;
    else reinterpret_cast<float4*>(raw)[t] = kept ? reinterpret_cast<const float4*>(compact)[slot] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// The kept rows of Graw (total, 4) as the compact (Mp, 4) buffer the backward passes read; its padding rows M .. Mp are zero.
// One thread per sample, then one per padding row.
__global__ __launch_bounds__(kBs) void graw_gather_kernel(const float* __restrict__ graw, long long total, long long M,
                                                          long long Mp, const uint8_t* __restrict__ mask,
                                                          const uint32_t* __restrict__ first, float* __restrict__ compact) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t < total) {
        size_t slot;
        if (sample_slot(mask, first, t, &slot)) reinterpret_cast<float4*>(compact)[slot] = reinterpret_cast<const float4*>(graw)[t];
    } else if (t - total < Mp - M) {
        reinterpret_cast<float4*>(compact)[M + (t - total)] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// pe_bwd_kernel (train_kernels.hip) for a culled pass: one thread per SAMPLE; a kept sample reads its encoding gradient at its
// compact row and adds dL/dp . d to d_z at its own index, a culled one leaves d_z alone.  The arithmetic is that kernel's,
// operation for operation (the build does not contract), so under a full grid (slot == t) d_z comes out bit-identical.
template <int LX>      // octaves of the gradient rows' layout
__global__ __launch_bounds__(kBs) void pe_bwd_compact_kernel(const float* __restrict__ dA0, const float* __restrict__ dA0b,
                                                             const float* __restrict__ o, const float* __restrict__ d,
                                                             const float* __restrict__ z, long long total, int S,
                                                             const uint8_t* __restrict__ mask, const uint32_t* __restrict__ first,
                                                             float* __restrict__ d_z, int frag) {
    const long long t = (long long)blockIdx.x * kBs + threadIdx.x;
    if (t >= total) return;
    size_t slot;
    if (!sample_slot(mask, first, t, &slot)) return;
    const long long m = (long long)slot;
    const long long r = t / S;
    const float zz = z[t];
    const float kPi = 3.1415927410125732f;
    const float4 oo = reinterpret_cast<const float4*>(o)[r], dd = reinterpret_cast<const float4*>(d)[r];
    const float p[3] = {__fadd_rn(oo.x, __fmul_rn(dd.x, zz)), __fadd_rn(oo.y, __fmul_rn(dd.y, zz)),
                        __fadd_rn(oo.z, __fmul_rn(dd.z, zz))};
    const float dv[3] = {dd.x, dd.y, dd.z};
    constexpr int Q = (3 * (1 + 2 * LX) + 3) / 4;    // float4s covering the 3 + 6 LX encoding columns (rows are 64 floats)
    static_assert(4 * Q <= kXyzPad, "the encoding columns fit a gradient row");
    float g[4 * Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const long long e = frag ? frag_index(m, 4 * q, kXyzPad) : m * kXyzPad + 4 * q;
        float4 v = *reinterpret_cast<const float4*>(dA0 + e);
        if (dA0b) { const float4 w = *reinterpret_cast<const float4*>(dA0b + e); v.x += w.x; v.y += w.y; v.z += w.z; v.w += w.w; }
        g[4 * q] = v.x; g[4 * q + 1] = v.y; g[4 * q + 2] = v.z; g[4 * q + 3] = v.w;
    }
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        constexpr int XC = 1 + 2 * LX;
        float dp = g[c * XC];
#pragma unroll
        for (int k = 0; k < LX; ++k) {
            const float f = kPi * (float)(1 << k);
            const float th = __fmul_rn(p[c], f);
            const float sn = sin_shifted(th, 0), cs = sin_shifted(th, 1);
            dp += (cs * g[c * XC + 1 + 2 * k] - sn * g[c * XC + 2 + 2 * k]) * f;
        }
        acc += dp * dv[c];
    }
    d_z[t] += acc;
}

}  // namespace

void launch_sample_keep(const SceneBox& box, const uint32_t* bits, int R, const float* orig, const float* dirs, const float* z,
                        long long N, int S, uint64_t* mask, int* verdict, hipStream_t stream) {
    const long long total = N * S;
    if (total <= 0) return;
    hipLaunchKernelGGL(sample_keep_kernel, dim3(blocks_for(total)), dim3(kBs), 0, stream, cull_args(box, bits, R), orig, dirs, z,
                       total, S, (unsigned long long*)mask, verdict);
}

void launch_sample_gather(const float* orig, const float* dirs, const float* z, long long N, int S, const uint8_t* mask,
                          const uint32_t* first, float* xyz, float* view, hipStream_t stream) {
    const long long total = N * S;
    if (total <= 0) return;
    hipLaunchKernelGGL(sample_gather_kernel, dim3(blocks_for(total)), dim3(kBs), 0, stream, orig, dirs, z, total, S, mask, first,
                       xyz, view);
}

void launch_raw_expand(const float* compact, long long total, bool sigma_only, const uint8_t* mask, const uint32_t* first,
                       float* raw, hipStream_t stream) {
    if (total <= 0) return;
    if (sigma_only)
        hipLaunchKernelGGL(raw_expand_kernel<true>, dim3(blocks_for(total)), dim3(kBs), 0, stream, compact, total, mask, first, raw);
    else
        hipLaunchKernelGGL(raw_expand_kernel<false>, dim3(blocks_for(total)), dim3(kBs), 0, stream, compact, total, mask, first, raw);
}

void launch_graw_gather(const float* graw, long long total, long long M, long long Mp, const uint8_t* mask, const uint32_t* first,
                        float* compact, hipStream_t stream) {
    const long long items = total + (Mp - M);
    if (items <= 0) return;
    hipLaunchKernelGGL(graw_gather_kernel, dim3(blocks_for(items)), dim3(kBs), 0, stream, graw, total, M, Mp, mask, first, compact);
}

void launch_pe_bwd_compact(const float* dA0, const float* dA0b, const float* o, const float* d, const float* z, long long N, int S,
                           int lx, const uint8_t* mask, const uint32_t* first, float* d_z, hipStream_t s, bool frag) {
    const long long total = N * S;
    if (total <= 0) return;
    const dim3 grid(blocks_for(total)), block(kBs);
    const int fr = frag ? 1 : 0;
#define NERF_PE_BWD_COMPACT(L) \
    case L: hipLaunchKernelGGL(pe_bwd_compact_kernel<L>, grid, block, 0, s, dA0, dA0b, o, d, z, total, S, mask, first, d_z, fr); break;
    switch (lx < 1 ? 1 : lx > 10 ? 10 : lx) {
        NERF_PE_BWD_COMPACT(1) NERF_PE_BWD_COMPACT(2) NERF_PE_BWD_COMPACT(3) NERF_PE_BWD_COMPACT(4) NERF_PE_BWD_COMPACT(5)
        NERF_PE_BWD_COMPACT(6) NERF_PE_BWD_COMPACT(7) NERF_PE_BWD_COMPACT(8) NERF_PE_BWD_COMPACT(9) NERF_PE_BWD_COMPACT(10)
    }
#undef NERF_PE_BWD_COMPACT
}

}  // namespace nerf
