// distortion_kernels.hip -- the distortion loss of mip-NeRF 360 on the compositing weights of one pass, and its gradient.
// For a ray with sorted depths z_0..z_{S-1} and weights w_i (near / far: the ctx's bounds):
//     t_i = (z_i - near) / (far - near),  t_S = 1;   sample i owns [t_i, t_{i+1}]: m_i its midpoint, d_i its length
//     L_ray = sum_i sum_j w_i w_j |m_i - m_j|  +  (1/3) sum_i w_i^2 d_i
// The m_i are sorted, so with the inclusive prefix sums P_i = sum_{j<=i} w_j, Q_i = sum_{j<=i} w_j m_j, W = P_{S-1}, Qt = Q_{S-1}:
//     A_i     = sum_j w_j |m_i - m_j| = (m_i P_{i-1} - Q_{i-1}) + ((Qt - Q_i) - m_i (W - P_i))
//     L_ray   = sum_i w_i A_i + (1/3) sum_i w_i^2 d_i
//     dL/dw_i = 2 A_i + (2/3) w_i d_i
//     dL/dm_i = 2 w_i (P_{i-1} - (W - P_i)),   dL/dd_i = w_i^2 / 3
//     dL/dt_i = dL/dm_i / 2 - dL/dd_i + dL/dm_{i-1} / 2 + dL/dd_{i-1}        (index -1: absent; t_S is a constant)
//     dL/dz_i = dL/dt_i / (far - near)
// (equal midpoints are ordered by index).  ONE RAY PER WAVEFRONT, four rays per block, the ray walked in 64-sample chunks like
// the compositing kernels (aux_kernels.hip::composite_kernel, train_kernels.hip::composite_bwd_kernel): coalesced row reads,
// no LDS, any S.  Two sweeps over the ray: the first closes the two scans (W, Qt), the second repeats them -- the same
// operations on the same values, hence the same bits -- and writes the outputs.  A chunk's scan is six shuffle steps
// (Kogge-Stone over the 64 lanes) on top of the running totals of the chunks before it.  No atomics anywhere: the same inputs
// give the same bits on every run and for every batching of the rays.
#include "train_kernels.h"

namespace nerf {

namespace {

struct DistChunk { float w, m, d, P, Q; };     // one lane's sample of a chunk; P, Q: inclusive, over the whole ray so far

// samples s0 .. s0 + 63 of a ray (wr, zr: its rows); lanes past the ray's end carry w = 0 and change no sum
__device__ __forceinline__ DistChunk dist_chunk(const float* __restrict__ wr, const float* __restrict__ zr, int S, int s0,
                                                int lane, float near_b, float range, float carryP, float carryQ) {
    const int s = s0 + lane;
    const bool in = s < S;
    DistChunk c;
    c.w = in ? wr[s] : 0.f;
    const float t0 = in ? (zr[s] - near_b) / range : 1.0f;
    const float t1 = s + 1 < S ? (zr[s + 1] - near_b) / range : 1.0f;
    c.m = (t0 + t1) * 0.5f;
    c.d = t1 - t0;
    float p = c.w, q = c.w * c.m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float pu = __shfl_up(p, o), qu = __shfl_up(q, o);      // (unconditional: every lane takes part in a shuffle)
        if (lane >= o) { p += pu; q += qu; }
    }
    c.P = carryP + p;
    c.Q = carryQ + q;
    return c;
}

}  // namespace

// weights, z (N, S).  st (nullable): gradients are multiplied by st->scale, the loss scale of the mixed_float16 policy, read on
// the device; factor: lambda / N in the trainer, 1 for the bare operator.  loss_per_ray (N): the UNSCALED L_ray.  d_w, d_z
// (N, S): factor * scale * dL/dw, dL/dz -- stored, or added to what is there (add_w, add_z).  Any output may be null.
__global__ __launch_bounds__(256) void distortion_kernel(const float* __restrict__ weights, const float* __restrict__ z,
                                                         long long N, int S, float near_b, float range,
                                                         const OptState* __restrict__ st, float factor,
                                                         float* __restrict__ loss_per_ray, float* __restrict__ d_w, int add_w,
                                                         float* __restrict__ d_z, int add_z) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= N) return;                                        // uniform per wavefront
    const float* wr = weights + r * S;
    const float* zr = z + r * S;
    const float g = st ? factor * st->scale : factor;
    // first sweep: the totals
    float W = 0.f, Qt = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const DistChunk c = dist_chunk(wr, zr, S, s0, lane, near_b, range, W, Qt);
        W = __shfl(c.P, 63);
        Qt = __shfl(c.Q, 63);
    }
    // second sweep: the same scans again, and everything that needs the totals
    float cP = 0.f, cQ = 0.f;          // totals of the chunks before this one
    float dm_far = 0.f, dd_far = 0.f;  // dL/dm, dL/dd of the last sample of the chunk before this one
    float acc = 0.f;
    for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool in = s < S;
        const DistChunk c = dist_chunk(wr, zr, S, s0, lane, near_b, range, cP, cQ);
        const float Pl = __shfl_up(c.P, 1), Ql = __shfl_up(c.Q, 1);
        const float Pe = lane == 0 ? cP : Pl, Qe = lane == 0 ? cQ : Ql;       // P_{i-1}, Q_{i-1}
        const float A = (c.m * Pe - Qe) + ((Qt - c.Q) - c.m * (W - c.P));
        acc += c.w * A + c.w * c.w * c.d / 3.0f;
        const float dm = 2.0f * c.w * (Pe - (W - c.P));
        const float dd = c.w * c.w / 3.0f;
        const float dml = __shfl_up(dm, 1), ddl = __shfl_up(dd, 1);
        const float dm_prev = lane == 0 ? dm_far : dml, dd_prev = lane == 0 ? dd_far : ddl;
        if (in) {
            const long long i = r * S + s;
            if (d_w) {
                const float v = g * (2.0f * A + 2.0f * c.w * c.d / 3.0f);
                d_w[i] = add_w ? d_w[i] + v : v;
            }
            if (d_z) {
                const float dt = 0.5f * dm - dd + 0.5f * dm_prev + dd_prev;
                const float v = g * (dt / range);
                d_z[i] = add_z ? d_z[i] + v : v;
            }
        }
        cP = __shfl(c.P, 63); cQ = __shfl(c.Q, 63);
        dm_far = __shfl(dm, 63); dd_far = __shfl(dd, 63);
    }
    if (loss_per_ray) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) loss_per_ray[r] = acc;
    }
}

void launch_distortion(const float* weights, const float* z, long long N, int S, float near_b, float far_b, const OptState* st,
                       float factor, float* loss_per_ray, float* d_w, bool add_w, float* d_z, bool add_z, hipStream_t s) {
    if (N <= 0 || !(loss_per_ray || d_w || d_z)) return;
    hipLaunchKernelGGL(distortion_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, s, weights, z, N, S, near_b,
                       far_b - near_b, st, factor, loss_per_ray, d_w, add_w ? 1 : 0, d_z, add_z ? 1 : 0);
}

// The batch mean of the per-ray losses, one workgroup and a fixed reduction order (as mse_kernel), added to the running sum
// of its pass: acc[which] += mean; acc[2] counts the gradient computations that ran under the regulariser (count_step: once
// per computation, whichever passes it covers).
__global__ __launch_bounds__(1024) void distortion_mean_kernel(const float* __restrict__ loss_per_ray, long long N, int which,
                                                               int count_step, double* __restrict__ acc) {
    __shared__ float red[1024];
    float s = 0.f;
    for (long long i = threadIdx.x; i < N; i += 1024) s += loss_per_ray[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 512; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        acc[which] += (double)(red[0] / (float)N);
        if (count_step) acc[2] += 1.0;
    }
}

void launch_distortion_mean(const float* loss_per_ray, long long N, int which, bool count_step, double* acc, hipStream_t s) {
    if (N <= 0) return;
    hipLaunchKernelGGL(distortion_mean_kernel, dim3(1), dim3(1024), 0, s, loss_per_ray, N, which, count_step ? 1 : 0, acc);
}

}  // namespace nerf
