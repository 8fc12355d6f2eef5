// mlp_f16x3.hip -- fused positional-encoding + 11-layer NeRF MLP forward on the fp16 matrix cores with
// fp32-class accuracy: every fp32 operand is split x = hi + lo (two fp16 values, 22 significant bits)
// and each product is formed in three MFMA passes  hi*hi + lo*hi + hi*lo  (the lo*lo term, 2^-22
// relative, is dropped), accumulated in fp32 by v_mfma_f32_32x32x16_f16.
//
// Same reference chain as mlp_fp32.hip (src/UtilsCV.py:584-599,124-143; src/UtilsNRF.py:52-85;
// src/NeRF.py:316-339) and the same kernel skeleton: one wave per SIMD, 32 samples per wave on the
// lane, accumulator registers re-used as the next layer's B operand (here: converted to packed fp16
// hi/lo fragments by the epilogue), weights streamed L2 -> LDS ring by LDS-DMA.  Differences:
//   * k-step = 16 (one 32x32x16 MFMA): fragment element e of lane half h of k-step (t,s) is feature
//     32t + 16s + 8(e>>2) + 4h + (e&3) -- the accumulator-as-operand order of the 32x32 C/D layout;
//   * the weight stream holds an fp16 hi fragment and an fp16 lo fragment per (tile, k-step);
//   * the sigma head (280 -> 1) rides the MFMA as a 5th output tile of layer 8 (its inputs only
//     exist as fp16 hi/lo fragments); the rgb head (128 -> 3) stays on the VALU in fp32.
// The coarse pass of a render reads nothing but the weights, which depend on sigma alone: mlp_f16x3_sig_kernel (SIGONLY)
// ends in BODY_SIG, layer 8's sigma tile by itself (same bias, same 18 k-steps in the same pass order, same register
// as the full kernel's tile 4, so sigma is bit-identical), skips the four rgb tiles and the rgb head, and writes sigma
// alone: raw is then a compact (M,) vector.
// A render that reads rgb only through the pixel sums runs mlp_f16x3_rgbskip_kernel (RGBSKIP, see mlp_f16_body): layer 8 sigma
// first, and a 128-row tile without density skips the rgb tiles (BODY_RGB) and the rgb head.  The non-finite watch then sees a
// skipped tile's sigma but not its rgb, which is not computed.
// Measured accuracy (tests/test_gpu_parity.py): final RGB within 1e-4 of the fp32 oracle.
//
// NERF_BF16 (mlp_bf16x3.hip, mlp_bf16x3_wide.hip) builds the 3-pass render kernels of this source a second time with bf16
// elements (NERF_PRECISION_BF16X3): x = hi + lo with hi = the top 16 bits of the fp32 value (exact in bf16, no conversion)
// and lo = x - hi rounded to bf16, the same three passes on v_mfma_f32_32x32x16_bf16 -- same lane map, k-step, C/D layout,
// fragment order, ring and epilogue schedule; ~16 significant bits per operand and fp32's exponent range (nothing
// saturates at 65504).  Only the view-direction, xyz-only and sigma-only render kernels exist in that build (no
// single-pass, no stash variant); the device-side re-pack of its streams reads the fp16 build's gather tables (same slots).
#include "mlp_f16_frag.h"

#include <math.h>
#include <string.h>

#if defined(NERF_BF16) && NERF_PE_LX == 5
namespace nerf::bf16 {     // the bf16 build (mlp_bf16x3.hip): the 3-pass render kernels with bf16 elements
#elif defined(NERF_BF16)
namespace nerf::bf16::wide {   // ... and its wide-PE build (mlp_bf16x3_wide.hip)
#elif NERF_PE_LX == 5
namespace nerf {
#else
namespace nerf::wide {     // the wide-PE build (mlp_f16x3_wide.hip): same kernels with 10 xyz octaves
#endif

// ---- element format of the 3-pass kernels: fp16, or bf16 under NERF_BF16 ----
#ifdef NERF_BF16
typedef __bf16 e8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
#define NERF_MFMA_E16 __builtin_amdgcn_mfma_f32_32x32x16_bf16
// hi = the top 16 bits (8 significant bits, exact in bf16), lo = y - hi (exact in fp32, |lo| < 2^-7 |y|)
__device__ __forceinline__ void split_e(float y, float& hi_f, float& lo_f) {
    hi_f = __uint_as_float(__float_as_uint(y) & 0xFFFF0000u);
    lo_f = y - hi_f;
}
// two hi parts -> one dword: their upper halves, one v_perm_b32, no conversion
__device__ __forceinline__ uint32_t pack_hi(float a, float b) {
    return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
__device__ __forceinline__ uint32_t pack_lo(float a, float b) {   // RNE; v_cvt_pk_bf16_f32
    const bf2 t = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, t);
}
#else
typedef h8 e8;
#define NERF_MFMA_E16 __builtin_amdgcn_mfma_f32_32x32x16_f16
__device__ __forceinline__ void split_e(float y, float& hi_f, float& lo_f) { split_trunc(y, hi_f, lo_f); }
__device__ __forceinline__ uint32_t pack_hi(float a, float b) { return pack_h2(a, b); }
__device__ __forceinline__ uint32_t pack_lo(float a, float b) { return pack_h2(a, b); }
#endif

#ifdef NERF_STAMPS
__device__ unsigned long long g_stamps_h[16];
#endif

// One dense layer on the fp16 matrix cores, u-outer (one accumulator chain per 32-wide output tile).
// The epilogue of a tile (bias, LeakyReLU, hi/lo split, fp16 pack) is dealt out ONE accumulator
// register per k-step over the NEXT tile's chain -- also across layer boundaries (PENDING: the
// previous layer's last tile is finished during this layer's first tile), so no epilogue is exposed.
//   fragments of the layer input live in xh/xl[16]; outputs of tiles 0..6 go to nh/nl and are copied
//   back as the last tile's chain retires the k-steps that read them; tile 7 lands in xh/xl[14..15].
// FAST = single-pass fp16 mode (NERF_PRECISION_F16: the reference's production mixed_float16 numerics): only the
// hi*hi product is formed and the activations are rounded (RNE) to fp16 between layers; same stream, same schedule.
// Since round 4 its hidden layers use the two-tile render kernel's packed-pair epilogue (NERF_FAST_PACKED_EPI): the fp32
// sum (bias = C-in) is cast to fp16 FIRST, LeakyReLU runs on the pair in fp16 with alpha rounded to fp16 -- where Keras'
// mixed_float16 LeakyReLU rounds; the oracles' emulations round there too (oracle.mlp_forward_fp16(..., "c_in"),
// oracle.train_oracle._LRelu16).  The stash forward of the mixed_float16 trainer: 966 -> 908 us per step.
// STASH = training forward: every activation is also written as fp32 to HBM (st_prev: the previous layer's output rows
// of this lane's sample, for its PENDING tile 7; st_cur: this layer's), four consecutive features per float4 store, in the
// FRAGMENT-MAJOR layout of frag_layout.h::frag_index (a store instruction writes 1 KiB / 512 B of consecutive bytes).
// FAST + STASH (the mixed_float16 policy's forward) writes the stash in fp16 -- the very dwords it packs as the next
// layer's operand, four consecutive features per 8-byte store -- and st_prev / st_cur then point at fp16 rows.
// It also records the LeakyReLU' masks the fused backward (mlp_bwd_f16x3.hip) multiplies by: one bit per activation
// (its SIGN bit: 1 = negative), bit mask_bit(ut, r) (mlp_f16_frag.h) of word ut >> 1 of the lane's 128-bit record =
// accumulator register r of output tile ut, i.e. indexed exactly as the backward's accumulators hold the gradient of
// that activation; one 16-byte store per lane and layer (32 B per sample row instead of re-reading the 1 KB stash row
// for its signs).
// ROT rotates the four accumulators: tile u works in accs[(u + ROT) & 3] and a PENDING tile is looked for in
// accs[(ROT + 3) & 3]; every body but BODY_LAST0 (which follows the 9-tile BODY_HIDSIG) uses ROT = 0.
// PP (ping-pong, the 3-pass render kernels): consecutive layers swap the two fragment sets instead of copying the new
// activations back -- the caller passes (x, n) to one layer and (n, x) to the next, tiles 0..6 land in the other set's
// fragments 0..13 and the PENDING tile 7 in its fragments 14..15, which the following layer reads as its own xh/xl[14..15].
// No fragment is ever copied; every value is computed by the same instructions in the same order.
template <int BODY, bool PENDING, bool FAST, bool STASH = false, int ROT = 0, bool PP = false>
__device__ __forceinline__ void layer_body_h(Pipe& p, uint32_t lane16, uint32_t cb_h, int bias_off_bytes,
                                             float alpha, float* st_prev, float* st_cur, frag4* mk_prev_ptr,
                                             frag4* mk_cur_ptr, frag4& mk_prev, frag4& mk_cur, f32x16 (&accs)[4],
                                             frag4 (&xh)[16], frag4 (&xl)[16], frag4 (&nh)[PP ? 16 : 14], frag4 (&nl)[PP ? 16 : 14],
                                             const frag4 (&peh)[kHStepsPE], const frag4 (&pel)[kHStepsPE], const frag4 (&dh)[2],
                                             const frag4 (&dl)[2], float (&xc)[64], float& sigma_raw) {
    constexpr int NU = BODY == BODY_LAST ? kHTilesLast : BODY == BODY_SIG ? 1 : BODY == BODY_HIDSIG ? 9 : (BODY == BODY_LAST0 || BODY == BODY_RGB) ? 4 : 8;
    constexpr int NSTEP = BODY == BODY_PE ? kHStepsPE : (BODY == BODY_HID || BODY == BODY_HIDSIG || BODY == BODY_LAST0) ? kHStepsHid
                          : BODY == BODY_SKIP ? kHStepsPE + kHStepsHid : kHStepsHid + kHStepsDir;   // BODY_LAST, BODY_SIG, BODY_RGB: [h7, dir]
    constexpr int SIG0 = BODY == BODY_HIDSIG ? 1 : 0;      // tiles before the first hidden tile (the leading sigma tile)
    constexpr int TPS = FAST ? 1 : 2;        // quads (A fragments) per k-step: hi [, lo]
    constexpr int QPU = TPS * NSTEP;
    constexpr int NQ = NU * QPU;
    // A fragments are fetched kPf quads (2 k-steps = 6 MFMAs = 192 cycles) ahead of their MFMAs.  The
    // ds_read is inline asm with a hand-counted s_waitcnt: left to itself hipcc sinks the reads next to
    // their MFMA (register pressure) and every k-step then waits out the LDS latency.  Destinations are
    // AGPRs ("a"): plentiful here, legal as MFMA A operands, and never shuffled by the allocator between
    // the read and its wait.  LDS returns in order, so lgkmcnt(kPf-1) before quad Q's use means "Q has
    // landed" however many younger compiler-issued LDS reads are in flight (they only make it stricter).
#ifndef NERF_KPF
#define NERF_KPF 4
#endif
#ifndef NERF_KPF_FAST
#define NERF_KPF_FAST 8
#endif
    constexpr int kPf = FAST ? NERF_KPF_FAST : NERF_KPF;   // single-pass: a quad is consumed every 32 cycles, look further ahead
#ifndef NERF_STASH_EXTRA_FAST
#define NERF_STASH_EXTRA_FAST 0
#endif
#ifndef NERF_STASH_EXTRA_3P
#define NERF_STASH_EXTRA_3P 0
#endif
    constexpr int kStashExtra = STASH ? (FAST ? NERF_STASH_EXTRA_FAST : NERF_STASH_EXTRA_3P) : 0;
    f32x4 pf[kPf];
    const int ck0 = p.ck;   // chunk of quad 0 of this body; quad Q lives in chunk ck0 + Q/16
    uint32_t rdbase[2];     // LDS address of the ring slot of an even / odd chunk (refreshed as chunks retire)
    rdbase[0] = lane16 + (uint32_t)((ck0 + 0) & (kHRing - 1)) * kHChunkBytes;
    rdbase[1] = lane16 + (uint32_t)((ck0 + 1) & (kHRing - 1)) * kHChunkBytes;
    auto issue_read = [&](auto qc) {
        constexpr int Qa = decltype(qc)::value;
        lds_read_frag_asm<(Qa % kHCQ) * kQuadBytes>(pf[Qa % kPf], rdbase[(Qa / kHCQ) & 1]);
    };
    static_for<0, kPf>([&](auto ic) {
        if constexpr (decltype(ic)::value < NQ) issue_read(ic);
    });

    // Epilogue of accumulator registers r, r+1 (r even) of output tile `ut` of a hidden layer, in three
    // phases that the k-step interleaves with its three MFMAs (each 32-cycle MFMA hides ~4 plain VALU
    // ops or ~2 conversions/moves; clustered they stall the matrix pipe):
    //   A/B: y = LeakyReLU(acc + bias) for r / r+1     C: split hi/lo, pack fp16 pairs, store fragment dword
    auto act = [&](float v) -> float {
        const float av = alpha * v;
        float y;
        asm("v_max_f32 %0, %1, %2" : "=v"(y) : "v"(v), "v"(av));
        return y;
    };
    // bias = initial accumulator (C-in), loaded one tile ahead into the accumulator that tile will use
    auto load_bias = [&](int off_bytes, f32x16& dst) {
        static_for<0, 4>([&](auto gc) {
            constexpr int g = decltype(gc)::value;
            const f32x4 b = lds_read4(cb_h + off_bytes + g * 32);
            dst[4 * g + 0] = b[0]; dst[4 * g + 1] = b[1]; dst[4 * g + 2] = b[2]; dst[4 * g + 3] = b[3];
        });
    };
    float sq0 = 0.f, sq1 = 0.f;      // first half of the float4 being collected for the stash
    (void)sq0; (void)sq1;
    auto stash4 = [&](auto utc, auto rc, float y0, float y1, float* base) {
        // registers r..r+1 of output tile ut = features 32 ut + 8 (r >> 2) + 4 h + (r & 3) .. (+1); h sits in `base`
        constexpr int ut = decltype(utc)::value;
        constexpr int r = decltype(rc)::value;
        if constexpr ((r & 3) == 0) { sq0 = y0; sq1 = y1; }
        else {
            f32x4 v;
            v[0] = sq0; v[1] = sq1; v[2] = y0; v[3] = y1;
#ifndef NERF_DIAG_NO_STASH_STORES   // timing-only diagnostic: everything but the store instruction itself
            stream_store(reinterpret_cast<f32x4*>(base + 32 * (32 * ut + 8 * (r >> 2))), v);
#else
            asm volatile("" :: "v"(v), "v"(base));
#endif
        }
    };
    uint32_t sqh = 0u;               // fp16 stash: the first packed pair of the four features being collected
    (void)sqh;
    auto stash4h = [&](auto utc, auto rc, uint32_t ph, float* base) {
        constexpr int ut = decltype(utc)::value;
        constexpr int r = decltype(rc)::value;
        if constexpr ((r & 3) == 0) sqh = ph;
#ifndef NERF_DIAG_NO_STASH_STORES
        else stream_store(reinterpret_cast<uint2*>(reinterpret_cast<uint16_t*>(base) + 32 * (32 * ut + 8 * (r >> 2))), make_uint2(sqh, ph));
#else
        else asm volatile("" :: "v"(sqh), "v"(ph), "v"(base));
#endif
    };
    auto store_pair = [&](auto utc, auto rc, float y0, float y1, auto dest_sel, auto pend_sel) {
        constexpr int ut = decltype(utc)::value;
        constexpr int r = decltype(rc)::value;
        constexpr int n = 2 * ut + (r >> 3), e = r & 7;
        uint32_t ph, pl = 0u;
        if constexpr (FAST) {
            ph = pack_h2(y0, y1);                                         // round to fp16, no lo part
        } else {
            float h0, l0, h1, l1;
            split_e(y0, h0, l0);
            split_e(y1, h1, l1);
            ph = pack_hi(h0, h1); pl = pack_lo(l0, l1);                   // whole-register writes
            // PP: nothing in this body reads the new fragments, and left to itself hipcc keeps the fp32 values and sinks
            // every split and pack to the end of the layer; pinned here they stay under the k-step they were dealt to
            if constexpr (PP && BODY != BODY_PE) asm volatile("" : "+v"(ph), "+v"(pl));
        }
        if constexpr (STASH) {
            if constexpr (FAST) stash4h(utc, rc, ph, decltype(pend_sel)::value ? st_prev : st_cur);
            else stash4(utc, rc, y0, y1, decltype(pend_sel)::value ? st_prev : st_cur);
            // LeakyReLU' record: the two SIGN bits of the packed pair, shifted in (mask_push, mlp_f16_frag.h) -- two plain
            // VALU ops per pair (two compares, two selects and an or before: the mask alone was a third of this
            // kernel's VALU work beside the single-pass MFMAs)
            if constexpr (decltype(pend_sel)::value) mk_prev[ut >> 1] = mask_push(mk_prev[ut >> 1], ph);
            else mk_cur[ut >> 1] = mask_push(mk_cur[ut >> 1], ph);
        }
        if constexpr (decltype(dest_sel)::value) { xh[n][e >> 1] = ph; if constexpr (!FAST) xl[n][e >> 1] = pl; }
        else { nh[n][e >> 1] = ph; if constexpr (!FAST) nl[n][e >> 1] = pl; }
    };

    // FAST, packed-pair epilogue (NERF_FAST_PACKED_EPI, the two-tile render kernel's: mlp_f16_2t.hip): the accumulator pair is
    // converted FIRST (v_cvt_pk_f16_f32), then alpha and max act on the pair (v_pk_mul_f16, v_pk_max_f16): 1.5 plain vector
    // instructions per value instead of 2.5 (the bias is the accumulator's C-in here)
#ifndef NERF_FAST_PACKED_EPI
#define NERF_FAST_PACKED_EPI 1
#endif
    constexpr bool kPackedEpi = FAST && NERF_FAST_PACKED_EPI != 0;
    const uint32_t alpha2 = pack_h2(alpha, alpha);
    (void)alpha2;
    auto act_pair = [&](float v0, float v1) -> uint32_t {
        const uint32_t pk = pack_h2(v0, v1);
        uint32_t q, y;
        asm("v_pk_mul_f16 %0, %1, %2" : "=v"(q) : "v"(pk), "v"(alpha2));
        asm("v_pk_max_f16 %0, %1, %2" : "=v"(y) : "v"(pk), "v"(q));
        return y;
    };
    auto store_pair_p = [&](auto utc, auto rc, uint32_t ph, auto dest_sel, auto pend_sel) {
        constexpr int ut = decltype(utc)::value;
        constexpr int r = decltype(rc)::value;
        constexpr int n = 2 * ut + (r >> 3), e = r & 7;
        if constexpr (STASH) {
            stash4h(utc, rc, ph, decltype(pend_sel)::value ? st_prev : st_cur);
            if constexpr (decltype(pend_sel)::value) mk_prev[ut >> 1] = mask_push(mk_prev[ut >> 1], ph);
            else mk_cur[ut >> 1] = mask_push(mk_cur[ut >> 1], ph);
        }
        if constexpr (decltype(dest_sel)::value) xh[n][e >> 1] = ph;
        else nh[n][e >> 1] = ph;
    };
    (void)act_pair; (void)store_pair_p;
    float ycarry = 0.f;
    (void)ycarry;
    static_for<0, NU>([&](auto uc) {
        constexpr int u = decltype(uc)::value;
        f32x16& acc = accs[(u + ROT) & 3];
        f32x16& prv = accs[(u + ROT + 3) & 3];
        f32x16& nxt = accs[(u + ROT + 1) & 3];
        if constexpr (u == 0 && !PENDING) load_bias(bias_off_bytes, acc);   // first layer of a tile: exposed once
        static_for<0, NSTEP>([&](auto nc) {
            constexpr int n = decltype(nc)::value;
            f32x4 araw[2];
            static_for<0, TPS>([&](auto tc) {
                constexpr int t = decltype(tc)::value;
                constexpr int Q = u * QPU + TPS * n + t;
                constexpr int left = NQ - Q;
                (void)left;
                constexpr int qc = Q % kHCQ;        // position inside the chunk
                if constexpr (qc == 0 && Q > 0) p.ck += 1;
                if constexpr (qc == kHCQ / 2) {
                    // pieces 1.. go out at quads +2, +4, ...; those that would fall past the body's end go now
                    constexpr int room = (NQ - 1 - Q) / 2;                 // pieces that still find a quad
                    pipe_sync_c<kHCQ, kHRing, (room + 1 < kHCQ / 4 ? room + 1 : kHCQ / 4), kStashExtra>(p);
                }
                if constexpr (qc > kHCQ / 2 && (qc - kHCQ / 2) % 2 == 0) {
                    // was this chunk's sync a tail case (pieces issued out of order)?  then re-establish M0
                    constexpr int Qs = Q - (qc - kHCQ / 2);
                    constexpr bool tail = (NQ - 1 - Qs) / 2 + 1 < kHCQ / 4;
                    pipe_piece_c<(qc - kHCQ / 2) / 2, tail>(p);
                }
                // quad Q has landed once at most the kPf-1 younger fragment reads are outstanding
                lds_wait_frag_asm<(NQ - Q >= kPf ? kPf - 1 : NQ - Q - 1)>(pf[Q % kPf]);
                araw[t] = pf[Q % kPf];
                // chunk ck+1 is complete for every wave once this chunk's sync (quad 8) has passed, so a
                // lookahead of 4 quads never reads ahead of a sync it depends on
                if constexpr (Q + kPf < NQ) {
                    constexpr int Qn = Q + kPf;
                    if constexpr (Qn % kHCQ == 0)   // first read of a new chunk: point its base at the slot
                        rdbase[(Qn / kHCQ) & 1] = lane16 + (uint32_t)((ck0 + Qn / kHCQ) & (kHRing - 1)) * kHChunkBytes;
                    issue_read(std::integral_constant<int, Qn>{});
                }
            });
            const e8 a_hi = __builtin_bit_cast(e8, araw[0]);
            const e8 a_lo = __builtin_bit_cast(e8, araw[FAST ? 0 : 1]);
            (void)a_lo;
            frag4 bh_, bl_;
            if constexpr (BODY == BODY_PE) { bh_ = peh[n]; bl_ = pel[n]; }
            else if constexpr (BODY == BODY_HID || BODY == BODY_HIDSIG || BODY == BODY_LAST0) { bh_ = xh[n]; bl_ = xl[n]; }
            else if constexpr (BODY == BODY_SKIP) {
                if constexpr (n < kHStepsPE) { bh_ = peh[n]; bl_ = pel[n]; }
                else { bh_ = xh[n - kHStepsPE]; bl_ = xl[n - kHStepsPE]; }
            } else {
                if constexpr (n < kHStepsHid) { bh_ = xh[n]; bl_ = xl[n]; }
                else { bh_ = dh[n - kHStepsHid]; bl_ = dl[n - kHStepsHid]; }
            }
            const e8 b_hi = __builtin_bit_cast(e8, bh_), b_lo = __builtin_bit_cast(e8, bl_);
            // Deferred epilogue: within a layer ONE accumulator register of the previous tile per k-step over
            // all 16 steps (fragment dwords are packed on odd steps); the previous LAYER's tile 7 goes a pair per
            // step over steps 0..7 because its fragments are read from step 14 on.
            constexpr bool kPend = (u == 0) && PENDING && n < 8;
            constexpr bool kPrevS = (u > SIG0) && BODY != BODY_PE && NSTEP >= 16 && n < 16;
            constexpr int et = kPend ? 7 : (u > SIG0 ? u - 1 - SIG0 : 0);      // hidden-tile index of the previous tile
            constexpr bool kXc = (BODY == BODY_LAST || BODY == BODY_LAST0 || BODY == BODY_RGB) && kPrevS;
            // the leading sigma tile (row 0 = the raw density, no activation, src/NeRF.py:283) is complete after tile 0
            if constexpr (BODY == BODY_HIDSIG && u == 1 && n == 0) sigma_raw = prv[0];
            if constexpr (!FAST) {
                acc = NERF_MFMA_E16(a_hi, b_lo, acc, 0, 0, 0);
                acc = NERF_MFMA_E16(a_lo, b_hi, acc, 0, 0, 0);
            }
            acc = NERF_MFMA_E16(a_hi, b_hi, acc, 0, 0, 0);
            if constexpr (kPend && kPackedEpi) {
                constexpr int er = 2 * n;
                store_pair_p(std::integral_constant<int, 7>{}, std::integral_constant<int, er>{}, act_pair(prv[er], prv[er + 1]), std::true_type{}, std::true_type{});
            } else if constexpr (kPrevS && !kXc && kPackedEpi) {
                if constexpr ((n & 1) == 1)
                    store_pair_p(std::integral_constant<int, et>{}, std::integral_constant<int, n - 1>{}, act_pair(prv[n - 1], prv[n]), std::false_type{}, std::false_type{});
            } else if constexpr (kPend) {
                constexpr int er = 2 * n;
                float y0, y1;
                if constexpr (PP) {
                    // the PENDING tile is complete before the body starts and hipcc hoists its alpha * acc in front of the
                    // first MFMA; read the pair here, in the k-step that packs it
                    float v0 = prv[er], v1 = prv[er + 1];
                    asm volatile("" : "+v"(v0), "+v"(v1));
                    y0 = act(v0); y1 = act(v1);
                } else {
                    y0 = act(prv[er]); y1 = act(prv[er + 1]);
                }
                store_pair(std::integral_constant<int, 7>{}, std::integral_constant<int, er>{}, y0, y1, std::true_type{}, std::true_type{});
            } else if constexpr (kPrevS) {
                const float y = act(prv[n]);
                if constexpr (kXc) {
                    xc[et * 16 + n] = y;
                    if constexpr (STASH) {      // layer 8's outputs (128 features) go to the stash in fours as well
                        if constexpr ((n & 1) == 0) ycarry = y;
                        else {
                            const uint32_t pp = pack_h2(ycarry, y);
                            if constexpr (FAST) stash4h(std::integral_constant<int, et>{}, std::integral_constant<int, n - 1>{}, pp, st_cur);
                            else stash4(std::integral_constant<int, et>{}, std::integral_constant<int, n - 1>{}, ycarry, y, st_cur);
                            mk_cur[et >> 1] = mask_push(mk_cur[et >> 1], pp);
                        }
                    }
                }
                else if constexpr ((n & 1) == 0) ycarry = y;
                else store_pair(std::integral_constant<int, et>{}, std::integral_constant<int, n - 1>{}, ycarry, y, std::false_type{}, std::false_type{});
            }
            if constexpr (u == 0 && PENDING) {
                if constexpr (STASH && n == 8) { if (mk_prev_ptr) stream_store(mk_prev_ptr, mk_prev); }   // that layer's mask word is complete
                // previous layer's tile 6 sits complete in nh/nl[12..13]; its k-steps are long retired
                if constexpr (!PP && n == 8) { xh[12] = nh[12]; xl[12] = nl[12]; }
                if constexpr (!PP && n == 9) { xh[13] = nh[13]; xl[13] = nl[13]; }
            }
            // preload the bias of the NEXT tile (or of the next layer's tile 0: the layers' biases are
            // contiguous in the constant region) into the accumulator it will use -- free since 2 tiles
            if constexpr (n == (NSTEP >= 12 ? 10 : 0)) {
                if constexpr (u + 1 < NU) load_bias(bias_off_bytes + (u + 1) * 128, nxt);
                else if constexpr (BODY != BODY_LAST && BODY != BODY_LAST0 && BODY != BODY_SIG && BODY != BODY_RGB) load_bias(bias_off_bytes + NU * 128, nxt);
            }
            // layer 0 has only 3 k-steps per tile: its epilogues go in one block per tile
            if constexpr (BODY == BODY_PE && u > 0 && n == 0) {
                static_for<0, 8>([&](auto pc) {
                    constexpr int r = 2 * decltype(pc)::value;
                    if constexpr (kPackedEpi) {
                        const uint32_t ph = act_pair(prv[r], prv[r + 1]);
                        if constexpr (u - 1 <= 5) store_pair_p(std::integral_constant<int, u - 1>{}, std::integral_constant<int, r>{}, ph, std::true_type{}, std::false_type{});
                        else store_pair_p(std::integral_constant<int, u - 1>{}, std::integral_constant<int, r>{}, ph, std::false_type{}, std::false_type{});
                        return;
                    }
                    const float z0 = act(prv[r]), z1 = act(prv[r + 1]);
                    if constexpr (u - 1 <= 5 || PP) store_pair(std::integral_constant<int, u - 1>{}, std::integral_constant<int, r>{}, z0, z1, std::true_type{}, std::false_type{});
                    else store_pair(std::integral_constant<int, u - 1>{}, std::integral_constant<int, r>{}, z0, z1, std::false_type{}, std::false_type{});
                });
            }
            // last tile of an in-place layer: fragment m-1 of x-in died with k-step m-1; tiles 0..5 of
            // the new activations (fragments 0..11) are complete by now
            if constexpr (!PP && (BODY == BODY_HID || BODY == BODY_SKIP || BODY == BODY_HIDSIG) && u == NU - 1) {
                constexpr int m = BODY == BODY_SKIP ? n - kHStepsPE : n;
                if constexpr (m >= 1 && m - 1 < 12) { xh[m - 1] = nh[m - 1]; xl[m - 1] = nl[m - 1]; }
            }
        });
    });
    if constexpr (BODY == BODY_LAST0 || BODY == BODY_RGB) {
        // the last 32 features have no following chain in this body: their activation is exposed once per tile
        f32x16& lastacc = accs[(NU - 1 + ROT) & 3];
#pragma unroll
        for (int r = 0; r < 16; ++r) xc[(NU - 1) * 16 + r] = act(lastacc[r]);
        if constexpr (STASH) {
            static_for<0, 8>([&](auto pc) {
                constexpr int r = 2 * decltype(pc)::value;
                const float y0 = xc[(NU - 1) * 16 + r], y1 = xc[(NU - 1) * 16 + r + 1];
                const uint32_t pp = pack_h2(y0, y1);
                if constexpr (FAST) stash4h(std::integral_constant<int, NU - 1>{}, std::integral_constant<int, r>{}, pp, st_cur);
                else stash4(std::integral_constant<int, NU - 1>{}, std::integral_constant<int, r>{}, y0, y1, st_cur);
                mk_cur[(NU - 1) >> 1] = mask_push(mk_cur[(NU - 1) >> 1], pp);
            });
            if (mk_cur_ptr) stream_store(mk_cur_ptr, mk_cur);      // the 128-wide layer's record is complete
        }
    }
    if constexpr (BODY == BODY_LAST || BODY == BODY_SIG) {
        // sigma row: feature row 0 of tile 4 (BODY_SIG: its only tile) = register 0 of lane half 0; raw, no activation
        // (NeRF.py:336).  Both bodies keep that tile in accs[0].
        static_assert(((NU - 1 + ROT) & 3) == 0, "the sigma tile's accumulator");
        sigma_raw = accs[(NU - 1) & 3][0];
        if constexpr (STASH) { if (mk_cur_ptr) stream_store(mk_cur_ptr, mk_cur); }   // layer 8 (128 features): all four tiles are finished
    }
    if constexpr (NQ % kHCQ != 0 && NQ % kHCQ <= kHCQ / 2) pipe_sync_c<kHCQ, kHRing, 1, kStashExtra>(p);
    p.ck += 1;
}

// fp32 values -> fp16 hi / lo fragments (FAST: hi = the value rounded to fp16, no lo)
template <bool FAST>
__device__ __forceinline__ void split8(const float (&v)[8], frag4& hi, frag4& lo) {
#pragma unroll
    for (int e = 0; e < 8; e += 2) {
        if constexpr (FAST) {
            hi[e >> 1] = pack_h2(v[e], v[e + 1]);
            lo[e >> 1] = 0u;
            continue;
        }
        float h0, l0, h1, l1;
        split_e(v[e], h0, l0);
        split_e(v[e + 1], h1, l1);
        hi[e >> 1] = pack_hi(h0, h1);
        lo[e >> 1] = pack_lo(l0, l1);
    }
}

// The weight ring primed for a tile that starts at chunk p.ck: the cyclic stream rewound to its start, chunks 0 .. R-2 on their
// way into the slots of p.ck .. p.ck + R-2.  The caller waits for chunk 0 (vmcnt((kHCQ / 4) * (kHRing - 2)), then a barrier)
// before the tile's first fragment read.  The kernel's prologue, and the rgb-skipping kernel's fast-forward past a tile's
// rgb chunks.
// The fast-forward calls it with no barrier of its own, which rests on two things.  (1) A wave's pieces write only its own
// share of a slot: bytes [wave_lds, wave_lds + kHCQ / 4 KiB) of every chunk, by Pipe::voff / wave_lds -- so a wave that has
// waited vmcnt(0) on its own pieces may aim new ones at the same slots whatever its neighbours have in flight.  (2) Every
// body ends chunk-aligned with R-1 chunks issued beyond the one it finished (layer_body_h's closing pipe_sync_c), so behind
// BODY_SIG the slots of p.ck .. p.ck + R-2 are exactly the ones the dropped chunks occupy and slot p.ck - 1 is the one the
// next mid-chunk sync refills.  A change to the piece distribution or to the bodies' alignment has to revisit the skip path.
static_assert(4 * (kHCQ / 4) * kQuadBytes == kHChunkBytes, "four waves' shares of kHCQ / 4 pieces make one chunk");
__device__ __forceinline__ void pipe_prime(Pipe& p) {
    p.src_next = 0;
#pragma unroll
    for (int c = 0; c < kHRing - 1; ++c) {
        p.cur_src = p.wbase + (size_t)p.src_next * kHChunkBytes;
        p.cur_dst = kLdsRing + ((p.ck + c) & (kHRing - 1)) * kHChunkBytes + p.wave_lds;
        p.src_next += 1;
#pragma unroll
        for (int j = 0; j < kHCQ / 4; ++j) dma_piece(p.cur_src, p.voff + j * kQuadBytes, p.cur_dst + j * kQuadBytes);
    }
}
__device__ __forceinline__ void pipe_prime_land() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((kHCQ / 4) * (kHRing - 2)) : "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
}

// RGBSKIP (mlp_f16x3_rgbskip_kernel; the fp16 ping-pong build with view directions, as SIGONLY): a render whose caller reads
// no per-sample rgb needs layer 8's rgb half and the rgb head only where a sample has weight, and a sample with raw sigma <= 0
// has alpha = 1 - exp(-0 * delta) = 0 exactly: its rgb reaches the pixel as +0 whatever it is.  The kernel therefore runs
// layer 8 sigma first -- BODY_SIG as the sigma-only kernel has it (sigma is the bits the full kernel gives) -- and the four
// waves then vote: if every row of the 128-row tile is empty (raw sigma <= 0, or past M; a NaN never is), the tile writes
// {0, 0, 0, sigma}, issues no rgb MFMA, fragment read or head, drops the rgb chunks the ring had prefetched and re-primes
// it for the next tile (pipe_prime; the landing wait hides behind that tile's front end).  Otherwise BODY_RGB runs the four
// rgb tiles, each with the chain it has in BODY_LAST (bias as C-in, 16 hidden and 2 direction k-steps, three passes), then
// the head and the store as in the full kernel: rgb bit-identical.  The decision is uniform across the workgroup because the
// waves share the ring.  The non-finite watch counts a non-finite sigma on both paths; the rgb of a skipped tile is not
// computed and so not watched.
template <bool FAST, bool STASH = false, bool XYZ = false, bool SIGONLY = false, bool RGBSKIP = false>
__device__ __forceinline__ void mlp_f16_body(const MlpArgs& a, unsigned long long* skip_count = nullptr) {
    static_assert(!SIGONLY || (!FAST && !STASH && !XYZ), "the sigma-only variant is a render kernel of the 3-pass network");
    static_assert(!RGBSKIP || (!FAST && !STASH && !XYZ && !SIGONLY), "the rgb-skipping variant is a render kernel of the 3-pass network");
    // the fp16 3-pass render kernels with view directions (mlp_f16x3_kernel, mlp_f16x3_sig_kernel) ping-pong their fragment
    // sets across layers (layer_body_h's PP); every other instantiation and build keeps the copy-back schedule
#if defined(NERF_BF16) || NERF_PE_LX != 5
    constexpr bool kPPBuild = false;
#else
    constexpr bool kPPBuild = true;
#endif
    constexpr bool kPP = kPPBuild && !FAST && !STASH && !XYZ;     // (dependent in every build: the untaken calls are discarded)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int j = lane & 31;
    const int h = lane >> 5;
    const uint32_t lane16 = kLdsRing + lane * 16;
    // opaque to the compiler: with the constant visible, hipcc folds kLdsConst (128 KiB, beyond a ds_read's 16-bit offset
    // field) into every constant-block address and keeps one base VGPR per distinct address (see mlp_f16_2t.hip)
    uint32_t cb_h = kLdsConst + h * 16;
    asm volatile("" : "+v"(cb_h));

    const long long ntiles = (a.M + 127) / 128;
    if ((long long)blockIdx.x >= ntiles) return;

    // SIGONLY: layer 7's last tile preloads the next body's bias from kHConstBias8 (the layers' biases are contiguous), and
    // the next body is the sigma tile: its 32-float block (kHConstBiasSig) is copied there instead
    // RGBSKIP: the sigma tile comes first and the rgb tiles after it: [sigma block (32), layer 8's bias (128)] at kHConstBias8
    if constexpr (RGBSKIP) {
        for (int i = tid; i < kHConstFloats / 4; i += 256) {
            int s = i;
            if (i >= kHConstBias8 / 4 && i < (kHConstBias8 + 32) / 4) s = i + (kHConstBiasSig - kHConstBias8) / 4;
            else if (i >= (kHConstBias8 + 32) / 4 && i < (kHConstBiasSig + 32) / 4) s = i - 32 / 4;
            reinterpret_cast<f32x4*>(smem + kLdsConst)[i] = reinterpret_cast<const f32x4*>(a.wconst)[s];
        }
    } else
    for (int i = tid; i < (XYZ ? kXConstFloats : kHConstFloats) / 4; i += 256) {
        const bool sig = SIGONLY && i >= kHConstBias8 / 4 && i < (kHConstBias8 + 32) / 4;
        reinterpret_cast<f32x4*>(smem + kLdsConst)[i] =
            reinterpret_cast<const f32x4*>(a.wconst)[sig ? i + (kHConstBiasSig - kHConstBias8) / 4 : i];
    }

    Pipe p;
    p.ck = 0;
    p.src_next = 0;
    p.n_chunks = XYZ ? (FAST ? kXFStreamChunks : kXStreamChunks) : SIGONLY ? kHStreamChunksSig : RGBSKIP ? kHStreamChunksSkip : (FAST ? kFStreamChunks : kHStreamChunks);
    p.wbase = reinterpret_cast<const char*>(a.wstream);
    p.voff = wave * (kHCQ / 4 * kQuadBytes) + lane * 16;
    p.wave_lds = wave * (kHCQ / 4 * kQuadBytes);
    __syncthreads();
    // pipeline prologue: chunks 0 .. R-2 in flight, chunk 0 landed for everyone
    pipe_prime(p);
    pipe_prime_land();

    frag4 xh[16], xl[16], nh[kPP ? 16 : 14], nl[kPP ? 16 : 14], peh[kHStepsPE], pel[kHStepsPE], dh[2], dl[2];
    f32x16 accs[4];
    float xc[64];
    float sigma_raw = 0.f;

    // phases 0..5 and the tile count 6 as tools/stamps.py names them; RGBSKIP: 7 = the vote, 8 = the skipped tiles' store and
    // fast-forward, 9 = the skipped tiles
    unsigned long long t0 = 0, t1 = 0, acc_t[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    (void)t0; (void)t1; (void)acc_t;
    bool landing = false;      // RGBSKIP: the ring was re-primed behind a skipped tile and chunk 0 has not been waited for
    (void)landing;
    unsigned long long n_tiles = 0, n_skipped = 0;     // RGBSKIP: this workgroup's tiles, for skip_count
    (void)n_tiles; (void)n_skipped;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        STAMP(t0);
        const long long m = tile * 128 + wave * 32 + j;
        const bool valid = m < a.M;
        const long long mm = valid ? m : a.M - 1;
        float px, py, pz, dx, dy, dz;
        if (a.mode == 0) {
            const long long ray = mm / a.S;
            const f32x4 o = *reinterpret_cast<const f32x4*>(a.in_a + ray * 4);
            const f32x4 d = *reinterpret_cast<const f32x4*>(a.in_b + ray * 4);
            const float zz = a.z[mm];
            px = __fadd_rn(o[0], __fmul_rn(d[0], zz));
            py = __fadd_rn(o[1], __fmul_rn(d[1], zz));
            pz = __fadd_rn(o[2], __fmul_rn(d[2], zz));
            dx = d[0]; dy = d[1]; dz = d[2];
        } else {
            px = a.in_a[mm * 3 + 0]; py = a.in_a[mm * 3 + 1]; pz = a.in_a[mm * 3 + 2];
            if constexpr (XYZ) { dx = dy = dz = 0.f; }        // no view directions in this network (may be null)
            else { dx = a.in_b[mm * 3 + 0]; dy = a.in_b[mm * 3 + 1]; dz = a.in_b[mm * 3 + 2]; }
        }
        const float kPi = 3.1415927410125732f;
        // 24 slots per lane half: h=0: sin of the 15 angles, x, y, z; h=1: cos of the 15 angles
        // (wide-PE build: 32 slots per half: sin / cos of the 30 angles, then h=0: x, y; h=1: z, pad -- h_pe_row)
        float pv[8 * kHStepsPE];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = c == 0 ? px : c == 1 ? py : pz;
            if constexpr (FAST) {
                sin_ladder_fp16_modes<kPeLx>(v * kPi, h, &pv[c * kPeLx]);     // angle doubling: single-pass fp16 modes only
            } else {
#pragma unroll
                for (int k = 0; k < kPeLx; ++k) pv[c * kPeLx + k] = sin_shifted(v * (kPi * (float)(1 << k)), h);
            }
        }
        if constexpr (kPeLx == 5) {
            pv[15] = h ? 0.f : px; pv[16] = h ? 0.f : py; pv[17] = h ? 0.f : pz;
#pragma unroll
            for (int i = 18; i < 24; ++i) pv[i] = 0.f;
        } else {
            static_assert(kPeLx == 10, "the wide-PE layout holds exactly 10 octaves");
            pv[30] = h ? pz : px; pv[31] = h ? 0.f : py;
        }
#pragma unroll
        for (int n = 0; n < kHStepsPE; ++n) {
            float t8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) t8[e] = pv[n * 8 + e];
            split8<FAST>(t8, peh[n], pel[n]);
        }
        float dv[16];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = c == 0 ? dx : c == 1 ? dy : dz;
            if constexpr (FAST) {
                sin_ladder_fp16_modes<kLd>(v * kPi, h, &dv[c * kLd]);
            } else {
#pragma unroll
                for (int k = 0; k < kLd; ++k) dv[c * kLd + k] = sin_shifted(v * (kPi * (float)(1 << k)), h);
            }
        }
#pragma unroll
        for (int i = 12; i < 16; ++i) dv[i] = 0.f;
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            float t8[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) t8[e] = dv[n * 8 + e];
            split8<FAST>(t8, dh[n], dl[n]);
        }

        // stash rows of this lane's sample (rows beyond M exist: the buffers are padded to whole 128-row tiles)
        auto st_of = [&](int l) -> float* {
            if constexpr (!STASH) return nullptr;
            else {
                // row offset in elements (st_ld[l] elements per row): fp32 elements, or fp16 ones under FAST (the pointer
                // arithmetic below is in floats, so halve it there)
                // fragment-major rows (frag_layout.h::frag_index): the wave's 32 samples are one block, lane (h, j) owns
                // the 4-element slot h * 32 + j of every 8-feature group; a feature offset c (c % 8 == 0) is 32 c elements
                const long long row0 = a.diag_wrap ? (long long)(blockIdx.x & 63) * 128 + wave * 32 : tile * 128 + wave * 32;
                const long long off = row0 * (long long)a.st_ld[l] + (h * 32 + j) * 4;
                if constexpr (FAST) return reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(a.st_ptr[l]) + off);
                else return a.st_ptr[l] + off;
            }
        };
        auto mk_of = [&](int l) -> frag4* {
            if constexpr (!STASH) return nullptr;
            else return a.mask_ptr[l] ? reinterpret_cast<frag4*>(a.mask_ptr[l]) + (tile * 128 + wave * 32 + j) * 2 + h
                                      : nullptr;      // no record wanted (layer-by-layer backward)
        };
        frag4 mk_prev = {0u, 0u, 0u, 0u}, mk_cur = {0u, 0u, 0u, 0u};
        frag4 *mk_prev_ptr = nullptr, *mk_cur_ptr = mk_of(0);
        float* st_prev = nullptr;
        float* st_cur = st_of(0);
        if constexpr (RGBSKIP) {
            if (landing) { pipe_prime_land(); landing = false; }
        }
        STAMP(t1); acc_t[0] += t1 - t0;
        layer_body_h<BODY_PE, false, FAST, STASH, 0, kPP>(p, lane16, cb_h, (kHConstBias + 0 * 256) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
        STAMP(t0); acc_t[1] += t0 - t1;
        if constexpr (kPP) {
            // layers 1..7 in pairs: an odd layer reads x and writes n, the even one after it (the skip layer among them)
            // reads n and writes x; layer 7 leaves its output in n, where layer 8 reads it
#pragma unroll 1
            for (int l = 1;; l += 2) {
                layer_body_h<BODY_HID, true, FAST, STASH, 0, true>(p, lane16, cb_h, (kHConstBias + l * 256) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
                STAMP(t1); acc_t[2] += t1 - t0; t0 = t1;
                if (l == 7) break;
                if (l == 3) {
                    layer_body_h<BODY_SKIP, true, FAST, STASH, 0, true>(p, lane16, cb_h, (kHConstBias + 4 * 256) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, nh, nl, xh, xl, peh, pel, dh, dl, xc, sigma_raw);
                    STAMP(t1); acc_t[3] += t1 - t0; t0 = t1;
                } else {
                    layer_body_h<BODY_HID, true, FAST, STASH, 0, true>(p, lane16, cb_h, (kHConstBias + (l + 1) * 256) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, nh, nl, xh, xl, peh, pel, dh, dl, xc, sigma_raw);
                    STAMP(t1); acc_t[2] += t1 - t0; t0 = t1;
                }
            }
        } else {
#pragma unroll 1
            for (int l = 1; l <= 7; ++l) {
                st_prev = st_cur;
                st_cur = st_of(l);
                mk_prev_ptr = mk_cur_ptr; mk_cur_ptr = mk_of(l);
                mk_prev = mk_cur; mk_cur = frag4{0u, 0u, 0u, 0u};
                if (l == 4) {
                    layer_body_h<BODY_SKIP, true, FAST, STASH>(p, lane16, cb_h, (kHConstBias + 4 * 256) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
                    STAMP(t1); acc_t[3] += t1 - t0; t0 = t1;
                } else {
                    layer_body_h<BODY_HID, true, FAST, STASH>(p, lane16, cb_h, (kHConstBias + l * 256) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
                    STAMP(t1); acc_t[2] += t1 - t0; t0 = t1;
                }
            }
        }
        if constexpr (XYZ) {
            // (training: stash slot 8 = the extra 256-wide layer, slot 9 = the 128-wide one; each body finishes its
            // predecessor's last tile, so the records rotate as above)
            st_prev = st_cur; st_cur = st_of(8);
            mk_prev_ptr = mk_cur_ptr; mk_cur_ptr = mk_of(8);
            mk_prev = mk_cur; mk_cur = frag4{0u, 0u, 0u, 0u};
            layer_body_h<BODY_HIDSIG, true, FAST, STASH, 0>(p, lane16, cb_h, kXConstBiasSig * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
            st_prev = st_cur; st_cur = st_of(9);
            mk_prev_ptr = mk_cur_ptr; mk_cur_ptr = mk_of(9);
            mk_prev = mk_cur; mk_cur = frag4{0u, 0u, 0u, 0u};
            layer_body_h<BODY_LAST0, true, FAST, STASH, 1>(p, lane16, cb_h, kXConstBias9 * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
        } else if constexpr (SIGONLY) {
            if constexpr (kPP) layer_body_h<BODY_SIG, true, FAST, STASH, 0, true>(p, lane16, cb_h, kHConstBias8 * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, nh, nl, xh, xl, peh, pel, dh, dl, xc, sigma_raw);
            else layer_body_h<BODY_SIG, true, FAST, STASH>(p, lane16, cb_h, kHConstBias8 * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
            STAMP(t1); acc_t[4] += t1 - t0;
        } else if constexpr (RGBSKIP) {
            static_assert(!RGBSKIP || kPP, "the rgb-skipping kernel exists in the ping-pong build only");
            layer_body_h<BODY_SIG, true, FAST, STASH, 0, true>(p, lane16, cb_h, kHConstBias8 * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, nh, nl, xh, xl, peh, pel, dh, dl, xc, sigma_raw);
            STAMP(t1); acc_t[4] += t1 - t0;
            // The vote.  A lane's row is empty if it lies past M or its raw sigma is <= 0 (false for a NaN); sigma sits in
            // lane half 0.  One word per wave, one barrier, and the sum of the four words through readfirstlane: a scalar,
            // the same in every wave.  (The barrier waits for no DMA: the rgb chunks stay in flight under the vote.)
            const bool row_empty = !valid || h != 0 || sigma_raw <= 0.f;
            const uint32_t wave_empty = __builtin_amdgcn_ballot_w64(row_empty) == ~0ull ? 1u : 0u;
            uint32_t vote_w = kLdsVote + wave * 4, vote_r = kLdsVote;
            frag4 votes;
            asm volatile("ds_write_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" ::"v"(vote_w), "v"(wave_empty) : "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(votes) : "v"(vote_r) : "memory");
            const bool skip = __builtin_amdgcn_readfirstlane(votes[0] + votes[1] + votes[2] + votes[3]) == 4u;
            STAMP(t0); acc_t[7] += t0 - t1;
            n_tiles += 1;
            if (skip) {
                n_skipped += 1;
                if (valid && h == 0) {
                    f32x4 out;
                    out[0] = 0.f; out[1] = 0.f; out[2] = 0.f; out[3] = sigma_raw;
                    *reinterpret_cast<f32x4*>(a.raw + m * 4) = out;
                    if (a.nonfinite && !(fabsf(sigma_raw) <= 3.0e38f)) atomicAdd(a.nonfinite, 1ull);
                }
                // Fast-forward to the next tile.  Every wave finished its fragment reads before the vote's barrier, and a
                // wave's DMA pieces only ever write its own share of a slot: once its own outstanding pieces (the rgb
                // chunks, dropped) have landed it may aim new ones at the same slots.  Nobody reads them before the landing
                // barrier behind the next tile's front end.  The last tile of a workgroup primes nothing.
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                if (tile + gridDim.x < ntiles) {
                    pipe_prime(p);
                    landing = true;
                }
                STAMP(t1); acc_t[8] += t1 - t0; acc_t[9] += 1; acc_t[6] += 1;
                continue;
            }
            layer_body_h<BODY_RGB, false, FAST, STASH, 0, true>(p, lane16, cb_h, (kHConstBias8 + 32) * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, nh, nl, xh, xl, peh, pel, dh, dl, xc, sigma_raw);
            STAMP(t1); acc_t[4] += t1 - t0;
        } else {
            st_prev = st_cur;
            st_cur = st_of(8);
            mk_prev_ptr = mk_cur_ptr; mk_cur_ptr = mk_of(8);
            mk_prev = mk_cur; mk_cur = frag4{0u, 0u, 0u, 0u};
            if constexpr (kPP) layer_body_h<BODY_LAST, true, FAST, STASH, 0, true>(p, lane16, cb_h, kHConstBias8 * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, nh, nl, xh, xl, peh, pel, dh, dl, xc, sigma_raw);
            else layer_body_h<BODY_LAST, true, FAST, STASH>(p, lane16, cb_h, kHConstBias8 * 4, a.alpha, st_prev, st_cur, mk_prev_ptr, mk_cur_ptr, mk_prev, mk_cur, accs, xh, xl, nh, nl, peh, pel, dh, dl, xc, sigma_raw);
            STAMP(t1); acc_t[4] += t1 - t0;
        }
        if constexpr (SIGONLY) {
            if (valid && h == 0) {
                a.raw[m] = sigma_raw;
                if (a.nonfinite && !(fabsf(sigma_raw) <= 3.0e38f)) atomicAdd(a.nonfinite, 1ull);
            }
            STAMP(t0); acc_t[5] += t0 - t1; acc_t[6] += 1;
            continue;
        }
        // rgb head (128 -> 3) on the VALU in fp32
        float o0 = 0.f, o1 = 0.f, o2 = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                constexpr int kW = XYZ ? kXConstWrgb : kHConstWrgb;
                const f32x4 w0 = lds_read4(cb_h + (kW + 0 * 128 + t * 32 + g * 8) * 4);
                const f32x4 w1 = lds_read4(cb_h + (kW + 1 * 128 + t * 32 + g * 8) * 4);
                const f32x4 w2 = lds_read4(cb_h + (kW + 2 * 128 + t * 32 + g * 8) * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = xc[t * 16 + g * 4 + e];
                    o0 = fmaf(w0[e], x, o0);
                    o1 = fmaf(w1[e], x, o1);
                    o2 = fmaf(w2[e], x, o2);
                }
            }
        }
        o0 += __shfl_xor(o0, 32);
        o1 += __shfl_xor(o1, 32);
        o2 += __shfl_xor(o2, 32);
        const f32x4 bh = lds_read4(kLdsConst + (XYZ ? kXConstBHead : kHConstBHead) * 4);
        if (valid && h == 0) {
            f32x4 out;
            out[0] = o0 + bh[0]; out[1] = o1 + bh[1]; out[2] = o2 + bh[2]; out[3] = sigma_raw;
            *reinterpret_cast<f32x4*>(a.raw + m * 4) = out;
            // overflow / NaN watch (the f16x3 mode saturates above 65504): count, never hide
            const float chk = out[0] + out[1] + out[2] + out[3];
            if (a.nonfinite && !(fabsf(chk) <= 3.0e38f)) atomicAdd(a.nonfinite, 1ull);
        }
        STAMP(t0); acc_t[5] += t0 - t1; acc_t[6] += 1;
    }
#ifdef NERF_STAMPS
    if (blockIdx.x == 0 && tid == 0)
        for (int i = 0; i < 10; ++i) g_stamps_h[i] = acc_t[i];
#endif
    if constexpr (RGBSKIP) {      // what the host's per-launch gate reads (nerf_ctx.h: RgbSkipGate; the kernel's second argument): two atomics per workgroup
        if (skip_count && tid == 0) {
            atomicAdd(skip_count + 0, n_tiles);
            atomicAdd(skip_count + 1, n_skipped);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#ifdef NERF_BF16
__global__ __launch_bounds__(256, 1) void mlp_bf16x3_kernel(const MlpArgs a) { mlp_f16_body<false>(a); }
__global__ __launch_bounds__(256, 1) void mlp_bf16x3_xyz_kernel(const MlpArgs a) { mlp_f16_body<false, false, true>(a); }
#if NERF_PE_LX == 5
__global__ __launch_bounds__(256, 1) void mlp_bf16x3_sig_kernel(const MlpArgs a) { mlp_f16_body<false, false, false, true>(a); }
#endif

static int bf_grid(const MlpArgs& a, int num_cus) {
    const long long ntiles = (a.M + 127) / 128;
    return (int)(ntiles < (long long)num_cus ? ntiles : (long long)num_cus);
}
void launch_mlp_bf16x3(const MlpArgs& a, int num_cus, hipStream_t stream, bool xyz_only) {
    if (a.M <= 0) return;
    if (xyz_only) hipLaunchKernelGGL(mlp_bf16x3_xyz_kernel, dim3(bf_grid(a, num_cus)), dim3(256), kLdsTotal, stream, a);
    else hipLaunchKernelGGL(mlp_bf16x3_kernel, dim3(bf_grid(a, num_cus)), dim3(256), kLdsTotal, stream, a);
}
#if NERF_PE_LX == 5
void launch_mlp_bf16x3_sig(const MlpArgs& a, int num_cus, hipStream_t stream) {
    if (a.M <= 0) return;
    hipLaunchKernelGGL(mlp_bf16x3_sig_kernel, dim3(bf_grid(a, num_cus)), dim3(256), kLdsTotal, stream, a);
}
#endif
void mlp_bf16x3_set_attributes() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_bf16x3_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_bf16x3_xyz_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
#if NERF_PE_LX == 5
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_bf16x3_sig_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
#endif
}
#else    // !NERF_BF16: the fp16 kernels
__global__ __launch_bounds__(256, 1) void mlp_f16x3_kernel(const MlpArgs a) { mlp_f16_body<false>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16_kernel(const MlpArgs a) { mlp_f16_body<true>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16x3_stash_kernel(const MlpArgs a) { mlp_f16_body<false, true>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16_stash_kernel(const MlpArgs a) { mlp_f16_body<true, true>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16x3_xyz_kernel(const MlpArgs a) { mlp_f16_body<false, false, true>(a); }
#if NERF_PE_LX == 5
__global__ __launch_bounds__(256, 1) void mlp_f16x3_sig_kernel(const MlpArgs a) { mlp_f16_body<false, false, false, true>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16x3_rgbskip_kernel(const MlpArgs a, unsigned long long* skip_count) {
    mlp_f16_body<false, false, false, false, true>(a, skip_count);
}
#endif
__global__ __launch_bounds__(256, 1) void mlp_f16_xyz_kernel(const MlpArgs a) { mlp_f16_body<true, false, true>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16x3_xyz_stash_kernel(const MlpArgs a) { mlp_f16_body<false, true, true>(a); }
__global__ __launch_bounds__(256, 1) void mlp_f16_xyz_stash_kernel(const MlpArgs a) { mlp_f16_body<true, true, true>(a); }

void launch_mlp_f16x3_stash(const MlpArgs& a, int num_cus, hipStream_t stream, bool single_pass, bool xyz_only) {
    if (a.M <= 0) return;
    const long long ntiles = (a.M + 127) / 128;
    const int grid = (int)(ntiles < (long long)num_cus ? ntiles : (long long)num_cus);
    if (xyz_only) {
        if (single_pass) hipLaunchKernelGGL(mlp_f16_xyz_stash_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
        else hipLaunchKernelGGL(mlp_f16x3_xyz_stash_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
        return;
    }
    if (single_pass) hipLaunchKernelGGL(mlp_f16_stash_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
    else hipLaunchKernelGGL(mlp_f16x3_stash_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
}

void launch_mlp_f16x3(const MlpArgs& a, int num_cus, hipStream_t stream, bool single_pass, bool xyz_only) {
    if (a.M <= 0) return;
    const long long ntiles = (a.M + 127) / 128;
    const int grid = (int)(ntiles < (long long)num_cus ? ntiles : (long long)num_cus);
    if (xyz_only) {
        if (single_pass) hipLaunchKernelGGL(mlp_f16_xyz_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
        else hipLaunchKernelGGL(mlp_f16x3_xyz_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
        return;
    }
    if (single_pass) hipLaunchKernelGGL(mlp_f16_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
    else hipLaunchKernelGGL(mlp_f16x3_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
}

#if NERF_PE_LX == 5
void launch_mlp_f16x3_sig(const MlpArgs& a, int num_cus, hipStream_t stream) {
    if (a.M <= 0) return;
    const long long ntiles = (a.M + 127) / 128;
    const int grid = (int)(ntiles < (long long)num_cus ? ntiles : (long long)num_cus);
    hipLaunchKernelGGL(mlp_f16x3_sig_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a);
}
void launch_mlp_f16x3_rgbskip(const MlpArgs& a, int num_cus, hipStream_t stream, unsigned long long* skip_count) {
    if (a.M <= 0) return;
    const long long ntiles = (a.M + 127) / 128;
    const int grid = (int)(ntiles < (long long)num_cus ? ntiles : (long long)num_cus);
    hipLaunchKernelGGL(mlp_f16x3_rgbskip_kernel, dim3(grid), dim3(256), kLdsTotal, stream, a, skip_count);
}
#endif

#if defined(NERF_STAMPS) && NERF_PE_LX == 5
extern "C" void nerf_debug_read_stamps_h(unsigned long long* out) {
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps_h), sizeof(unsigned long long) * 16);
}
#endif

void mlp_f16x3_set_attributes() {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16x3_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16x3_stash_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16_stash_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16x3_xyz_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16_xyz_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16x3_xyz_stash_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16_xyz_stash_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
#if NERF_PE_LX == 5
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16x3_sig_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(mlp_f16x3_rgbskip_kernel),
                              hipFuncAttributeMaxDynamicSharedMemorySize, kLdsTotal);
#endif
}

// ------------------------------------------------------------------------------------------------
// The streams + constants as index maps (host) over the (kPeLx, kLd) blob (Keras get_weights() order).  The fp16 builds
// alone have them: a bf16 stream is re-packed from its fp16 twin's table (same slots).
// ------------------------------------------------------------------------------------------------
namespace {
int h_pe_row(int v, int h) {   // slot v (0..23) of lane half h -> row of the (33, .) kernel; -1 = pad
    if (v < 3 * kPeLx) { const int c = v / kPeLx, k = v % kPeLx; return c * (1 + 2 * kPeLx) + 1 + 2 * k + h; }
    if (kPeLx != 5) {              // wide-PE build: slots 0..31 of the (63, .) kernel; raw x, y in half 0, z in half 1
        if (v == 30) return h ? 2 * (1 + 2 * kPeLx) : 0;
        return v == 31 && h == 0 ? 1 + 2 * kPeLx : -1;
    }
    if (v < 18 && h == 0) return (v - 15) * 11;
    return -1;
}
int h_hid_row(int n, int e, int h) { const int t = n >> 1, s = n & 1; return 32 * t + 16 * s + 8 * (e >> 2) + 4 * h + (e & 3); }
int h_dir_row(int v, int h, int n_angles) {   // slot v (0..15) -> row of the dir block (24 or 16 rows), -1 = pad
    if (v >= 12) return -1;
    const int c = v / 4, k = v % 4;
    if (n_angles == 2) return c * 8 + 2 * k + h;
    if (c == 1) return -1;                       // n_angles == 1: (x,z) only, src/UtilsCV.py:134-135
    return (c == 0 ? 0 : 1) * 8 + 2 * k + h;
}
}  // namespace

// EmitW(pos_hi, pos_lo (-1 in the hi-only stream), src) for every 16-bit slot pair of the stream, EmitC(pos, src) for
// every float of the constant region; src = index into the blob, -1 = zero padding.
// tail (3-pass, n_angles 1 or 2): how layer 8 is laid out -- kTailFull: BODY_LAST; kTailSig, the sigma-only stream: BODY_SIG
// alone; kTailSigFirst, the rgb-skipping kernel's stream: BODY_SIG, then the four rgb tiles as BODY_RGB.  Same constants.
enum { kTailFull = 0, kTailSig = 1, kTailSigFirst = 2 };
template <class EmitW, class EmitC>
static void pack_f16_map(int n_angles, bool hi_only, EmitW emit_w, EmitC emit_c, int tail = kTailFull) {
    const bool xyz_only = n_angles == 0;
    int shapes[12][2];
    const int n_layers = layer_dims(kPeLx, kLd, n_angles, shapes);
    struct Lay { long long k, b; int in, out; } L[12];
    long long off = 0;
    for (int i = 0; i < n_layers; ++i) {
        L[i].in = shapes[i][0]; L[i].out = shapes[i][1];
        L[i].k = off; off += (long long)L[i].in * L[i].out;
        L[i].b = off; off += L[i].out;
    }
    size_t chunk = 0;
    auto emit_body = [&](int layer, int body) {
        const int NU = body == BODY_LAST ? kHTilesLast : body == BODY_SIG ? 1 : body == BODY_HIDSIG ? 9 : (body == BODY_LAST0 || body == BODY_RGB) ? 4 : 8;
        const int NSTEP = body == BODY_PE ? kHStepsPE : (body == BODY_HID || body == BODY_HIDSIG || body == BODY_LAST0) ? kHStepsHid
                          : body == BODY_SKIP ? kHStepsPE + kHStepsHid : kHStepsHid + kHStepsDir;
        const long long b0 = (long long)chunk * (kHChunkBytes / 2);
        for (int u = 0; u < NU; ++u)
            for (int n = 0; n < NSTEP; ++n)
                for (int lane = 0; lane < 64; ++lane)
                    for (int e = 0; e < 8; ++e) {
                        const int i = lane & 31, h = lane >> 5;
                        int row;
                        if (body == BODY_PE) row = h_pe_row(n * 8 + e, h);
                        else if (body == BODY_HID || body == BODY_HIDSIG || body == BODY_LAST0) row = h_hid_row(n, e, h);
                        else if (body == BODY_SKIP) {
                            if (n < kHStepsPE) row = h_pe_row(n * 8 + e, h);
                            else row = kPeDim + h_hid_row(n - kHStepsPE, e, h);
                        } else {
                            if (n < kHStepsHid) row = h_hid_row(n, e, h);
                            else { const int r = h_dir_row((n - kHStepsHid) * 8 + e, h, n_angles); row = r < 0 ? -1 : kHidden + r; }
                        }
                        long long src = -1;
                        if (row >= 0) {
                            if ((body == BODY_LAST && u == kHTilesLast - 1) || body == BODY_SIG)
                                src = i == 0 ? L[10].k + row : -1;                                                 // sigma row
                            else if (body == BODY_HIDSIG && u == 0) src = i == 0 ? L[11].k + row : -1;           // leading sigma row
                            else if (body == BODY_HIDSIG) src = L[layer].k + (long long)row * L[layer].out + 32 * (u - 1) + i;
                            else src = L[layer].k + (long long)row * L[layer].out + 32 * u + i;
                        }
                        if (hi_only) {
                            emit_w(b0 + (long long)(u * NSTEP + n) * (kQuadBytes / 2) + lane * 8 + e, -1LL, src);
                        } else {
                            const long long q = (long long)(u * NSTEP + n) * 2;
                            emit_w(b0 + (q + 0) * (kQuadBytes / 2) + lane * 8 + e, b0 + (q + 1) * (kQuadBytes / 2) + lane * 8 + e, src);
                        }
                    }
        chunk += (NU * NSTEP * (hi_only ? 1 : 2) + kHCQ - 1) / kHCQ;
    };
    emit_body(0, BODY_PE);
    for (int l = 1; l <= 3; ++l) emit_body(l, BODY_HID);
    emit_body(4, BODY_SKIP);
    for (int l = 5; l <= 7; ++l) emit_body(l, BODY_HID);
    for (int l = 0; l < 8; ++l)
        for (int f = 0; f < 256; ++f) emit_c(kHConstBias + l * 256 + f, L[l].b + f);
    if (xyz_only) {
        emit_body(8, BODY_HIDSIG);
        emit_body(9, BODY_LAST0);
        emit_c(kXConstBiasSig + 0, L[11].b);
        for (int f = 0; f < 256; ++f) emit_c(kXConstBias8 + f, L[8].b + f);
        for (int f = 0; f < 128; ++f) emit_c(kXConstBias9 + f, L[9].b + f);
        for (int c = 0; c < 3; ++c)
            for (int f = 0; f < 128; ++f) emit_c(kXConstWrgb + c * 128 + f, L[10].k + f * 3 + c);
        for (int c = 0; c < 3; ++c) emit_c(kXConstBHead + c, L[10].b + c);
        for (int f = 0; f < 256; ++f) emit_c(kXConstWsig + f, L[11].k + f);
        return;
    }
    emit_body(8, tail == kTailFull ? BODY_LAST : BODY_SIG);
    if (tail == kTailSigFirst) emit_body(8, BODY_RGB);
    for (int f = 0; f < 128; ++f) emit_c(kHConstBias8 + f, L[8].b + f);
    emit_c(kHConstBiasSig + 0, L[10].b);
    for (int c = 0; c < 3; ++c)
        for (int f = 0; f < 128; ++f) emit_c(kHConstWrgb + c * 128 + f, L[9].k + f * 3 + c);
    for (int c = 0; c < 3; ++c) emit_c(kHConstBHead + c, L[9].b + c);
}

// stream_idx[slot] = 2 * (src + 1) + is_lo, const_idx[float] = src + 1 (nullable); 0 = padding
static void build_gather(int n_angles, bool hi_only, int tail, int32_t* stream_idx, size_t stream_bytes, int32_t* const_idx) {
    memset(stream_idx, 0, (stream_bytes / 2) * sizeof(int32_t));
    if (const_idx) memset(const_idx, 0, kConstFloats * sizeof(int32_t));
    pack_f16_map(n_angles, hi_only,
                 [&](long long ph, long long pl, long long src) {
                     if (src < 0) return;
                     stream_idx[ph] = (int32_t)(2 * (src + 1));
                     if (pl >= 0) stream_idx[pl] = (int32_t)(2 * (src + 1) + 1);
                 },
                 [&](long long pos, long long src) { if (const_idx) const_idx[pos] = (int32_t)(src + 1); }, tail);
}

void build_f16x3_gather(int n_angles, bool hi_only, int32_t* stream_idx, int32_t* const_idx) {
    const size_t bytes = n_angles == 0 ? (hi_only ? kStreamBytesF16HiXyz : kStreamBytesF16Xyz) : (hi_only ? kStreamBytesF16Hi : kStreamBytesF16);
    build_gather(n_angles, hi_only, kTailFull, stream_idx, bytes, const_idx);
}
#if NERF_PE_LX == 5
void build_f16x3_sig_gather(int n_angles, int32_t* stream_idx) {
    build_gather(n_angles, false, kTailSig, stream_idx, kStreamBytesF16Sig, nullptr);
}
void build_f16x3_rgbskip_gather(int n_angles, int32_t* stream_idx) {
    build_gather(n_angles, false, kTailSigFirst, stream_idx, kStreamBytesF16Skip, nullptr);
}
#endif
#endif   // NERF_BF16

}  // namespace nerf (:: wide, :: bf16, :: bf16::wide)
