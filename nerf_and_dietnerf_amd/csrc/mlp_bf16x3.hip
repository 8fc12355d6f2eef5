// mlp_bf16x3.hip -- the bf16 build of mlp_f16x3.hip (namespace nerf::bf16): its 3-pass render kernels -- view-direction
// network, xyz-only network, sigma-only coarse pass -- with every operand split into two bf16 values (hi = the top 16 bits
// of the fp32 value, lo = the rounded rest) and v_mfma_f32_32x32x16_bf16: NERF_PRECISION_BF16X3, fp32-class results with
// fp32's exponent range.  Kernels only: the bf16 hi/lo streams have the geometry and constants of the fp16 3-pass streams
// and are re-packed from their gather tables.  Its own translation unit: the Makefile's mlp_%.o rule lints its ISA.
#define NERF_BF16 1
#include "mlp_f16x3.hip"
