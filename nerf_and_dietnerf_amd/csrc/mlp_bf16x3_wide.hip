// mlp_bf16x3_wide.hip -- the wide-PE build of mlp_bf16x3.hip for networks with n_pos_enc_dim_xyz 6..10 (namespace
// nerf::bf16::wide): the bf16 3-pass render kernels with 10 xyz octaves, as mlp_f16x3_wide.hip is to mlp_f16x3.hip.
#define NERF_BF16 1
#define NERF_PE_LX 10
#include "mlp_f16x3.hip"
