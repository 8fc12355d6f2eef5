// mlp_f16x3_wide.hip -- the wide-PE build of mlp_f16x3.hip for networks with n_pos_enc_dim_xyz 6..10 (namespace
// nerf::wide): the same fused kernels (3-pass, one-tile single-pass, stash forwards; view-direction and xyz-only networks)
// with 10 xyz octaves encoded in registers and 4 PE k-steps (64 slots >= 3 + 6 * 10) instead of 3, and the gather
// tables of that layout.  Lx 6..9 run on it with zero rows for the octaves they lack (weight_tables.hip, aim_gather).  Its own translation unit: the Makefile's mlp_%.o rule lints its ISA like the others'.
#define NERF_PE_LX 10
#include "mlp_f16x3.hip"
