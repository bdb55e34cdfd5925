// Linear-layer dispatch of a transformer block: which kernel runs the QKV projection, the MLP half block, their backwards
// and the four weight-gradient products for a (shape, mode, arithmetic), decided once (ral_block_plan.hip).  Pure host
// arithmetic - no HIP call, usable without a device; the launchers (ral_kernels.hpp) execute a plan and never choose.
// DESIGN.md section 3, "Linear-layer dispatch", has the first-match tables.
#pragma once
#include <stddef.h>

// One enumerator per kernel instance the launchers can start: X(enumerator, template-id as a kernel trace prints it).
// (Default template arguments spelled out: k_mlp_bwd_h<C, NCH, NTH>, k_dw<M, NC, MS, NS, LAYY, XF, H>.)
#define BLOCK_KERNELS(X)                                                                                                 \
  /* QKV projection (ral_fwd.hip): fp32 MFMA <C>; split operands <C, GT>: weight-stationary / token groups */           \
  X(QKV_FWD_8, "k_qkv_fwd<8>")                                                                                          \
  X(QKV_FWD_16, "k_qkv_fwd<16>")                                                                                        \
  X(QKV_FWD_32, "k_qkv_fwd<32>")                                                                                        \
  X(QKV_FWD_64, "k_qkv_fwd<64>")                                                                                        \
  X(QKV_FWD_128, "k_qkv_fwd<128>")                                                                                      \
  X(QKV_FWD_WS_64, "k_qkv_fwd_ws<64, 64>")                                                                              \
  X(QKV_FWD_WS_128, "k_qkv_fwd_ws<128, 64>")                                                                            \
  X(QKV_FWD_H_32, "k_qkv_fwd_h<32, 64>")                                                                                \
  X(QKV_FWD_H_64, "k_qkv_fwd_h<64, 64>")                                                                                \
  /* MLP half block, forward: fp32 MFMA <C, NCH> (ral_fwd.hip) */                                                       \
  X(MLP_FWD_8_1, "k_mlp_fwd<8, 1>")                                                                                     \
  X(MLP_FWD_8_2, "k_mlp_fwd<8, 2>")                                                                                     \
  X(MLP_FWD_8_4, "k_mlp_fwd<8, 4>")                                                                                     \
  X(MLP_FWD_16_1, "k_mlp_fwd<16, 1>")                                                                                   \
  X(MLP_FWD_16_2, "k_mlp_fwd<16, 2>")                                                                                   \
  X(MLP_FWD_16_4, "k_mlp_fwd<16, 4>")                                                                                   \
  X(MLP_FWD_32_1, "k_mlp_fwd<32, 1>")                                                                                   \
  X(MLP_FWD_32_2, "k_mlp_fwd<32, 2>")                                                                                   \
  X(MLP_FWD_32_4, "k_mlp_fwd<32, 4>")                                                                                   \
  X(MLP_FWD_64_1, "k_mlp_fwd<64, 1>")                                                                                   \
  X(MLP_FWD_64_2, "k_mlp_fwd<64, 2>")                                                                                   \
  X(MLP_FWD_64_4, "k_mlp_fwd<64, 4>")                                                                                   \
  X(MLP_FWD_128_1, "k_mlp_fwd<128, 1>")                                                                                 \
  X(MLP_FWD_128_2, "k_mlp_fwd<128, 2>")                                                                                 \
  X(MLP_FWD_128_4, "k_mlp_fwd<128, 4>")                                                                                 \
  /* ... split operands <C, NCH, NTH> (ral_fwd.hip) */                                                                  \
  X(MLP_FWD_H_32_1, "k_mlp_fwd_h<32, 1, 512>")                                                                          \
  X(MLP_FWD_H_32_2, "k_mlp_fwd_h<32, 2, 512>")                                                                          \
  X(MLP_FWD_H_32_4, "k_mlp_fwd_h<32, 4, 512>")                                                                          \
  X(MLP_FWD_H_64_1, "k_mlp_fwd_h<64, 1, 256>")                                                                          \
  X(MLP_FWD_H_64_8, "k_mlp_fwd_h<64, 8, 256>")                                                                          \
  X(MLP_FWD_H_128_4, "k_mlp_fwd_h<128, 4, 256>")                                                                        \
  X(MLP_FWD_H_128_8, "k_mlp_fwd_h<128, 8, 256>")                                                                        \
  /* ... wave-autonomous strips of the narrow levels (ral_mlpw.hip): fp32 MFMA, fp16 pairs */                           \
  X(MLP_FWD_W_8, "k_mlp_fwd_w<8>")                                                                                      \
  X(MLP_FWD_W_16, "k_mlp_fwd_w<16>")                                                                                    \
  X(MLP_FWD_W_32, "k_mlp_fwd_w<32>")                                                                                    \
  X(MLP_FWD_WH_8, "k_mlp_fwd_wh<8>")                                                                                    \
  X(MLP_FWD_WH_16, "k_mlp_fwd_wh<16>")                                                                                  \
  X(MLP_FWD_WH_32, "k_mlp_fwd_wh<32>")                                                                                  \
  /* MLP half block, backward: fp32 MFMA <C, NCH> (ral_bwd.hip) */                                                      \
  X(MLP_BWD_8_1, "k_mlp_bwd<8, 1>")                                                                                     \
  X(MLP_BWD_8_2, "k_mlp_bwd<8, 2>")                                                                                     \
  X(MLP_BWD_8_4, "k_mlp_bwd<8, 4>")                                                                                     \
  X(MLP_BWD_16_1, "k_mlp_bwd<16, 1>")                                                                                   \
  X(MLP_BWD_16_2, "k_mlp_bwd<16, 2>")                                                                                   \
  X(MLP_BWD_16_4, "k_mlp_bwd<16, 4>")                                                                                   \
  X(MLP_BWD_32_1, "k_mlp_bwd<32, 1>")                                                                                   \
  X(MLP_BWD_32_2, "k_mlp_bwd<32, 2>")                                                                                   \
  X(MLP_BWD_32_4, "k_mlp_bwd<32, 4>")                                                                                   \
  X(MLP_BWD_64_1, "k_mlp_bwd<64, 1>")                                                                                   \
  X(MLP_BWD_64_2, "k_mlp_bwd<64, 2>")                                                                                   \
  X(MLP_BWD_64_4, "k_mlp_bwd<64, 4>")                                                                                   \
  X(MLP_BWD_128_1, "k_mlp_bwd<128, 1>")                                                                                 \
  X(MLP_BWD_128_2, "k_mlp_bwd<128, 2>")                                                                                 \
  X(MLP_BWD_128_4, "k_mlp_bwd<128, 4>")                                                                                 \
  /* ... narrow levels with the fc1 / fc2 weight gradients fused <C, TW> (ral_bwd.hip) */                               \
  X(MLP_BWD_S_8_1, "k_mlp_bwd_s<8, 1>")                                                                                 \
  X(MLP_BWD_S_8_2, "k_mlp_bwd_s<8, 2>")                                                                                 \
  X(MLP_BWD_S_8_4, "k_mlp_bwd_s<8, 4>")                                                                                 \
  X(MLP_BWD_S_16_1, "k_mlp_bwd_s<16, 1>")                                                                               \
  X(MLP_BWD_S_16_2, "k_mlp_bwd_s<16, 2>")                                                                               \
  X(MLP_BWD_S_32_1, "k_mlp_bwd_s<32, 1>")                                                                               \
  X(MLP_BWD_S_32_2, "k_mlp_bwd_s<32, 2>")                                                                               \
  /* ... split operands <C, NCH, NTH>: four waves (256), eight waves (512) (ral_bwd.hip) */                             \
  X(MLP_BWD_H4_32_4, "k_mlp_bwd_h<32, 4, 256>")                                                                         \
  X(MLP_BWD_H4_64_4, "k_mlp_bwd_h<64, 4, 256>")                                                                         \
  X(MLP_BWD_H4_128_4, "k_mlp_bwd_h<128, 4, 256>")                                                                       \
  X(MLP_BWD_H8_32_1, "k_mlp_bwd_h<32, 1, 512>")                                                                         \
  X(MLP_BWD_H8_64_1, "k_mlp_bwd_h<64, 1, 512>")                                                                         \
  /* ... strips of the narrow levels, weight gradients fused (ral_mlpw.hip): <C>; two waves per tile <32, fp16 pairs> */ \
  X(MLP_BWD_W_8, "k_mlp_bwd_w<8>")                                                                                      \
  X(MLP_BWD_W_16, "k_mlp_bwd_w<16>")                                                                                    \
  X(MLP_BWD_W2_32, "k_mlp_bwd_w2<32, false>")                                                                           \
  X(MLP_BWD_W2_32_H, "k_mlp_bwd_w2<32, true>")                                                                          \
  /* QKV projection, backward (ral_bwd.hip): fp32 MFMA, split operands */                                               \
  X(QKV_BWD_8, "k_qkv_bwd<8>")                                                                                          \
  X(QKV_BWD_16, "k_qkv_bwd<16>")                                                                                        \
  X(QKV_BWD_32, "k_qkv_bwd<32>")                                                                                        \
  X(QKV_BWD_64, "k_qkv_bwd<64>")                                                                                        \
  X(QKV_BWD_128, "k_qkv_bwd<128>")                                                                                      \
  X(QKV_BWD_H_32, "k_qkv_bwd_h<32>")                                                                                    \
  X(QKV_BWD_H_64, "k_qkv_bwd_h<64>")                                                                                    \
  X(QKV_BWD_H_128, "k_qkv_bwd_h<128>")                                                                                  \
  /* weight gradients (ral_dw.hip), <M, NC, MS, NS, LAYY, XF, H>: fc2, fc1, proj, qkv; _H: split operands */            \
  X(DW_FC2_8, "k_dw<8, 32, 8, 32, 0, 3, false>")                                                                        \
  X(DW_FC2_16, "k_dw<16, 64, 16, 64, 0, 3, false>")                                                                     \
  X(DW_FC2_32, "k_dw<32, 128, 32, 128, 0, 3, false>")                                                                   \
  X(DW_FC2_64, "k_dw<64, 256, 64, 128, 0, 3, false>")                                                                   \
  X(DW_FC2_128, "k_dw<128, 512, 128, 128, 0, 3, false>")                                                                \
  X(DW_FC2_32_H, "k_dw<32, 128, 32, 128, 0, 3, true>")                                                                  \
  X(DW_FC2_64_H, "k_dw<64, 256, 64, 128, 0, 3, true>")                                                                  \
  X(DW_FC2_128_H, "k_dw<128, 512, 128, 128, 0, 3, true>")                                                               \
  X(DW_FC1_8, "k_dw<32, 8, 32, 8, 0, 1, false>")                                                                        \
  X(DW_FC1_16, "k_dw<64, 16, 64, 16, 0, 1, false>")                                                                     \
  X(DW_FC1_32, "k_dw<128, 32, 128, 32, 0, 1, false>")                                                                   \
  X(DW_FC1_64, "k_dw<256, 64, 128, 64, 0, 1, false>")                                                                   \
  X(DW_FC1_128, "k_dw<512, 128, 128, 128, 0, 1, false>")                                                                \
  X(DW_FC1_32_H, "k_dw<128, 32, 128, 32, 0, 1, true>")                                                                  \
  X(DW_FC1_64_H, "k_dw<256, 64, 128, 64, 0, 1, true>")                                                                  \
  X(DW_FC1_128_H, "k_dw<512, 128, 128, 128, 0, 1, true>")                                                               \
  X(DW_PROJ_8, "k_dw<8, 8, 8, 8, 0, 0, false>")                                                                         \
  X(DW_PROJ_16, "k_dw<16, 16, 16, 16, 0, 0, false>")                                                                    \
  X(DW_PROJ_32, "k_dw<32, 32, 32, 32, 0, 0, false>")                                                                    \
  X(DW_PROJ_64, "k_dw<64, 64, 64, 64, 0, 0, false>")                                                                    \
  X(DW_PROJ_128, "k_dw<128, 128, 128, 128, 0, 0, false>")                                                               \
  X(DW_PROJ_32_H, "k_dw<32, 32, 32, 32, 0, 0, true>")                                                                   \
  X(DW_PROJ_64_H, "k_dw<64, 64, 64, 64, 0, 0, true>")                                                                   \
  X(DW_PROJ_128_H, "k_dw<128, 128, 128, 128, 0, 0, true>")                                                              \
  X(DW_QKV_8, "k_dw<24, 8, 24, 8, 1, 2, false>")                                                                        \
  X(DW_QKV_16, "k_dw<48, 16, 48, 16, 1, 2, false>")                                                                     \
  X(DW_QKV_32, "k_dw<96, 32, 96, 32, 1, 2, false>")                                                                     \
  X(DW_QKV_64, "k_dw<192, 64, 96, 64, 1, 2, false>")                                                                    \
  X(DW_QKV_128, "k_dw<384, 128, 128, 128, 1, 2, false>")                                                                \
  X(DW_QKV_32_H, "k_dw<96, 32, 96, 32, 1, 2, true>")                                                                    \
  X(DW_QKV_64_H, "k_dw<192, 64, 96, 64, 1, 2, true>")                                                                   \
  X(DW_QKV_128_H, "k_dw<384, 128, 128, 128, 1, 2, true>")

enum class BlockKernel : int {
  NONE = -1,   // a weight-gradient product that is not launched: the MLP backward produced it (mlp_dw_fused)
#define X(e, name) e,
  BLOCK_KERNELS(X)
#undef X
};

// what a plan is a function of
struct BlockShape {
  int C, N;           // channel width {8, 16, 32, 64, 128}, token slots of a window (a multiple of 16)
  int NE;             // existing tokens of the N slots (0 or N: all; fewer: padded windows)
  bool training;      // the forward keeps what a backward reads
  bool second_out;    // the MLP forward also writes block output + addend (sum_out)
  bool want_dw;       // the backward produces weight gradients (false: data gradients only)
  bool f16_wide;      // the model allows fp16-pair products at this width: f16_split > 0 && C >= f16_split
  bool f16_narrow;    // ... and in the strip kernels of the narrow levels: f16_split > 0 && narrow_f16
};
struct BlockLaunch {
  BlockKernel kernel;
  const char* name;   // the template-id of BLOCK_KERNELS ("" for NONE)
  int threads;
  size_t lds;         // dynamic LDS bytes per workgroup
  int chunks;         // hidden chunks of an MLP kernel (0: it has none); token chunk of a weight-gradient product
  bool split;         // weight-gradient product: operands as fp16 pairs (k_dw<..., true>)
};
enum { DW_FC2 = 0, DW_FC1 = 1, DW_PROJ = 2, DW_QKV = 3 };
struct BlockPlan {
  BlockLaunch qkv_fwd, mlp_fwd, mlp_bwd, qkv_bwd, dw[4];
  bool stores_upre;    // the training forward keeps u_pre for this block (workspace layout, forward and backward read it here)
  bool mlp_dw_fused;   // the MLP backward produces the fc1 / fc2 weight and bias gradients itself: dw[DW_FC2], dw[DW_FC1] are NONE
  bool dw_split;       // the data-gradient kernels publish gmax and the weight-gradient products run on split operands
};
BlockPlan block_plan(const BlockShape& sh);
// a launcher was handed an entry it has no case for (an enumerator added to the list and the plan but not to the launcher): a
// missing kernel is an error, never a silent no-op
[[noreturn]] void block_launch_missing(const char* launcher, const BlockLaunch& p);
// widths whose Linear layers have split-operand kernels: their weight matrices get tiled fp16 planes
inline bool block_has_planes(int C) { return C == 32 || C == 64 || C == 128; }
