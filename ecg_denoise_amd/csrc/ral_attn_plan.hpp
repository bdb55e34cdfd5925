// Attention dispatch: which kernel runs for a (direction, shape, arithmetic), decided once (ral_attn_plan.hip).  The plan
// functions are pure host code - no HIP call, usable without a device; the launchers (ral_kernels.hpp) execute a plan and
// never choose.  DESIGN.md section 3 has the two dispatch tables.
#pragma once
#include <stddef.h>

// One enumerator per kernel instance the launchers can start: X(enumerator, template-id as a kernel trace prints it).
// (Default template arguments spelled out: k_attn_fwd<QT, NT, TAB, F16, RAG>, k_attn_bwd<QT, NT, TAB, RAG>.)
#define ATTN_KERNELS(X)                                                                                                  \
  /* forward: tile kernels of ral_fwd.hip (workgroup per (window, head group)) */                                       \
  X(FWD_RAG, "k_attn_fwd<1, 0, true, false, true>")                                                                     \
  X(FWD_G1, "k_attn_fwd<1, 0, true, false, false>")                                                                     \
  X(FWD_G2, "k_attn_fwd<2, 0, true, false, false>")                                                                     \
  X(FWD_G2_F16, "k_attn_fwd<2, 0, true, true, false>")                                                                  \
  X(FWD_G2_N32, "k_attn_fwd<2, 32, false, false, false>")                                                               \
  X(FWD_T32, "k_attn_fwd_t32<2, false>")                                                                                \
  X(FWD_T32_TAB, "k_attn_fwd_t32<2, true>")                                                                             \
  /* forward: query per lane on the scalar path (ral_fwd.hip) */                                                        \
  X(FWD_V, "k_attn_fwd_v<false>")                                                                                       \
  X(FWD_V_TAB, "k_attn_fwd_v<true>")                                                                                    \
  /* forward: wave per head (ral_attn.hip), <N, table, f16> */                                                          \
  X(FWD_W32, "k_attn_fwd_w<32, false, false>")                                                                          \
  X(FWD_W32_F16, "k_attn_fwd_w<32, false, true>")                                                                       \
  X(FWD_W32_TAB, "k_attn_fwd_w<32, true, false>")                                                                       \
  X(FWD_W32_TAB_F16, "k_attn_fwd_w<32, true, true>")                                                                    \
  X(FWD_W64, "k_attn_fwd_w<64, false, false>")                                                                          \
  X(FWD_W64_F16, "k_attn_fwd_w<64, false, true>")                                                                       \
  X(FWD_W64_TAB, "k_attn_fwd_w<64, true, false>")                                                                       \
  X(FWD_W64_TAB_F16, "k_attn_fwd_w<64, true, true>")                                                                    \
  X(FWD_W128, "k_attn_fwd_w<128, false, false>")                                                                        \
  X(FWD_W128_F16, "k_attn_fwd_w<128, false, true>")                                                                     \
  X(FWD_W128_TAB, "k_attn_fwd_w<128, true, false>")                                                                     \
  X(FWD_W128_TAB_F16, "k_attn_fwd_w<128, true, true>")                                                                  \
  /* backward: tile kernels of ral_bwd.hip */                                                                           \
  X(BWD_RAG, "k_attn_bwd<1, 0, true, true>")                                                                            \
  X(BWD_G1, "k_attn_bwd<1, 0, true, false>")                                                                            \
  X(BWD_G2, "k_attn_bwd<2, 0, true, false>")                                                                            \
  X(BWD_G2_N32, "k_attn_bwd<2, 32, false, false>")                                                                      \
  X(BWD_G2_N64_TAB, "k_attn_bwd<2, 64, true, false>")                                                                   \
  /* backward: the two scalar-path sweeps (ral_bwd.hip) */                                                              \
  X(BWD_V, "k_attn_bwd_vq + k_attn_bwd_vkv")                                                                            \
  /* backward: wave per head, fp32 tiles (ral_attn.hip), <N, table> */                                                  \
  X(BWD_W32, "k_attn_bwd_w<32, false>")                                                                                 \
  X(BWD_W32_TAB, "k_attn_bwd_w<32, true>")                                                                              \
  X(BWD_W64, "k_attn_bwd_w<64, false>")                                                                                 \
  X(BWD_W64_TAB, "k_attn_bwd_w<64, true>")                                                                              \
  X(BWD_W128, "k_attn_bwd_w<128, false>")                                                                               \
  X(BWD_W128_TAB, "k_attn_bwd_w<128, true>")                                                                            \
  /* backward: one sweep on the f16 matrix cores (ral_attnm.hip): wave per head <N, table>, workgroup <KT, table> */    \
  X(BWD_M32, "k_attn_bwd_m<32, false>")                                                                                 \
  X(BWD_M32_TAB, "k_attn_bwd_m<32, true>")                                                                              \
  X(BWD_M64, "k_attn_bwd_m<64, false>")                                                                                 \
  X(BWD_M64_TAB, "k_attn_bwd_m<64, true>")                                                                              \
  X(BWD_M128, "k_attn_bwd_m<128, false>")                                                                               \
  X(BWD_M128_TAB, "k_attn_bwd_m<128, true>")                                                                            \
  X(BWD_MH4, "k_attn_bwd_mh<4, false>")                                                                                 \
  X(BWD_MH4_TAB, "k_attn_bwd_mh<4, true>")                                                                              \
  X(BWD_MH8, "k_attn_bwd_mh<8, false>")                                                                                 \
  X(BWD_MH8_TAB, "k_attn_bwd_mh<8, true>")

enum class AttnKernel : int {
#define X(e, name) e,
  ATTN_KERNELS(X)
#undef X
};

struct AttnPlan {
  AttnKernel kernel;
  const char* name;        // the template-id of ATTN_KERNELS
  int hg;                  // heads per work item
  int threads;
  size_t lds;              // dynamic LDS bytes per workgroup
  size_t scratch_floats;   // bwd only, for batch B: what the caller hands to launch_attn_bwd
  bool table_partials;     // bwd: leaves one row of R-wave table-gradient partials per workgroup for k_attn_tpart_reduce
  int rows;                // bwd, persistent kernels: upper bound of the grid = the rows of partials the scratch is sized for
};
// Len: 0 = no R-wave table.  f16: S / dP tiles as fp16-pair products on the f16 matrix cores (0: exact fp32 MFMA).
// NE: existing tokens of the N slots (0 or N: all; fewer: padded windows, the generic kernel masks the keys past NE).
AttnPlan attn_fwd_plan(int N, int H, int Len, int f16, int NE);
AttnPlan attn_bwd_plan(int N, int H, int Len, int f16, int NE, int B);
// 1 unless the switch ATTN_F16 is 0 (what the handle-free operator entry points use; a model handle follows its f16_split option)
int attn_f16_default();
// the persistent wave-per-head kernels run at most one workgroup per four tasks and at most this many workgroups
constexpr int ATTN_ROWS_MAX = 1024;
