// U-Net stage dispatch: the network's 11 conv stages as ONE table, and which kernel runs a stage at a (leads, L, B, mode) with
// what grid, windows per pass and dynamic LDS, decided once (ral_unet_plan.hip).  Pure host arithmetic - no HIP call, usable
// without a device; the launchers (ral_unet.hip) execute a plan and never choose.  DESIGN.md section 3, "U-Net stage dispatch",
// has the table and the first-match rules.
#pragma once
#include <stddef.h>

#define UNET_STAGES 11
#define UNET_MAXC 32             // widest stage
#ifndef UNET_FWD_THREADS
#define UNET_FWD_THREADS 512     // workgroup of k_unet_fwd_t / k_unet_bwd_t (their __launch_bounds__)
#endif
#define UNET_BWD_THREADS 512
#define UNET_PART_ROWS 1024      // most scratch rows the workspace keeps for the weight-gradient partials of a backward stage
#define UINF_COEFF_FLOATS 512    // biases + BatchNorm (scale, shift) pairs the fused inference kernel keeps in LDS (uinf::PTOT - PB)

enum { ACT_NONE = 0, ACT_LRELU = 1 };
enum { CONV = 0, CONVT = 1 };    // Stage::mode
enum { TY_ZBN = 0 /* z -> BN -> [lrelu] */, TY_ABN = 1 /* lrelu(z) -> BN */, TY_PLAIN = 2 /* no BN */ };
enum { UMODE_CONV = 0, UMODE_BOTTLENECK = 1, UMODE_CONVT = 2 };   // the MODE of k_unet_fwd_t / k_unet_bwd_t
enum { UZ_NONE = -1, UZ_X = -2 };   // an operand that is not a stage output: absent / the network's input x

// One input operand of a stage: act(BatchNorm(z[z])); accumulate: the backward ADDS this operand's gradient to G[z] (a consumer
// that ran before it - stages run in reverse - has written it), 0: it writes it
struct UOperand { int z, act, accumulate; };
// One stage = one conv layer; its output is z[stage index]: 0-3 encoder, 4-6 bottleneck, 7-10 decoder
struct UStageGeom {
  int cin, cout, ks, mode /* UMODE_* */, stride, pad;   // (stride, pad: of Stage, read in CONV mode; CONVT is k4 s2 p1 by construction)
  int type /* TY_* */, post_lrelu;
  int bn;                 // BatchNorm index of the output (0-3 enc, 4-5 bottleneck, 6-9 dec), -1: none (z[6] = r)
  UOperand a, b, r;       // main input, additive skip, residual added to the OUTPUT
  int len_shift;          // lout = L >> len_shift
};
const UStageGeom* unet_stages(int leads);   // UNET_STAGES rows; leads 1 or 2
inline int unet_len(const UStageGeom* g, int z, int L) { return z == UZ_X ? L : L >> g[z].len_shift; }   // length of z[z]

// <CIN, COUT, KS, MODE> of the specialised stage kernels, forward and backward: stages 4 and 6 share <32, 32, 1, 1>; stages 0
// and 10 have an instance per lead count.  (The plan's lookup and the two launchers expand it; enumerator _T_ci_co_k_md.)
#define UNET_T_INSTANCES(T) \
  T(1, 4, 3, 0) T(2, 4, 3, 0) T(4, 8, 3, 0) T(8, 16, 3, 0) T(16, 32, 3, 0) T(32, 32, 1, 1) T(32, 32, 3, 1) \
  T(32, 16, 4, 2) T(16, 8, 4, 2) T(8, 4, 4, 2) T(4, 1, 4, 2) T(4, 2, 4, 2)
// One enumerator per kernel instance the launchers can start: X(enumerator, template-id as a kernel trace prints it).
#define UNET_KERNELS(X)                           \
  X(FWD, "k_unet_fwd")                            \
  X(BWD, "k_unet_bwd")                            \
  X(FWD_T_1_4_3_0, "k_unet_fwd_t<1, 4, 3, 0>")    \
  X(FWD_T_2_4_3_0, "k_unet_fwd_t<2, 4, 3, 0>")    \
  X(FWD_T_4_8_3_0, "k_unet_fwd_t<4, 8, 3, 0>")    \
  X(FWD_T_8_16_3_0, "k_unet_fwd_t<8, 16, 3, 0>")  \
  X(FWD_T_16_32_3_0, "k_unet_fwd_t<16, 32, 3, 0>") \
  X(FWD_T_32_32_1_1, "k_unet_fwd_t<32, 32, 1, 1>") \
  X(FWD_T_32_32_3_1, "k_unet_fwd_t<32, 32, 3, 1>") \
  X(FWD_T_32_16_4_2, "k_unet_fwd_t<32, 16, 4, 2>") \
  X(FWD_T_16_8_4_2, "k_unet_fwd_t<16, 8, 4, 2>")  \
  X(FWD_T_8_4_4_2, "k_unet_fwd_t<8, 4, 4, 2>")    \
  X(FWD_T_4_1_4_2, "k_unet_fwd_t<4, 1, 4, 2>")    \
  X(FWD_T_4_2_4_2, "k_unet_fwd_t<4, 2, 4, 2>")    \
  X(BWD_T_1_4_3_0, "k_unet_bwd_t<1, 4, 3, 0>")    \
  X(BWD_T_2_4_3_0, "k_unet_bwd_t<2, 4, 3, 0>")    \
  X(BWD_T_4_8_3_0, "k_unet_bwd_t<4, 8, 3, 0>")    \
  X(BWD_T_8_16_3_0, "k_unet_bwd_t<8, 16, 3, 0>")  \
  X(BWD_T_16_32_3_0, "k_unet_bwd_t<16, 32, 3, 0>") \
  X(BWD_T_32_32_1_1, "k_unet_bwd_t<32, 32, 1, 1>") \
  X(BWD_T_32_32_3_1, "k_unet_bwd_t<32, 32, 3, 1>") \
  X(BWD_T_32_16_4_2, "k_unet_bwd_t<32, 16, 4, 2>") \
  X(BWD_T_16_8_4_2, "k_unet_bwd_t<16, 8, 4, 2>")  \
  X(BWD_T_8_4_4_2, "k_unet_bwd_t<8, 4, 4, 2>")    \
  X(BWD_T_4_1_4_2, "k_unet_bwd_t<4, 1, 4, 2>")    \
  X(BWD_T_4_2_4_2, "k_unet_bwd_t<4, 2, 4, 2>")    \
  X(INFER_1, "k_unet_infer<1>")                   \
  X(INFER_2, "k_unet_infer<2>")

enum class UKernel : int {
  NONE = -1,   // a pass-level answer that is no kernel: the eval forward runs stage by stage
#define X(e, name) e,
  UNET_KERNELS(X)
#undef X
};

struct UStageLaunch {
  UKernel kernel;
  const char* name;        // the template-id of UNET_KERNELS ("" for NONE)
  int threads;
  int grid;                // workgroups; 0 for the fused kernel: the workgroups resident at once, a device question (occupancy
                           // query at the model's first fused forward)
  int windows_per_pass;    // WP of the specialised kernels (a workgroup loops over passes of WP windows); 1: the generic kernels
  size_t lds;              // dynamic LDS bytes per workgroup
};
// stage si of a forward (training: batch statistics, else the stage-by-stage eval forward) or a backward pass over B windows
UStageLaunch unet_stage_plan(int leads, int L, int B, bool training, bool backward, int si);

struct UPassPlan {
  bool fold;               // backward stages leave weight-gradient partials in scratch rows that k_unet_fold sums (every stage
                           // runs a specialised kernel); else some stage is generic and every gradient is an atomic
  bool fused_eval;         // the eval forward is ONE kernel: `fused`
  UStageLaunch fused;      // (kernel NONE unless fused_eval)
};
UPassPlan unet_pass_plan(int leads, int L, bool train_cfg, bool fused_option);
bool unet_fused_default();   // the process-wide default of a model's "unet_fused" option (switch UNET_FUSED, default 1)
// a launcher was handed an entry it has no case for: a missing kernel is an error, never another kernel
[[noreturn]] void unet_launch_missing(const char* launcher, const UStageLaunch& p);
