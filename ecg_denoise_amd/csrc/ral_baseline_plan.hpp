// Baseline network dispatch: the two comparison baselines, ACDAE and DANet, each as ONE table of 8 rows, and the ordered list of
// launches of a forward or backward pass at a (leads, L, B) - kernel, grid, threads, dynamic LDS - decided once
// (ral_baseline_plan.hip).  Pure host arithmetic - no HIP call, usable without a device; the launchers (ral_acdae.hip,
// ral_danet.hip) execute a pass and never choose.  DESIGN.md section 3, "Baseline network dispatch", has the tables, the
// first-match rules and the grid caps.
#pragma once
#include <stddef.h>
#include <string>
#include "../../include/ralenet.h"

#define BASELINE_LAYERS 8             // rows of either table
#define BASELINE_MAX_LAUNCHES 38      // the longest pass (DANet, either direction)
#define BASELINE_LDS_MAX (160 * 1024) // LDS of a CU: no planned launch of the legal space needs more (the plan aborts on one that
                                      // does; tests/test_baseline_plan_cpu.py sweeps the space)
enum { BL_NONE = -1 };                // a row's skip / second input that does not exist
#define BASELINE_THREADS 256          // workgroup of every kernel of both networks (their __launch_bounds__)
#define ACDAE_HALO 8                  // zero halo of ACDAE's LDS rows (HALO in every k_acd_* kernel)
#define DANET_HALO 12                 // zero halo of DANet's conv tiles (CH in ral_danet.hip)

// ---- ACDAE: encoder 0-3 (Conv1d -> MaxPool1d(2) -> LeakyReLU), decoder 0-3 (ConvTranspose1d -> Upsample x2 -> LeakyReLU -> ECA,
// + the skip).  The input of row i is the output of row i - 1 (row 0: x); lengths are L >> shift.
struct AcdaeLayer {
  int cin, cout, ks;
  int convt;                 // 0: encoder row, 1: decoder row
  int in_shift, out_shift;
  int skip;                  // the row whose output is added to this row's output (an encoder row), or BL_NONE
};
const AcdaeLayer* acdae_layers();

// ---- DANet: encoder cell 0-3, decoder cell 0-3 as rows 4-7.  cin .. tr are the kernels' Geo with the lengths as shifts; the
// input of row i is the output of row i - 1 (row 0: x) plus, where in1 names one, the output of row in1.
struct DanetCell {
  int cin, c, k, p, tr;      // channels in / out, taps, padding, transposed (stride 2 both ways)
  int in_shift, out_shift;
  int in1;                   // the encoder row whose output a decoder cell adds to its input, or BL_NONE
  int dam;                   // the cell ends in a DAM
};
const DanetCell* danet_cells(int leads);   // leads must be 2 (danet_legal)

// One enumerator per kernel instance the launchers can start: X(enumerator, template-id as a kernel trace prints it).  Exactly
// the instances some legal configuration launches.
#define ACDAE_KERNELS(X)                         \
  X(ACD_ENC_FWD_13, "k_acd_enc_fwd<13>")         \
  X(ACD_ENC_FWD_7, "k_acd_enc_fwd<7>")           \
  X(ACD_ENC_FWD_M_7, "k_acd_enc_fwd_m<7>")       \
  X(ACD_DEC_FWD_7, "k_acd_dec_fwd<7>")           \
  X(ACD_DEC_FWD_13, "k_acd_dec_fwd<13>")         \
  X(ACD_DEC_BWD_7, "k_acd_dec_bwd<7>")           \
  X(ACD_DEC_BWD_13, "k_acd_dec_bwd<13>")         \
  X(ACD_ENC_BWD_13, "k_acd_enc_bwd<13>")         \
  X(ACD_ENC_BWD_7, "k_acd_enc_bwd<7>")           \
  X(ACD_DW_M_13_C, "k_acd_dw_m<13, false>")      \
  X(ACD_DW_M_7_C, "k_acd_dw_m<7, false>")        \
  X(ACD_DW_M_7_T, "k_acd_dw_m<7, true>")         \
  X(ACD_DW_13_T, "k_acd_dw<13, true>")
#define DANET_KERNELS(X)                         \
  X(DN_CONV_17_C, "k_dn_conv<17, false>")        \
  X(DN_CONV_3_C, "k_dn_conv<3, false>")          \
  X(DN_CONV_4_T, "k_dn_conv<4, true>")           \
  X(DN_CONV_18_T, "k_dn_conv<18, true>")         \
  X(DN_CONV_B_17_C, "k_dn_conv_b<17, false>")    \
  X(DN_CONV_B_3_C, "k_dn_conv_b<3, false>")      \
  X(DN_CONV_B_4_T, "k_dn_conv_b<4, true>")       \
  X(DN_CONV_B_18_T, "k_dn_conv_b<18, true>")     \
  X(DN_FCN_MID, "k_dn_fcn_mid")                  \
  X(DN_ACT_4, "k_dn_act<4>")                     \
  X(DN_ACT_1, "k_dn_act<1>")                     \
  X(DN_DAM1, "k_dn_dam1")                        \
  X(DN_OUT, "k_dn_out")                          \
  X(DN_DAM_B, "k_dn_dam_b")                      \
  X(DN_FCN_BMID, "k_dn_fcn_bmid")                \
  X(DN_BN_B, "k_dn_bn_b")                        \
  X(DN_ACT_B_4, "k_dn_act_b<4>")                 \
  X(DN_ACT_B_1, "k_dn_act_b<1>")

enum class BKernel : int {
#define X(e, name) e,
  ACDAE_KERNELS(X) DANET_KERNELS(X)
#undef X
};

struct BLaunch {
  int layer;               // row of the network's table
  BKernel kernel;
  const char* name;        // the template-id of the lists above
  int gx, gy, threads;     // grid and workgroup
  size_t lds;              // dynamic LDS bytes per workgroup
  int extra;               // the one further launch parameter some kernels take: k_acd_dw_m's NG (column-tile groups per row tile),
                           // k_dn_fcn_mid's / k_dn_fcn_bmid's np (1: the APReLU's fcn of the cell, 2: the DAM's, both paths); else 0
};
// the launches of one pass in order (the memsets in front of them are the model's)
struct BPass { int n; BLaunch e[BASELINE_MAX_LAUNCHES]; };
// ACDAE: forward 8 launches (table order); backward 16: rows 7 .. 0, each its data kernel, then its weight-gradient kernel
BPass acdae_pass(int L, int B, bool backward);
// DANet: 38 launches either way (4 per plain cell, 6 per DAM cell); forward in table order, backward rows 7 .. 0.  A training
// and an eval forward launch the same (the kernels take the mode as an argument).
BPass danet_pass(int leads, int L, int B, bool backward);

// the legal (leads, L): empty, or why a model of this configuration is refused (the text of ral_create's error)
std::string acdae_legal(const ral_config& c);
std::string danet_legal(const ral_config& c);
// a launcher was handed an entry it has no case for: a missing kernel is an error, never another kernel
[[noreturn]] void baseline_launch_missing(const char* launcher, const BLaunch& p);
