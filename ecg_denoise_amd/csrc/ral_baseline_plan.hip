// Baseline network dispatch (see ral_baseline_plan.hpp): the only place the shapes of ACDAE and DANet are written, and the only
// place that knows which kernel a row gets at a shape, with what grid and how much LDS.  Host code only.
#include <stdio.h>
#include <stdlib.h>
#include "ral_baseline_plan.hpp"

// ---- grid caps.  Every kernel of both networks loops over its windows, so a cap trades launch width against what a workgroup
// sets up once (zero halos, staged weights) and flushes once (atomics).
constexpr int WINDOW_GRID = 1024;      // a window per workgroup and iteration: every k_acd_* data kernel, DANet's conv / dam1 / out
                                       // and conv_b (DANet train step at batch 2048: 3.84 / 3.58 / 4.43 ms with 512 / 1024 / 2048)
constexpr int ACD_ENC_M_GRID = 512;    // k_acd_enc_fwd_m: a workgroup stages its 32-channel slice of the weights in LDS first
constexpr int DN_DESC_GRID = 256;      // descriptor-level kernels (k_dn_fcn_mid, k_dn_fcn_bmid): a wave per window, four windows of a
constexpr int DN_DESC_WINDOWS = 16;    //   wave in flight: 16 windows per workgroup and pass
constexpr int DN_ACT_GRID = 256;       // elementwise kernels (k_dn_act, k_dn_act_b):
constexpr int DN_ACT_WINDOWS = 4;      //   EW = 4 windows per workgroup and pass
constexpr int DN_FLUSH_GRID = 512;     // window-at-a-time backward kernels that end with column-sum flushes (k_dn_dam_b, k_dn_bn_b;
                                       // DANet train step at batch 2048: 2.33 / 2.23 / 2.26 / 2.44 ms with 1024 / 512 / 256 / 128)
constexpr int ACD_DW_WORKGROUPS = 2048;    // k_acd_dw: channel blocks x window splits aim at ~2048 workgroups per launch
constexpr int ACD_DW_M_WORKGROUPS = 512;   // k_acd_dw_m: (row tiles x column-tile groups) x window splits aim at ~512

// ---- the legal window lengths.  ACDAE: every level keeps float4 rows down to the bottleneck (L / 16 a multiple of 4), and
// decoder 0's forward tile at L = 2048 would be 172 576 bytes, past BASELINE_LDS_MAX.  DANet: four stride-2 levels.
constexpr int ACDAE_L_STEP = 64, ACDAE_L_MAX = 1024;
constexpr int DANET_L_STEP = 16, DANET_L_MIN = 32, DANET_L_MAX = 2048;

static std::string text(const char* fmt, int v) {
  char buf[160];
  snprintf(buf, sizeof(buf), fmt, v);
  return buf;
}
std::string acdae_legal(const ral_config& c) {
  if (c.leads != 2) return text("ACDAE has 2 input channels (got leads=%d)", c.leads);
  if (c.L <= 0 || c.L % ACDAE_L_STEP != 0 || c.L > ACDAE_L_MAX) return text("ACDAE: L must be a multiple of 64 and <= 1024 (got %d)", c.L);
  return "";
}
std::string danet_legal(const ral_config& c) {
  if (c.leads != 2) return text("DANet: the last decoder cell has 2 output channels, so leads must be 2 (got %d)", c.leads);
  if (c.L < DANET_L_MIN || c.L % DANET_L_STEP != 0 || c.L > DANET_L_MAX) return text("DANet: L must be a multiple of 16 in [32, 2048], got %d", c.L);
  return "";
}

// ---- the networks
const AcdaeLayer* acdae_layers() {   // reference model/ACDAE.py: channels 2 -> 16 -> 32 -> 64 -> 128 -> 64 -> 32 -> 16 -> 2
  static const AcdaeLayer tab[BASELINE_LAYERS] = {
      /* cin cout ks convt in out skip */
      {2, 16, 13, 0, 0, 1, BL_NONE},
      {16, 32, 7, 0, 1, 2, BL_NONE},
      {32, 64, 7, 0, 2, 3, BL_NONE},
      {64, 128, 7, 0, 3, 4, BL_NONE},
      {128, 64, 7, 1, 4, 3, 2},
      {64, 32, 7, 1, 3, 2, 1},
      {32, 16, 7, 1, 2, 1, 0},
      {16, 2, 13, 1, 1, 0, BL_NONE},
  };
  return tab;
}
const DanetCell* danet_cells(int leads) {   // reference model/DAM.py::Seq2Seq2: leads -> 4 -> 8 -> 16 -> 32 -> 16 -> 8 -> 4 -> 2
  static const DanetCell tab[BASELINE_LAYERS] = {
      /* cin c k p tr in out in1 dam */
      {2, 4, 17, 8, 0, 0, 1, BL_NONE, 0},
      {4, 8, 17, 8, 0, 1, 2, BL_NONE, 0},
      {8, 16, 3, 1, 0, 2, 3, BL_NONE, 0},
      {16, 32, 3, 1, 0, 3, 4, BL_NONE, 0},
      {32, 16, 4, 1, 1, 4, 3, BL_NONE, 1},
      {16, 8, 4, 1, 1, 3, 2, 2, 1},
      {8, 4, 18, 8, 1, 2, 1, 1, 1},
      {4, 2, 18, 8, 1, 1, 0, 0, 0},
  };
  if (leads != tab[0].cin) { fprintf(stderr, "ral_baseline_plan: DANet has no table for leads=%d\n", leads); abort(); }
  return tab;
}

// ---- entries
using K = BKernel;
static const char* const NAMES[] = {
#define X(e, name) name,
    ACDAE_KERNELS(X) DANET_KERNELS(X)
#undef X
};
void baseline_launch_missing(const char* launcher, const BLaunch& p) {
  fprintf(stderr, "%s: no launch code for plan entry %d (%s) of row %d\n", launcher, (int)p.kernel, p.name ? p.name : "", p.layer);
  abort();
}
[[noreturn]] static void no_instance(const char* family, int k, int transposed) {
  fprintf(stderr, "ral_baseline_plan: no instance of %s for %d taps%s\n", family, k, transposed ? ", transposed" : "");
  abort();
}
static void add(BPass& P, int layer, K k, int gx, int gy, size_t lds, int extra = 0) {
  if (P.n >= BASELINE_MAX_LAUNCHES || lds > BASELINE_LDS_MAX || gx < 1 || gy < 1) {
    fprintf(stderr, "ral_baseline_plan: row %d, %s: entry %d, grid (%d, %d), %zu bytes of LDS cannot be launched\n", layer, NAMES[(int)k], P.n, gx, gy, lds);
    abort();
  }
  P.e[P.n++] = BLaunch{layer, k, NAMES[(int)k], gx, gy, BASELINE_THREADS, lds, extra};
}
static int at_most(int v, int cap) { return v < cap ? v : cap; }
static int ceil_div(int a, int b) { return (a + b - 1) / b; }
// window splits of a weight-gradient launch: `target` workgroups over `blocks` channel blocks, at least one, at most a window each
static int dw_splits(int target, int blocks, int B) { return at_most(target / blocks < 1 ? 1 : target / blocks, B); }

// ---- ACDAE: dynamic LDS of the kernel families (bytes; each follows the carve-up at the head of its kernel in ral_acdae.hip)
static size_t acd_rows(int c, int l) { return (size_t)c * (l + 2 * ACDAE_HALO); }                 // c rows of l values with a zero halo
static size_t acd_enc_fwd_lds(const AcdaeLayer& r, int lin) { return acd_rows(r.cin, lin) * sizeof(float); }   // xs
static size_t acd_enc_fwd_m_lds(const AcdaeLayer& r, int lin) {                                    // xs | ws: 32 output channels x (cin, tap)
  return (acd_rows(r.cin, lin) + (size_t)32 * r.cin * r.ks) * sizeof(float);
}
static size_t acd_dec_fwd_lds(const AcdaeLayer& r, int lin) {                                      // xs | ts | as | ms | ss
  return (acd_rows(r.cin, lin) + (size_t)r.cout * lin * 3 + 2 * r.cout + 8) * sizeof(float);
}
static size_t acd_dec_bwd_lds(const AcdaeLayer& r, int lin) {                                      // du | dts | ms | dz | dm | ge
  return ((size_t)r.cout * lin * 2 + acd_rows(r.cout, lin) + 3 * r.cout + 16) * sizeof(float);
}
static size_t acd_enc_bwd_lds(const AcdaeLayer& r, int lin) { return acd_rows(r.cout, lin) * sizeof(float); }   // dcs
static size_t acd_dw_lds(int l) { return ((size_t)8 * l + acd_rows(8, l)) * sizeof(float); }      // ys: 8 rows | xs: 8 haloed rows
static size_t acd_dw_m_lds(const AcdaeLayer& r, int l) {                                           // ys: 16 rows | xs: cxr haloed rows,
  const int cxr = at_most((16 * 16) / r.ks + 2, r.cin);                                            // the input channels the 16 column
  return ((size_t)16 * l + acd_rows(cxr, l)) * sizeof(float);                                      // tiles of a group touch
}

static void acd_forward(BPass& P, int li, const AcdaeLayer& r, int lin, int B) {
  const int grid = at_most(B, WINDOW_GRID);
  if (r.convt) {
    switch (r.ks) {
      case 7: return add(P, li, K::ACD_DEC_FWD_7, grid, 1, acd_dec_fwd_lds(r, lin));
      case 13: return add(P, li, K::ACD_DEC_FWD_13, grid, 1, acd_dec_fwd_lds(r, lin));
    }
    no_instance("k_acd_dec_fwd", r.ks, 1);
  }
  // first match: 1. a 13-tap row has the direct form only;
  if (r.ks == 13) return add(P, li, K::ACD_ENC_FWD_13, grid, 1, acd_enc_fwd_lds(r, lin));
  if (r.ks != 7) no_instance("k_acd_enc_fwd", r.ks, 0);
  // 2. the convolution on the fp32 MFMA: K = (input channel, tap) pairs in steps of 16 (cin >= 16), 32 output channels per
  // workgroup (blockIdx.y), whole 16-position tiles - encoder 3 misses it when L is not a multiple of 128;
  if (r.cin >= 16 && r.cout % 32 == 0 && lin % 16 == 0)
    return add(P, li, K::ACD_ENC_FWD_M_7, at_most(B, ACD_ENC_M_GRID), r.cout / 32, acd_enc_fwd_m_lds(r, lin));
  // 3. the direct form
  add(P, li, K::ACD_ENC_FWD_7, grid, 1, acd_enc_fwd_lds(r, lin));
}
static void acd_backward_data(BPass& P, int li, const AcdaeLayer& r, int lin, int B) {
  const int grid = at_most(B, WINDOW_GRID);
  switch (r.convt * 100 + r.ks) {
    case 107: return add(P, li, K::ACD_DEC_BWD_7, grid, 1, acd_dec_bwd_lds(r, lin));
    case 113: return add(P, li, K::ACD_DEC_BWD_13, grid, 1, acd_dec_bwd_lds(r, lin));
    case 13: return add(P, li, K::ACD_ENC_BWD_13, grid, 1, acd_enc_bwd_lds(r, lin));
    case 7: return add(P, li, K::ACD_ENC_BWD_7, grid, 1, acd_enc_bwd_lds(r, lin));
  }
  no_instance(r.convt ? "k_acd_dec_bwd" : "k_acd_enc_bwd", r.ks, r.convt);
}
// weight gradient of a row: Y = the gradient at its conv output (cout rows), X = its input (cin rows), both of length lin
static void acd_backward_dw(BPass& P, int li, const AcdaeLayer& r, int lin, int B) {
  // the fp32-MFMA GEMM owns 16 output channels per row tile: every row but the 2-channel output layer
  if (r.cout >= 16) {
    const int NT = ceil_div(r.cin * r.ks, 16), NG = ceil_div(NT, 16), MT = ceil_div(r.cout, 16);
    const int sp = dw_splits(ACD_DW_M_WORKGROUPS, MT * NG, B);
    switch (r.convt * 100 + r.ks) {
      case 13: return add(P, li, K::ACD_DW_M_13_C, MT * NG, sp, acd_dw_m_lds(r, lin), NG);
      case 7: return add(P, li, K::ACD_DW_M_7_C, MT * NG, sp, acd_dw_m_lds(r, lin), NG);
      case 107: return add(P, li, K::ACD_DW_M_7_T, MT * NG, sp, acd_dw_m_lds(r, lin), NG);
    }
    no_instance("k_acd_dw_m", r.ks, r.convt);
  }
  const int nblk = ceil_div(r.cout, 8) * ceil_div(r.cin, 8);
  if (r.convt && r.ks == 13) return add(P, li, K::ACD_DW_13_T, nblk, dw_splits(ACD_DW_WORKGROUPS, nblk, B), acd_dw_lds(lin));
  no_instance("k_acd_dw", r.ks, r.convt);
}

BPass acdae_pass(int L, int B, bool backward) {
  const AcdaeLayer* const tab = acdae_layers();
  BPass P;
  P.n = 0;
  if (!backward) {
    for (int li = 0; li < BASELINE_LAYERS; ++li) acd_forward(P, li, tab[li], L >> tab[li].in_shift, B);
    return P;
  }
  for (int li = BASELINE_LAYERS - 1; li >= 0; --li) {
    acd_backward_data(P, li, tab[li], L >> tab[li].in_shift, B);
    acd_backward_dw(P, li, tab[li], L >> tab[li].in_shift, B);
  }
  return P;
}

// ---- DANet: dynamic LDS of the kernel families (bytes; each follows the carve-up at the head of its kernel in ral_danet.hip).
// The APReLU fcn of a cell is Linear(2c, 2c) -> Linear(2c, c), the DAM fcn Linear(c, c) -> Linear(c, c).
static size_t dn_rows(int c, int l) { return (size_t)c * (l + 2 * DANET_HALO); }
static size_t dn_conv_lds(const DanetCell& g, int lin, int lout) {                                 // xs | zs | ds
  return (dn_rows(g.cin, lin) + (size_t)g.c * lout + 2 * g.c) * sizeof(float);
}
static size_t dn_dam1_lds(const DanetCell& g, int lout) { return (size_t)g.c * lout * sizeof(float); }                   // xs
static size_t dn_out_lds(const DanetCell& g, int lout) { return ((size_t)g.c * lout + lout) * sizeof(float); }           // xs | ss
static size_t dn_dam_b_lds(const DanetCell& g, int lout) { return ((size_t)2 * g.c * lout + 3 * lout) * sizeof(float); } // xs | ts | ss | dsl | am
static size_t dn_fcn_bmid_lds(int dh, int dout) { return ((size_t)dout * dh + dout) * sizeof(float); }                   // aw3 | ab3
static size_t dn_bn_b_lds(const DanetCell& g, int lout) {                                          // xs | aw0 | ab0 (a DAM cell's fcn)
  return ((size_t)g.c * lout + (g.dam ? (size_t)g.c * g.c + g.c : 0)) * sizeof(float);
}
static size_t dn_conv_b_lds(const DanetCell& g, int lin, int lout) {                               // xs | dzs | aw | ab | aw0 | ab0
  return (dn_rows(g.cin, lin) + dn_rows(g.c, lout) + (size_t)g.c * g.cin * g.k + g.c + (size_t)2 * g.c * 2 * g.c + 2 * g.c) * sizeof(float);
}
static K dn_conv_instance(const DanetCell& g, bool backward) {
  switch (g.tr * 100 + g.k) {
    case 17: return backward ? K::DN_CONV_B_17_C : K::DN_CONV_17_C;
    case 3: return backward ? K::DN_CONV_B_3_C : K::DN_CONV_3_C;
    case 104: return backward ? K::DN_CONV_B_4_T : K::DN_CONV_4_T;
    case 118: return backward ? K::DN_CONV_B_18_T : K::DN_CONV_18_T;
  }
  no_instance(backward ? "k_dn_conv_b" : "k_dn_conv", g.k, g.tr);
}

BPass danet_pass(int leads, int L, int B, bool backward) {
  const DanetCell* const tab = danet_cells(leads);
  BPass P;
  P.n = 0;
  const int grid = at_most(B, WINDOW_GRID), gridw = at_most(B, DN_FLUSH_GRID);
  const int gridd = at_most(ceil_div(B, DN_DESC_WINDOWS), DN_DESC_GRID), grida = at_most(ceil_div(B, DN_ACT_WINDOWS), DN_ACT_GRID);
  for (int n = 0; n < BASELINE_LAYERS; ++n) {
    const int i = backward ? BASELINE_LAYERS - 1 - n : n;
    const DanetCell& g = tab[i];
    const int lin = L >> g.in_shift, lout = L >> g.out_shift;
    const bool v4 = lout % 4 == 0;      // the elementwise kernels move 16-byte items of one channel row
    if (!backward) {
      add(P, i, dn_conv_instance(g, false), grid, 1, dn_conv_lds(g, lin, lout));
      add(P, i, K::DN_FCN_MID, gridd, 1, 0, 1);
      add(P, i, v4 ? K::DN_ACT_4 : K::DN_ACT_1, grida, 1, 0);
      if (g.dam) {
        add(P, i, K::DN_DAM1, grid, 1, dn_dam1_lds(g, lout));
        add(P, i, K::DN_FCN_MID, gridd, 1, 0, 2);
      }
      add(P, i, K::DN_OUT, grid, 1, dn_out_lds(g, lout));
    } else {
      if (g.dam) {
        add(P, i, K::DN_DAM_B, gridw, 1, dn_dam_b_lds(g, lout));
        add(P, i, K::DN_FCN_BMID, gridd, 1, dn_fcn_bmid_lds(g.c, g.c), 2);
      }
      add(P, i, K::DN_BN_B, gridw, 1, dn_bn_b_lds(g, lout));
      add(P, i, v4 ? K::DN_ACT_B_4 : K::DN_ACT_B_1, grida, 1, 0);
      add(P, i, K::DN_FCN_BMID, gridd, 1, dn_fcn_bmid_lds(2 * g.c, g.c), 1);
      add(P, i, dn_conv_instance(g, true), grid, 1, dn_conv_b_lds(g, lin, lout));
    }
  }
  return P;
}
