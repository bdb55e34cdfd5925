// U-Net stage dispatch (see ral_unet_plan.hpp): the only place the network's shape is written, the only place that reads
// UNET_EVAL_GRID and UNET_FUSED, and the only place that knows which kernel a stage gets at a shape.  Host code only.
#include <stdio.h>
#include <stdlib.h>
#include "ral_device.hpp"
#include "ral_unet_plan.hpp"

// The switches (ral_global_option):
//   UNET_EVAL_GRID  most workgroups of a stage of the stage-by-stage eval forward (default 512; at batch 2048: 173 / 158 / 177 us
//                   with 256 / 512 / 1024 workgroups); latched at its first read
//   UNET_FUSED      default of a model's "unet_fused" option: the eval forward as one kernel where it applies (default 1);
//                   read when a model is created
static int sw_eval_grid() { static const int v = (int)ral_knob("UNET_EVAL_GRID", 512); return v; }
bool unet_fused_default() { return ral_knob("UNET_FUSED", 1) != 0; }

// Grid caps.  Training forward at batch 2048: 0.31 / 0.27 / 0.29 / 0.41 ms with 256 / 512 / 1024 / 2048 workgroups.  Backward:
// every workgroup ends with ~2 000 global atomics (its share of dW, db and the BatchNorm-backward sums) or a scratch row; the
// chip retires ~75 atomics per ns, so 1024 workgroups spend 30 us per launch on them alone - the train step at batch 2048 with
// 1024 / 512 / 384 workgroups: 1.23 / 1.08 / 1.12 ms.  A backward workgroup owns one scratch row of the fold: the workspace
// keeps min(max_batch, UNET_PART_ROWS) of them and B <= max_batch, so min(B, UNET_BWD_GRID) rows always exist.
constexpr int UNET_FWD_GRID = 512, UNET_BWD_GRID = 512;
static_assert(UNET_BWD_GRID <= UNET_PART_ROWS, "a backward workgroup needs a scratch row of its own");
constexpr int UNET_FWD_WP = 4, UNET_BWD_WP = 2;   // most windows per pass of the specialised kernels
constexpr size_t UNET_WP_LDS = 80 * 1024;         // more windows per pass only while two workgroups fit a CU

// ---- the network (reference model/UNet.py): encoder Conv1d(k3, s2, p1) -> BN -> LeakyReLU; bottleneck.0 1x1 conv -> LeakyReLU
// -> BN, bottleneck.3 k3 conv -> LeakyReLU -> BN, bottleneck.6 1x1 conv + x (x = lrelu(BN3(z3))); decoder ConvTranspose1d(k4,
// s2, p1) -> BN -> [LeakyReLU], + the encoder feature of its length, both applied by the consumer.
// A gradient of an encoder tensor is first WRITTEN by its decoder-side consumer (skip / residual, accumulate 0: the backward
// runs stages 10 .. 0) and later ACCUMULATED by the next encoder / bottleneck stage (accumulate 1).
#define NO {UZ_NONE, ACT_NONE, 0}
#define UNET_TABLE(leads)                                                                                          \
  { /* cin cout ks mode          s  p  type  post bn  a                   b                   r            shift */ \
    {leads, 4, 3, UMODE_CONV,       2, 1, TY_ZBN,   0, 0,  {UZ_X, ACT_NONE, 0}, NO,                 NO,                 1}, \
    {4, 8, 3, UMODE_CONV,           2, 1, TY_ZBN,   0, 1,  {0, ACT_LRELU, 1},   NO,                 NO,                 2}, \
    {8, 16, 3, UMODE_CONV,          2, 1, TY_ZBN,   0, 2,  {1, ACT_LRELU, 1},   NO,                 NO,                 3}, \
    {16, 32, 3, UMODE_CONV,         2, 1, TY_ZBN,   0, 3,  {2, ACT_LRELU, 1},   NO,                 NO,                 4}, \
    {32, 32, 1, UMODE_BOTTLENECK,   1, 0, TY_ABN,   1, 4,  {3, ACT_LRELU, 1},   NO,                 NO,                 4}, \
    {32, 32, 3, UMODE_BOTTLENECK,   1, 1, TY_ABN,   1, 5,  {4, ACT_NONE, 0},    NO,                 NO,                 4}, \
    {32, 32, 1, UMODE_BOTTLENECK,   1, 0, TY_PLAIN, 0, -1, {5, ACT_NONE, 0},    NO,                 {3, ACT_LRELU, 0},  4}, \
    {32, 16, 4, UMODE_CONVT,        1, 0, TY_ZBN,   0, 6,  {6, ACT_NONE, 0},    NO,                 NO,                 3}, \
    {16, 8, 4, UMODE_CONVT,         1, 0, TY_ZBN,   0, 7,  {7, ACT_LRELU, 0},   {2, ACT_LRELU, 0},  NO,                 2}, \
    {8, 4, 4, UMODE_CONVT,          1, 0, TY_ZBN,   0, 8,  {8, ACT_LRELU, 0},   {1, ACT_LRELU, 0},  NO,                 1}, \
    {4, leads, 4, UMODE_CONVT,      1, 0, TY_ZBN,   0, 9,  {9, ACT_LRELU, 0},   {0, ACT_LRELU, 0},  NO,                 0}, \
  }
const UStageGeom* unet_stages(int leads) {
  static const UStageGeom one[UNET_STAGES] = UNET_TABLE(1), two[UNET_STAGES] = UNET_TABLE(2);
  return leads == 1 ? one : two;
}
#undef UNET_TABLE
#undef NO

static const char* const UNET_NAMES[] = {
#define X(e, name) name,
  UNET_KERNELS(X)
#undef X
};
using K = UKernel;
static UStageLaunch launch_of(K k, int threads, int grid, int wp, size_t lds) {
  return UStageLaunch{k, k == K::NONE ? "" : UNET_NAMES[(int)k], threads, grid, wp, lds};
}
void unet_launch_missing(const char* launcher, const UStageLaunch& p) {
  fprintf(stderr, "%s: no launch code for plan entry %d (%s)\n", launcher, (int)p.kernel, p.name ? p.name : "");
  abort();
}
// the specialised instance of a stage's <CIN, COUT, KS, MODE>; an instance that is not built is an error, never another kernel
static K t_instance(const UStageGeom& g, bool backward) {
#define T(ci, co, k, md) \
  if (g.cin == ci && g.cout == co && g.ks == k && g.mode == md) return backward ? K::BWD_T_##ci##_##co##_##k##_##md : K::FWD_T_##ci##_##co##_##k##_##md;
  UNET_T_INSTANCES(T)
#undef T
  fprintf(stderr, "ral_unet_plan: no instance of k_unet_%s_t<%d, %d, %d, %d>\n", backward ? "bwd" : "fwd", g.cin, g.cout, g.ks, g.mode);
  abort();
}

// ---- dynamic LDS of the four stage kernels (floats of their tiles; the formulas follow the kernels' carve-up in ral_unet.hip)
static size_t fwd_lds(const UStageGeom& g, int lin) {   // k_unet_fwd: one window per pass
  return ((size_t)g.cin * lin + (size_t)g.cin * g.cout * g.ks + UNET_MAXC + 12 * UNET_MAXC + 2 * UNET_MAXC + 8) * sizeof(float);
}
static size_t bwd_lds(const UStageGeom& g, int lin, int lout) {   // k_unet_bwd
  return ((size_t)2 * g.cin * lin + (size_t)g.cout * lout + (size_t)g.cin * g.cout * g.ks + 16 * UNET_MAXC + 6 * UNET_MAXC + 7 * UNET_MAXC + 8) * sizeof(float);
}
// k_unet_fwd_t: WP input tiles, WP output tiles when a residual is added to them, the weights (rows padded by up to 4 floats),
// the column sums as doubles
static size_t fwd_t_lds(const UStageGeom& g, int lin, int lout, int WP) {
  return ((size_t)WP * g.cin * (lin + 8) + (g.r.z != UZ_NONE ? (size_t)WP * g.cout * lout : 0) + (size_t)g.cout * (g.cin * g.ks + 4) + UNET_MAXC +
          12 * UNET_MAXC + 4 * UNET_MAXC + 8) * sizeof(float);
}
// k_unet_bwd_t: the input tile, its gradient tile when the stage wants one (every stage but 0: x has no gradient), a third tile
// for the skip operand or for the gradient the stage accumulates into; weights twice (rows padded), 7 UNET_MAXC doubles of sums
static size_t bwd_t_lds(const UStageGeom& g, int lin, int lout, int WP) {
  const bool want_din = g.a.z != UZ_X, third = g.b.z != UZ_NONE || (want_din && g.a.accumulate);
  return ((size_t)WP * g.cin * (lin + 8) * (1 + (want_din ? 1 : 0) + (third ? 1 : 0)) + (size_t)WP * g.cout * (lout + 10) +
          (size_t)2 * g.cin * g.cout * g.ks + 4 * g.cin + 31 * UNET_MAXC + 12) * sizeof(float);
}

UStageLaunch unet_stage_plan(int leads, int L, int B, bool training, bool backward, int si) {
  const UStageGeom* const tab = unet_stages(leads);
  const UStageGeom& g = tab[si];
  const int lin = unet_len(tab, g.a.z, L), lout = unet_len(tab, si, L);
  const int cap = backward ? UNET_BWD_GRID : (training ? UNET_FWD_GRID : sw_eval_grid());
  const int grid = B < cap ? B : cap;
  // the specialised kernels move float4s: both lengths must be multiples of 4
  if (lin % 4 || lout % 4)
    return backward ? launch_of(K::BWD, 256, grid, 1, bwd_lds(g, lin, lout)) : launch_of(K::FWD, 256, grid, 1, fwd_lds(g, lin));
  // windows per pass: all of a workgroup's windows at once up to the direction's most - fewer while the tiles of a pass would
  // not leave room for two workgroups per CU (long windows: at L = 2048 the 32-channel stages take 64 KB at WP = 2 already)
  int WP = (B + grid - 1) / grid;
  if (WP < 1) WP = 1;
  if (backward) {
    if (WP > UNET_BWD_WP) WP = UNET_BWD_WP;
    while (WP > 1 && bwd_t_lds(g, lin, lout, WP) > UNET_WP_LDS) --WP;
    // (the grid stays: its workgroups are the fold's partial rows, the same for every stage of the pass)
    return launch_of(t_instance(g, true), UNET_BWD_THREADS, grid, WP, bwd_t_lds(g, lin, lout, WP));
  }
  if (WP > UNET_FWD_WP) WP = UNET_FWD_WP;
  while (WP > 1 && fwd_t_lds(g, lin, lout, WP) > UNET_WP_LDS) --WP;
  const int nwg = (B + WP - 1) / WP;   // (the kernel loops over passes)
  return launch_of(t_instance(g, false), UNET_FWD_THREADS, nwg < grid ? nwg : grid, WP, fwd_t_lds(g, lin, lout, WP));
}

// LDS floats of the fused inference kernel's tensors of one window (k_unet_infer's carve-up)
static size_t uinf_lds_floats(int L) {
  const int N1 = L / 2, N2 = L / 4, N3 = L / 8, N4 = L / 16;
  return (size_t)4 * (N1 + 8) + (size_t)N4 * 100 + (size_t)N2 * 8 + (size_t)N3 * 16 + (size_t)(N4 + 1) * 68 + (size_t)N4 * 36 * 2 +
         (size_t)(N3 + 1) * 36 + 288 + UINF_COEFF_FLOATS;
}

UPassPlan unet_pass_plan(int leads, int L, bool train_cfg, bool fused_option) {
  UPassPlan p;
  // every level's length is a multiple of 4 - every backward stage runs its specialised kernel - iff L is a multiple of 64
  p.fold = train_cfg && L % 64 == 0;
  // the fused eval forward: windows of 256 / 512 / 768 / 1024 samples (its GEMM layers need whole 16-row tiles at the deepest
  // level and the window's tensors must fit LDS); every other length, and training, runs stage by stage
  p.fused_eval = fused_option && L % 256 == 0 && L <= 1024;
  p.fused = p.fused_eval ? launch_of(leads == 1 ? K::INFER_1 : K::INFER_2, 256, 0, 1, uinf_lds_floats(L) * sizeof(float)) : launch_of(K::NONE, 0, 0, 0, 0);
  return p;
}
