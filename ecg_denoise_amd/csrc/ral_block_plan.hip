// Linear-layer dispatch (see ral_block_plan.hpp): the only place that reads MLP_FWD_W, MLP_BWD_W, MLP_BWD_W_F16 and FUSE_DW
// and the only place that knows which kernel a block's Linear layers get at a shape.  Host code only.  The LDS formulas it
// calls sit beside the kernels they describe (ral_kernels.hpp).
#include <stdio.h>
#include <stdlib.h>
#include "ral_kernels.hpp"

// The switches (ral_global_option; each latched at its first read):
//   MLP_FWD_W      strip forward of the narrow levels: 0 never, 1 fp32 strips at C = 16 only, 2 fp32 strips at every narrow
//                  width, 3 (default) f16 strips at every narrow width where the model allows them, else fp32 strips at C = 16
//                  (the measurements: ral_mlpw.hip)
//   MLP_BWD_W      strip backward: 0 never, 1 C = 16 only, 2 C = 8 and 16, 3 (default) C = 32 too (k_mlp_bwd_w2)
//   MLP_BWD_W_F16  C = 32 strip backward: the channel products as fp16 pairs where the model allows them (default 1)
//   FUSE_DW        widest level whose MLP backward fuses the fc1 / fc2 weight gradients and re-computes u_pre (default 32; 0
//                  disables it, 8 / 16 narrow it).  Measured at batch 2048: none 102.8k, C <= 8 103.8k, C <= 16 105.5k,
//                  C <= 32 105.8k windows/s
#define BLOCK_SWITCH(fn, name, dflt) \
  static int fn() { static const int v = (int)ral_knob(name, dflt); return v; }
BLOCK_SWITCH(sw_mlp_fwd_w, "MLP_FWD_W", 3)
BLOCK_SWITCH(sw_mlp_bwd_w, "MLP_BWD_W", 3)
BLOCK_SWITCH(sw_mlp_bwd_w_f16, "MLP_BWD_W_F16", 1)
BLOCK_SWITCH(sw_fuse_dw, "FUSE_DW", 32)
#undef BLOCK_SWITCH

static const char* const BLOCK_NAMES[] = {
#define X(e, name) name,
  BLOCK_KERNELS(X)
#undef X
};
using K = BlockKernel;
static BlockLaunch launch_of(K k, int threads, size_t lds, int chunks = 0, bool split = false) {
  return BlockLaunch{k, k == K::NONE ? "" : BLOCK_NAMES[(int)k], threads, lds, chunks, split};
}
// an instance that is not built: only a shape no level of a model has can ask for one (tests/test_block_plan_cpu.py sweeps the
// legal space and ral_block_plan refuses the rest); a missing kernel is an error, never another kernel
[[noreturn]] static void no_instance(const char* family, int C, int n) {
  fprintf(stderr, "ral_block_plan: no instance of %s for C=%d, %d\n", family, C, n);
  abort();
}
void block_launch_missing(const char* launcher, const BlockLaunch& p) {
  fprintf(stderr, "%s: no launch code for plan entry %d (%s)\n", launcher, (int)p.kernel, p.name ? p.name : "");
  abort();
}
// enumerator of a family's instance: <C> or <C, n>
#define BY_C(fn, family, ...) \
  static K fn(int C) { switch (C) { __VA_ARGS__ } no_instance(family, C, 0); }
#define BY_CN(fn, family, ...) \
  static K fn(int C, int n) { switch (C * 16 + n) { __VA_ARGS__ } no_instance(family, C, n); }
#define E(prefix, c) case c: return K::prefix##_##c;
#define EN(prefix, c, n) case c * 16 + n: return K::prefix##_##c##_##n;
BY_C(k_qkv_fwd, "k_qkv_fwd", E(QKV_FWD, 8) E(QKV_FWD, 16) E(QKV_FWD, 32) E(QKV_FWD, 64) E(QKV_FWD, 128))
BY_C(k_qkv_fwd_ws, "k_qkv_fwd_ws", E(QKV_FWD_WS, 64) E(QKV_FWD_WS, 128))
BY_C(k_qkv_fwd_h, "k_qkv_fwd_h", E(QKV_FWD_H, 32) E(QKV_FWD_H, 64))
BY_CN(k_mlp_fwd, "k_mlp_fwd",
      EN(MLP_FWD, 8, 1) EN(MLP_FWD, 8, 2) EN(MLP_FWD, 8, 4) EN(MLP_FWD, 16, 1) EN(MLP_FWD, 16, 2) EN(MLP_FWD, 16, 4)
      EN(MLP_FWD, 32, 1) EN(MLP_FWD, 32, 2) EN(MLP_FWD, 32, 4) EN(MLP_FWD, 64, 1) EN(MLP_FWD, 64, 2) EN(MLP_FWD, 64, 4)
      EN(MLP_FWD, 128, 1) EN(MLP_FWD, 128, 2) EN(MLP_FWD, 128, 4))
BY_CN(k_mlp_fwd_h, "k_mlp_fwd_h",
      EN(MLP_FWD_H, 32, 1) EN(MLP_FWD_H, 32, 2) EN(MLP_FWD_H, 32, 4) EN(MLP_FWD_H, 64, 1) EN(MLP_FWD_H, 64, 8)
      EN(MLP_FWD_H, 128, 4) EN(MLP_FWD_H, 128, 8))
BY_C(k_mlp_fwd_w, "k_mlp_fwd_w", E(MLP_FWD_W, 8) E(MLP_FWD_W, 16) E(MLP_FWD_W, 32))
BY_C(k_mlp_fwd_wh, "k_mlp_fwd_wh", E(MLP_FWD_WH, 8) E(MLP_FWD_WH, 16) E(MLP_FWD_WH, 32))
BY_CN(k_mlp_bwd, "k_mlp_bwd",
      EN(MLP_BWD, 8, 1) EN(MLP_BWD, 8, 2) EN(MLP_BWD, 8, 4) EN(MLP_BWD, 16, 1) EN(MLP_BWD, 16, 2) EN(MLP_BWD, 16, 4)
      EN(MLP_BWD, 32, 1) EN(MLP_BWD, 32, 2) EN(MLP_BWD, 32, 4) EN(MLP_BWD, 64, 1) EN(MLP_BWD, 64, 2) EN(MLP_BWD, 64, 4)
      EN(MLP_BWD, 128, 1) EN(MLP_BWD, 128, 2) EN(MLP_BWD, 128, 4))
BY_CN(k_mlp_bwd_s, "k_mlp_bwd_s",
      EN(MLP_BWD_S, 8, 1) EN(MLP_BWD_S, 8, 2) EN(MLP_BWD_S, 8, 4) EN(MLP_BWD_S, 16, 1) EN(MLP_BWD_S, 16, 2) EN(MLP_BWD_S, 32, 1) EN(MLP_BWD_S, 32, 2))
BY_CN(k_mlp_bwd_h4, "k_mlp_bwd_h (four waves)", EN(MLP_BWD_H4, 32, 4) EN(MLP_BWD_H4, 64, 4) EN(MLP_BWD_H4, 128, 4))
BY_CN(k_mlp_bwd_h8, "k_mlp_bwd_h (eight waves)", EN(MLP_BWD_H8, 32, 1) EN(MLP_BWD_H8, 64, 1))
BY_C(k_qkv_bwd, "k_qkv_bwd", E(QKV_BWD, 8) E(QKV_BWD, 16) E(QKV_BWD, 32) E(QKV_BWD, 64) E(QKV_BWD, 128))
BY_C(k_qkv_bwd_h, "k_qkv_bwd_h", E(QKV_BWD_H, 32) E(QKV_BWD_H, 64) E(QKV_BWD_H, 128))
#define DW_E(prod) \
  BY_C(k_dw_##prod, "k_dw", E(DW_##prod, 8) E(DW_##prod, 16) E(DW_##prod, 32) E(DW_##prod, 64) E(DW_##prod, 128)) \
  static K k_dw_##prod##_h(int C) { switch (C) { case 32: return K::DW_##prod##_32_H; case 64: return K::DW_##prod##_64_H; case 128: return K::DW_##prod##_128_H; } \
    no_instance("k_dw (split)", C, 0); }
DW_E(FC2) DW_E(FC1) DW_E(PROJ) DW_E(QKV)
#undef DW_E
#undef E
#undef EN
#undef BY_C
#undef BY_CN

// LDS budget of an fp32 MLP workgroup (bytes; fewer bytes = more hidden chunks but more co-resident workgroups per CU)
static constexpr size_t MLP_LDS = 78000;

// ---- does the narrow-level backward with fused weight gradients (k_mlp_bwd_s and the strips) take (C, N)?  When the window
// length gives each wave a whole number (1, 2, 4 or 8) of dg token tiles and the tiles fit 80 KB.  Everything else about the MLP
// follows from this one predicate: the forward does not store u_pre for such blocks, the backward re-computes it.
static int fused_tw(int C, int N) {   // token tiles per wave of k_mlp_bwd_s, or 0: not fused
  if (C > 32 || C > sw_fuse_dw()) return 0;
  const int MT = C >= 16 ? C / 16 : 1;
  if ((N * MT) % 128 != 0) return 0;
  const int tw = N * MT / 128;
  if (tw != 1 && tw != 2 && tw != 4 && tw != 8) return 0;
  return mlp_bwd_s_lds(C, N) <= 80 * 1024 ? tw : 0;
}

// ---- split-operand MLP backward: the hidden-chunk count that gives the fc2^T phase exactly one 32 x 32 unit per wave and fits
// the LDS budget: > 0 four waves, < 0 eight waves, 0 none.
// Threads of a k_mlp_bwd_h workgroup: 256: four waves, 37-39 KB of LDS, 150 registers per lane, three workgroups per CU; 512:
// eight waves, 75-78 KB, 128 registers (28-68 bytes of scratch), two per CU - the shapes the four-wave form does not cover.
// Measured at batch 2048 on the shapes both take: the four-wave form is the SLOWER kernel on an empty GPU (`mlp_bwd`
// 2.66 -> 2.76 ms per step serialised) and the faster training step (12.98 -> 12.88 ms, 13.57 -> 13.42 on a slower box;
// interleaved A/B, three rounds each).  What it changes beside the other lane's kernels and the 76 KB weight-gradient
// workgroups: half the LDS and half the waves per workgroup, no spills, and no dg read-modify-write through LDS per hidden chunk
// (k_qkv_bwd_h with half the LDS and waves alone - half-window work items - did not move the step).
static int mlp_bwd_h_nch(int C, int N) {
  if (!block_has_planes(C) || N % 32 != 0) return 0;
  // four waves: N C = 4096, one 32 x 32 unit of dg per wave; HC + 8 >= C + 4: the dg tile fits the chunk's bytes
  for (int nch = 1; nch <= 4; nch *= 2)
    if (N * C == 4096 && 4 * C / nch >= C && (4 * C / nch / 32) * (N / 32) == 4 && mlp_bwd_h_lds(C, N, nch, true) <= 54400) return nch;
  for (int nch = 1; nch <= 4; nch *= 2)   // eight waves
    if ((4 * C / nch / 32) * (N / 32) == 8 && mlp_bwd_h_lds(C, N, nch, false) <= 79872) return -nch;
  return 0;
}
static bool qkv_bwd_h_takes(int C, int N) { return block_has_planes(C) && N % 32 == 0 && N * 3 * C / 4 <= 6 * 512; }

// ---- the four launches of the chain, each a first-match table (DESIGN.md has them row by row)
static BlockLaunch plan_qkv_fwd(const BlockShape& sh) {
  const int C = sh.C, N = sh.N;
  if (sh.f16_wide && block_has_planes(C)) {
    // weight-stationary kernel: one workgroup per CU (C = 128) / two (C = 64), token groups of 64 = whole windows
    if (64 % N == 0 && C >= 64) return launch_of(k_qkv_fwd_ws(C), 6 * C, qkv_fwd_h_lds(C, 2));
    if (N % 64 == 0 || 64 % N == 0) return launch_of(k_qkv_fwd_h(C), 256, qkv_fwd_h_lds(C, 1));
  }
  return launch_of(k_qkv_fwd(C), 256, qkv_fwd_lds(C, N));
}

static BlockLaunch plan_mlp_fwd(const BlockShape& sh, bool padded, bool stores_upre) {
  const int C = sh.C, N = sh.N;
  if (!padded && sh.f16_wide && block_has_planes(C) && N % 32 == 0) {
    // threads of a k_mlp_fwd_h workgroup at C = 64, 128: 256 (four waves, four or eight hidden chunks, <= 53 000 bytes of LDS, three
    // workgroups per CU, every K-chunk's weight fragments of a proj / fc1 unit requested together: 135-163 registers).  Measured
    // 256 / 512 threads (512: two per CU at 128 registers): `mlp_fwd` 1.625 / 1.620 ms per step serialised, the step 12.67 / 12.69
    // ms (three interleaved rounds, each in favour of 256), inference 562.3 k / 557.6 k windows/s.  C = 32 runs 512.
    // Hidden chunks: the fewest whose tiles fit the workgroup's LDS budget.  (Four-wave workgroups: three per CU.  The hardware
    // admits one workgroup fewer than 160 KB / LDS suggests once the last one would end within a granule of the top: 53 000 bytes
    // run three per CU, 54 576 two - tools/diag/occ_probe.hip, census - while hipOccupancyMaxActiveBlocksPerMultiprocessor still
    // answers three.)
    const int nth = C == 32 ? 512 : 256;
    const size_t budget = nth == 256 ? 53000 : 78000;
    int nch = 1;
    while (nch < (nth == 256 ? 8 : 4) && mlp_fwd_h_lds(C, N, nch) > budget) nch *= 2;
    return launch_of(k_mlp_fwd_h(C, nch), nth, mlp_fwd_h_lds(C, N, nch), nch);
  }
  // strips of the narrow levels (64 tokens: a whole number of strips at every width); they write neither u_pre nor a second output
  if (!padded && !sh.second_out && !stores_upre && sw_mlp_fwd_w() && N % 64 == 0 && C <= 32) {
    if (sw_mlp_fwd_w() >= 3 && sh.f16_narrow) return launch_of(k_mlp_fwd_wh(C), 256, mlp_fwd_w_lds(C, true));
    if (sw_mlp_fwd_w() == 2 || C == 16) return launch_of(k_mlp_fwd_w(C), 256, mlp_fwd_w_lds(C, false));
  }
  int nch = 1;
  while (nch < 4 && mlp_fwd_lds(C, N, nch) > MLP_LDS) nch *= 2;
  return launch_of(k_mlp_fwd(C, nch), 512, mlp_fwd_lds(C, N, nch), nch);
}

static BlockLaunch plan_mlp_bwd(const BlockShape& sh, bool padded, int tw) {
  const int C = sh.C, N = sh.N;
  if (!padded && sh.f16_wide && !tw) {
    if (const int nh = mlp_bwd_h_nch(C, N))
      return nh > 0 ? launch_of(k_mlp_bwd_h4(C, nh), 256, mlp_bwd_h_lds(C, N, nh, true), nh)
                    : launch_of(k_mlp_bwd_h8(C, -nh), 512, mlp_bwd_h_lds(C, N, -nh, false), -nh);
  }
  if (!padded && tw && sw_mlp_bwd_w() && (C == 16 || (sw_mlp_bwd_w() >= 2 && C == 8) || (sw_mlp_bwd_w() >= 3 && C == 32))) {
    const bool h16 = C == 32 && sh.f16_narrow && sw_mlp_bwd_w_f16();
    int threads;
    const size_t lds = mlp_bwd_w_lds(C, h16, &threads);
    return launch_of(C == 32 ? (h16 ? K::MLP_BWD_W2_32_H : K::MLP_BWD_W2_32) : (C == 8 ? K::MLP_BWD_W_8 : K::MLP_BWD_W_16), threads, lds);
  }
  if (tw) {   // (padded windows at a fused shape too: its local-enhancement conv knows where the window ends)
    const size_t tiles = mlp_bwd_s_lds(C, N), flush = mlp_bwd_s_flush_lds(C);
    return launch_of(k_mlp_bwd_s(C, tw), 512, tiles > flush ? tiles : flush);
  }
  int nch = 1;
  while (nch < 4 && mlp_bwd_lds(C, N, nch) > MLP_LDS) nch *= 2;
  return launch_of(k_mlp_bwd(C, nch), 512, mlp_bwd_lds(C, N, nch), nch);
}

static BlockLaunch plan_qkv_bwd(const BlockShape& sh) {
  const int C = sh.C, N = sh.N;
  if (sh.f16_wide && qkv_bwd_h_takes(C, N)) return launch_of(k_qkv_bwd_h(C), 512, qkv_bwd_h_lds(C, N));
  return launch_of(k_qkv_bwd(C), 512, qkv_bwd_lds(C, N));
}

// a weight-gradient product: split operands when the block's data-gradient kernels publish their maxima and a token chunk of
// at least one 32-token MFMA step divides N within the LDS budget, else fp32 operands
static BlockLaunch plan_dw(int C, int N, int prod, bool split) {
  K (*const plain[4])(int) = {k_dw_FC2, k_dw_FC1, k_dw_PROJ, k_dw_QKV};
  K (*const halves[4])(int) = {k_dw_FC2_h, k_dw_FC1_h, k_dw_PROJ_h, k_dw_QKV_h};
  int tc; size_t lds;
  if (split && dw_chunk(C, prod, N, true, &tc, &lds)) return launch_of(halves[prod](C), 512, lds, tc, true);
  dw_chunk(C, prod, N, false, &tc, &lds);
  return launch_of(plain[prod](C), 512, lds, tc, false);
}

BlockPlan block_plan(const BlockShape& sh) {
  const int C = sh.C, N = sh.N;
  const bool padded = sh.NE > 0 && sh.NE < N;   // padded windows: the generic kernels (their local-enhancement conv knows where the window ends)
  const int tw = fused_tw(C, N);
  BlockPlan p;
  p.stores_upre = sh.training && !tw;
  p.mlp_dw_fused = tw != 0;
  // only when both split data-gradient kernels take the shape (they publish the maxima the split products scale by)
  p.dw_split = sh.f16_wide && sh.want_dw && !tw && mlp_bwd_h_nch(C, N) != 0 && qkv_bwd_h_takes(C, N);
  p.qkv_fwd = plan_qkv_fwd(sh);
  p.mlp_fwd = plan_mlp_fwd(sh, padded, p.stores_upre);
  p.mlp_bwd = plan_mlp_bwd(sh, padded, tw);
  p.qkv_bwd = plan_qkv_bwd(sh);
  for (int i = 0; i < 4; ++i)
    p.dw[i] = (p.mlp_dw_fused && (i == DW_FC2 || i == DW_FC1)) ? launch_of(K::NONE, 0, 0) : plan_dw(C, N, i, p.dw_split);
  return p;
}
