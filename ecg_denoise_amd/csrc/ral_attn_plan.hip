// Attention dispatch (see ral_attn_plan.hpp): the only place that reads the ATTN_* switches and the only place that knows
// which kernel a shape gets, what LDS it takes and what scratch it needs.  Host code only.
#include "ral_device.hpp"
#include "ral_attn_plan.hpp"

// The switches (ral_global_option; each latched at its first read):
//   ATTN_F16      default of the operator entry points' f16
//   ATTN_FWD_W    wave-per-head forward: 0 never, 1 at N = 32, 2 at N = 64 and 128 too.  Measured at batch 2048 (us per
//                 launch, k_attn_fwd_w with f16 tiles / the kernels of ral_fwd.hip): N = 32: 39 / 45, 64 (table): 64 / 54,
//                 128 (table): 90 / 91 - the scalar-path forward keeps N = 64 and 128
//   ATTN_FWD_H    smallest N whose tile kernel has its S tile on the f16 matrix cores (0 = never)
//   ATTN_FWD_T32  smallest N that takes the 32x32 score blocks of k_attn_fwd_t32 (0 = never).  Measured at batch 2048
//                 (tools/attn_bench.py, us per launch, three interleaved rounds, the kernel the level had before vs
//                 k_attn_fwd_t32): N = 512: 274 / 253, 278 / 252, 277 / 252, 256: 162 / 150, 161 / 151, 165 / 148,
//                 128: 91 / 107, 91 / 106, 91 / 106, 64: 53 / 80, 54 / 80, 53 / 80 (profiles/attn_fwd_t32_levels.txt)
//   ATTN_BWD_M / ATTN_BWD_MH / ATTN_BWD_W   0: that backward family is never chosen
#define ATTN_SWITCH(fn, name, dflt) \
  static int fn() { static const int v = (int)ral_knob(name, dflt); return v; }
ATTN_SWITCH(sw_f16, "ATTN_F16", 1)
ATTN_SWITCH(sw_fwd_w, "ATTN_FWD_W", 1)
ATTN_SWITCH(sw_fwd_h, "ATTN_FWD_H", 256)
ATTN_SWITCH(sw_fwd_t32, "ATTN_FWD_T32", 256)
ATTN_SWITCH(sw_bwd_m, "ATTN_BWD_M", 1)
ATTN_SWITCH(sw_bwd_mh, "ATTN_BWD_MH", 1)
ATTN_SWITCH(sw_bwd_w, "ATTN_BWD_W", 1)
#undef ATTN_SWITCH
int attn_f16_default() { return sw_f16(); }

static const char* const ATTN_NAMES[] = {
#define X(e, name) name,
  ATTN_KERNELS(X)
#undef X
};
using K = AttnKernel;
static AttnPlan plan_of(K k, int hg, int threads, size_t lds) {
  return AttnPlan{k, ATTN_NAMES[(int)k], hg, threads, lds, 0, false, 0};
}
// the instance of a <N, table[, f16]> family whose first enumerator is `first` (enumerators in ATTN_KERNELS order)
static K w_instance(K first, int N, bool table, int nf16, int f16) {
  const int n = N == 32 ? 0 : (N == 64 ? 1 : 2);
  return (K)((int)first + (n * 2 + (table ? 1 : 0)) * nf16 + (nf16 > 1 && f16 ? 1 : 0));
}

// LDS budgets of a tile-kernel workgroup (bytes; fewer bytes = smaller head groups but more co-resident workgroups per CU)
static constexpr size_t ATTN_FWD_LDS = 72 * 1024, ATTN_BWD_LDS = 78 * 1024;
// Workgroup split of the tile kernels (forward and backward): 1 / ATTN_SPLIT of the head group per item and 512 / ATTN_SPLIT
// threads, so that 2 * ATTN_SPLIT workgroups share a CU and one's staging latency and barrier waits hide behind the others'
// tiles (same waves per CU, same LDS).  Measured at batch 2048 (fwd + bwd attention, ms per step): split 1: 7.76,
// split 2: 7.53.  Head groups or windows it does not divide (HG % 2, N % 32) run unsplit.
static constexpr int ATTN_SPLIT = 2;

static size_t tile_fwd_lds(int N, int HG, int Len) {
  return ((size_t)3 * HG * N * 4 + (size_t)HG * N + 3 * HG + 8 + (Len > 0 ? (size_t)(2 * Len - 1) * HG : 0)) * sizeof(float);
}
static size_t tile_bwd_lds(int N, int HG, int Len) {
  return ((size_t)4 * HG * N * 4 + (size_t)2 * HG * N + (Len > 0 ? (size_t)2 * (2 * Len - 1) * HG : 0) + 4) * sizeof(float);
}
// head group of the tile kernels: the largest power-of-two fraction of the heads whose tiles fit the LDS budget
static int head_group(int N, int H, int Len, bool bwd) {
  int hg = H;
  while (hg > 1 && (bwd ? tile_bwd_lds(N, hg, Len) > ATTN_BWD_LDS : tile_fwd_lds(N, hg, Len) > ATTN_FWD_LDS)) hg /= 2;
  return hg;
}
// the wave-per-head kernels take the short windows (two heads per wave at N = 32; the table lives in the LDS)
static bool short_window(int N, int H, int Len) {
  return (N == 32 || N == 64 || N == 128) && !(N == 32 && (H & 1)) && !(Len > 0 && (2 * Len - 1) * H > 2048);
}
static int wave_heads(int N) { return N >= 64 ? 1 : 64 / N; }
// upper bound of a wave-per-head kernel's grid: one four-wave workgroup per four tasks
static int wave_rows(int N, int H, int B) {
  const int ntask = B * H / wave_heads(N), g = (ntask + 3) / 4;
  return g < ATTN_ROWS_MAX ? g : ATTN_ROWS_MAX;
}

AttnPlan attn_fwd_plan(int N, int H, int Len, int f16, int NE) {
  const bool table = Len > 0;
  const int HG = head_group(N, H, Len, false);
  if (NE > 0 && NE < N) return plan_of(K::FWD_RAG, HG, 512, tile_fwd_lds(N, HG, Len));   // padded windows: the generic tile kernel with its key mask
  if (sw_fwd_w() && short_window(N, H, Len) && (sw_fwd_w() >= 2 || N == 32)) {
    const int hw = wave_heads(N), ntab = table ? (2 * Len - 1) * H : 0;
    return plan_of(w_instance(K::FWD_W32, N, table, 2, f16), hw, 256, ((size_t)4 * hw * N * 13 + ntab + (table ? H : 0)) * sizeof(float));
  }
  const int split_hg = HG % ATTN_SPLIT == 0 ? HG / ATTN_SPLIT : HG, split_threads = split_hg == HG ? 512 : 512 / ATTN_SPLIT;
  if (f16 && sw_fwd_t32() > 0 && N >= sw_fwd_t32() && N % 64 == 0)
    return plan_of(table ? K::FWD_T32_TAB : K::FWD_T32, split_hg, split_threads, tile_fwd_lds(N, split_hg, Len));
  // Window lengths [64, 256] take the query-per-lane kernel on the scalar path.  Measured at batch 2048 (tools/attn_bench.py,
  // us per launch, fp32 MFMA-tile kernel vs scalar path): N = 512: 322 / 333, 256: 184 / 172, 128: 122 / 90, 64: 91 / 51.
  // With its S tile on the f16 matrix cores the tile kernel takes the long windows from the scalar path again.
  const bool tile16 = f16 && sw_fwd_h() > 0 && N >= sw_fwd_h() && N % 32 == 0;
  if (!tile16 && N >= 64 && N <= 256 && N % 4 == 0 && (!table || 2 * Len - 1 <= 64)) return plan_of(table ? K::FWD_V_TAB : K::FWD_V, 1, 256, 0);
  if (HG % ATTN_SPLIT == 0 && N % 32 == 0)
    return plan_of(N == 32 && !table ? K::FWD_G2_N32 : (tile16 ? K::FWD_G2_F16 : K::FWD_G2), split_hg, split_threads, tile_fwd_lds(N, split_hg, Len));
  return plan_of(N % 32 == 0 ? K::FWD_G2 : K::FWD_G1, HG, 512, tile_fwd_lds(N, HG, Len));
}

// ---- the one-sweep workgroup kernel of the long windows (k_attn_bwd_mh): eight waves of KT key tiles each
static int mh_kt(int N) { return N >= 1024 ? 8 : 4; }
static int mh_hg(int N) {
  const int wph = N / (16 * mh_kt(N));
  return wph >= 8 ? 1 : 8 / wph;
}
static size_t mh_lds(int N, int H, int hg, int Len) {
  return ((size_t)26 * hg * N + 4 * 32 + 4 * hg + 8 * 4 * 160 + (Len > 0 ? (size_t)3 * (2 * Len - 1) * H + 2 : 0) + 4) * sizeof(float);
}
static bool mh_takes(int N, int H, int Len) {
  if (!sw_bwd_mh() || N < 256) return false;
  const int kt = mh_kt(N), wph = N / (16 * kt);
  if (N % (16 * kt) != 0 || (wph != 1 && wph != 2 && wph != 4 && wph != 8)) return false;
  const int hg = mh_hg(N);
  if (H % hg != 0 || hg * N != 128 * kt) return false;   // (the kernel's T: eight waves of kt key tiles)
  if (Len > 0 && (2 * Len - 1) * H > 2048) return false;
  return mh_lds(N, H, hg, Len) <= 150 * 1024;
}

AttnPlan attn_bwd_plan(int N, int H, int Len, int f16, int NE, int B) {
  const bool table = Len > 0;
  const int HG = head_group(N, H, Len, true);
  if (NE > 0 && NE < N) return plan_of(K::BWD_RAG, HG, 512, tile_bwd_lds(N, HG, Len));
  const int ntab = table ? (2 * Len - 1) * H : 0;
  // the kernels that leave the table gradient as one row of partials per workgroup
  auto partials = [&](AttnPlan p, int rows) {
    p.rows = rows; p.table_partials = table; p.scratch_floats = table ? (size_t)rows * ntab : 0;
    return p;
  };
  const int hw = wave_heads(N), nwv = 4;   // (waves per workgroup of the wave-per-head kernels)
  // one sweep with every contraction on the f16 matrix cores (ral_attnm.hip)
  if (f16 && sw_bwd_m() && short_window(N, H, Len))
    return partials(plan_of(w_instance(K::BWD_M32, N, table, 1, 0), hw, 64 * nwv,
                            ((size_t)nwv * (hw * N * 18 + 4 * 32 + 4 * 160) + 3 * ntab + 2) * sizeof(float)), wave_rows(N, H, B));
  if (f16 && mh_takes(N, H, Len)) {
    const int hg = mh_hg(N), items = B * (H / hg);
    const K k = mh_kt(N) == 4 ? (table ? K::BWD_MH4_TAB : K::BWD_MH4) : (table ? K::BWD_MH8_TAB : K::BWD_MH8);
    return partials(plan_of(k, hg, 512, mh_lds(N, H, hg, Len)), items < ATTN_ROWS_MAX ? items : ATTN_ROWS_MAX);
  }
  // short windows: one wave per head, fp32 tiles, no workgroup barriers (ral_attn.hip): strict mode, or the one-sweep kernels switched off
  if (sw_bwd_w() && short_window(N, H, Len))
    return partials(plan_of(w_instance(K::BWD_W32, N, table, 1, 0), hw, 64 * nwv, ((size_t)nwv * hw * N * 18 + 2 * ntab) * sizeof(float)),
                    wave_rows(N, H, B));
  // Window lengths that take the scalar-path sweeps.  Measured at batch 2048 (tools/attn_bench.py, us per launch, MFMA-tile
  // kernel vs scalar path).  Without an R-wave table: N = 512: 790 / 853, 256: 446 / 464, 128: 285 / 265, 64: 208 / 155;
  // with one (the in-window keys cost two lane gathers each, plus a partial-sum pass): 128: 285 / 293, 64: 208 / 192, and
  // inside the training step (bench.py --kinds) the N = 64 case with a table came out 2 % slower than the MFMA-tile kernel.
  // So: N <= 128 without a table, never with one.  Scratch: (B, H, N, 2) floats handed from the query sweep to the key /
  // value sweep (the (B, 2, H, 64) tail is what callers have always been told to add; nothing reads it).
  if (!table && N >= 64 && N <= 128 && N % 4 == 0) {
    AttnPlan p = plan_of(K::BWD_V, 1, 256, 0);
    p.scratch_floats = (size_t)B * H * N * 2 + (size_t)B * 2 * H * 64;
    return p;
  }
  if (HG % ATTN_SPLIT == 0 && N % 32 == 0) {
    const int hg = HG / ATTN_SPLIT;
    return plan_of(N == 32 && !table ? K::BWD_G2_N32 : (N == 64 && table ? K::BWD_G2_N64_TAB : K::BWD_G2), hg, 512 / ATTN_SPLIT, tile_bwd_lds(N, hg, Len));
  }
  return plan_of(N % 32 == 0 ? K::BWD_G2 : K::BWD_G1, HG, 512, tile_bwd_lds(N, HG, Len));
}
