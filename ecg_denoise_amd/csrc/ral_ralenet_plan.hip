// RA-LENet pass (see ral_ralenet_plan.hpp): the only place the network's shape is written.  Host code only.
#include <stdio.h>

#include "ral_block_plan.hpp"
#include "ral_ralenet_plan.hpp"

// ---- the network (reference raletransformer.py:640-672): four encoder stages, each followed by a PatchMerging; the bottleneck
// with its residual; four decoder stages, each followed by a PatchSeparate that adds the encoder feature of its output's
// level (ps1: none - the head adds x0).  "utranformer3" is the reference's spelling.
#define ST(si, level, rw, name, in, add, out) {RN_STAGE, si, level, rw, 0, 0, name, in, add, out}
#define PM(ri, level, name, in, out) {RN_RES, ri, level, 0, CH[level], 0, name, in, RT_NONE, out}
#define PS(ri, level, name, in, add, out) {RN_RES, ri, level, 0, CH[level], 1, name, in, add, out}
const RalNode RAL_NET[RAL_NODES] = {
    ST(0, 0, 1, "dtransformer1", RT_X0, RT_NONE, RT_S0),  PM(0, 1, "pm1", RT_S0, RT_P1),
    ST(1, 1, 2, "dtransformer2", RT_P1, RT_NONE, RT_S1),  PM(1, 2, "pm2", RT_S1, RT_P2),
    ST(2, 2, 3, "dtransformer3", RT_P2, RT_NONE, RT_S2),  PM(2, 3, "pm3", RT_S2, RT_P3),
    ST(3, 3, 4, "dtransformer34", RT_P3, RT_NONE, RT_S3), PM(3, 4, "pm4", RT_S3, RT_P4),
    ST(4, 4, 0, "transformer", RT_P4, RT_P4, RT_XMID),
    ST(5, 4, 0, "utransformer4", RT_XMID, RT_NONE, RT_S5), PS(4, 3, "ps4", RT_S5, RT_P3, RT_U3),
    ST(6, 3, 4, "utranformer3", RT_U3, RT_NONE, RT_S6),    PS(5, 2, "ps3", RT_S6, RT_P2, RT_U2),
    ST(7, 2, 3, "utransformer2", RT_U2, RT_NONE, RT_S7),   PS(6, 1, "ps2", RT_S7, RT_P1, RT_U1),
    ST(8, 1, 2, "utransformer1", RT_U1, RT_NONE, RT_S8),   PS(7, 0, "ps1", RT_S8, RT_NONE, RT_U0),
};
#undef ST
#undef PM
#undef PS

static const int STAGE_NODE[9] = {0, 2, 4, 6, 8, 9, 11, 13, 15};   // rows of RAL_NET (tests/test_ralenet_plan_cpu.py checks them against it)
const RalNode& ralenet_stage(int si) { return RAL_NET[STAGE_NODE[si < 0 ? 0 : (si > 8 ? 8 : si)]]; }

const char* ralenet_tensor_name(int t) {
  static const char* const N[RT_COUNT] = {"x0", "s0", "s1", "s2", "s3", "s4", "s5", "s6", "s7", "s8", "p1", "p2", "p3", "p4", "xmid",
                                          "u3", "u2", "u1", "u0"};
  return N[t];
}
void ralenet_grad_name(int g, char out[8]) {
  if (g == RG_DU0) snprintf(out, 8, "du0");
  else if (g >= RG_GIN0) snprintf(out, 8, "gin%d", g - RG_GIN0);
  else snprintf(out, 8, "gy%d", g - RG_GY0);
}

int ralenet_grad_of(int t) {
  if (t == RAL_HEAD_IN) return RG_DU0;
  for (const RalNode& n : RAL_NET)
    if (n.kind == RN_STAGE && n.in == t) return RG_GIN0 + n.idx;
  for (const RalNode& n : RAL_NET)
    if (n.kind == RN_STAGE && n.out == t) return RG_GY0 + 2 * n.idx + 1;
  return RG_NONE;
}
bool ralenet_grad_is_buffer(int g) { return g >= RG_GIN0 || ralenet_gy(g / 2, g % 2) == g; }
int ralenet_gy(int si, int blk) { return blk == 0 ? RG_GY0 + 2 * si : ralenet_grad_of(ralenet_stage(si).out); }
int ralenet_extra_of(const RalNode& nd) {
  // (the head forms its sum in front of the conv: the gradient of the sum is the gradient of the head's input)
  if (RAL_HEAD_ADD == nd.in) return ralenet_grad_of(RAL_HEAD_IN);
  for (const RalNode& n : RAL_NET)
    if (n.add == nd.in) return ralenet_grad_of(n.out);
  return RG_NONE;
}

RalBinding ralenet_bind(const RalNode& nd, bool backward) {
  if (!backward) return RalBinding{nd.in, nd.add, nd.out, RT_NONE};
  return RalBinding{ralenet_grad_of(nd.out), nd.kind == RN_STAGE ? ralenet_extra_of(nd) : RG_NONE, ralenet_grad_of(nd.in), nd.in};
}

RalPassEntry ralenet_pass(bool backward, int e) {
  const int node = backward ? RAL_NODES - 1 - e : e;
  // the decoder's parameters have their final gradients once its first node, the last of them the backward reaches, has run
  return RalPassEntry{node, backward && node == RAL_DEC_NODE};
}

RalLaneSplit ralenet_lane_split(int B, int n_lanes) {
  RalLaneSplit s{};
  s.n = (B < 64 * n_lanes || B % n_lanes != 0) ? 1 : n_lanes;
  for (int i = 0; i < s.n; ++i) { s.w0[i] = i * (B / s.n); s.B[i] = B / s.n; }
  return s;
}

const BlockMat BLOCK_MATS[4] = {{&BlockOff::wqkv, 3, 1}, {&BlockOff::wp, 1, 1}, {&BlockOff::w1, 4, 1}, {&BlockOff::w2, 1, 4}};

int ralenet_mat_descs(const RalOff& O, bool planes_only, bool transposed, int unit_div, bool with_res, std::vector<int>& d) {
  int run = 0;
  auto add = [&](int64_t off, int rows, int cols) {
    const int v[4] = {(int)off, transposed ? cols : rows, transposed ? rows : cols, run};
    d.insert(d.end(), v, v + 4);
    run += rows * cols / unit_div;
  };
  for (int b = 0; b < RAL_NBLOCKS; ++b) {
    const int C = CH[ralenet_stage(b / 2).level];
    if (planes_only && !block_has_planes(C)) continue;
    for (const BlockMat& mt : BLOCK_MATS) add(O.blk[b].*mt.off, mt.rows * C, mt.cols * C);
  }
  if (with_res)
    for (const ResOff& r : O.res) add(r.w, r.D, r.D);
  return run;
}
