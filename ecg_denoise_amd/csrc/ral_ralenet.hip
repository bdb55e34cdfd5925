// RA-LENet (nra / full / mlp) behind the model interface of ral_model.hpp: its parameter layout, workspace plan, lanes and
// the host orchestration of its kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "ral_model.hpp"
#include "ral_kernels.hpp"
#include "ral_ralenet.hpp"
#include "ral_ralenet_plan.hpp"

// Event records / stream waits of the fork-join scheduler: a failed one would silently drop an ordering edge (a race,
// not an error), so the first failure is remembered and the entry point that issued it returns it (sched_check).
static thread_local hipError_t g_sched_err = hipSuccess;
static thread_local const char* g_sched_what = "";
#define EV(expr)                                                                             \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess && g_sched_err == hipSuccess) { g_sched_err = e_; g_sched_what = #expr; } \
  } while (0)
// every entry point that records events / stream waits starts from a clean slate (an error remembered by a call that left
// through another failure must not surface in a later, unrelated one) and ends with sched_check()
static void sched_reset() { g_sched_err = hipSuccess; g_sched_what = ""; }
static int sched_check() {
  if (g_sched_err == hipSuccess) return 0;
  const hipError_t e = g_sched_err;
  g_sched_err = hipSuccess;
  return ral_fail("stream scheduling: %s failed: %s (an ordering edge was lost: the results of this call are undefined)",
              g_sched_what, hipGetErrorString(e));
}

// ---------------------------------------------------------------------------------
// layout
// ---------------------------------------------------------------------------------
static void build_layout(const ral_config& c, ParamLayout& L, RalOff& O) {
  // 32-byte granules: the fp16 planes of a weight matrix are read 16 bytes (8 elements) at a time
  auto alloc_f = [&](int64_t n) { return L.alloc(n, 8); };
  const bool basic = c.variant != RAL_NRA;
  O.le = c.variant != RAL_MLP;
  O.rwave = c.variant != RAL_NRA;
  const int ld = c.leads;
  O.conv1_w = alloc_f(8 * ld * 3); O.conv1_b = alloc_f(8);
  O.bn_w = alloc_f(8); O.bn_b = alloc_f(8);
  L.add("conv1.0.weight", RAL_PARAM, O.conv1_w, {8, ld, 3});
  L.add("conv1.0.bias", RAL_PARAM, O.conv1_b, {8});
  L.add("conv1.2.weight", RAL_PARAM, O.bn_w, {8});
  L.add("conv1.2.bias", RAL_PARAM, O.bn_b, {8});
  L.add("conv1.2.running_mean", RAL_STATE_F32, 0, {8});
  L.add("conv1.2.running_var", RAL_STATE_F32, 8, {8});
  L.add("conv1.2.num_batches_tracked", RAL_COUNTER_I64, 0, {});
  L.nstate = 16;
  if (O.rwave) {
    for (int i = 0; i < 4; ++i) {
      const int h = CH[i] / 4, n = 2 * RWLEN[i] - 1;
      O.rw[i] = alloc_f((int64_t)n * h);
      const std::string p = "rwattn" + std::to_string(i + 1);
      L.add(p + ".relative_position_bias_table", RAL_PARAM, O.rw[i], {n, h});
      L.add(p + ".relative_position_index", RAL_INDEX_I64, 0, {RWLEN[i], RWLEN[i]});
    }
  }
  auto add_block = [&](int bi, const std::string& pre, int C) {
    BlockOff& b = O.blk[bi];
    b.wqkv = alloc_f(3 * C * C); b.bqkv = alloc_f(3 * C);
    b.wp = alloc_f(C * C); b.bp = alloc_f(C);
    b.ln1w = alloc_f(C); b.ln1b = alloc_f(C); b.ln2w = alloc_f(C); b.ln2b = alloc_f(C);
    b.w1 = alloc_f(4 * C * C); b.b1 = alloc_f(4 * C);
    b.w2 = alloc_f(4 * C * C); b.b2 = alloc_f(C);
    b.le = O.le ? alloc_f(3) : -1;
    L.add(pre + "attn.qkv_proj.to_q.weight", RAL_PARAM, b.wqkv, {C, C});
    L.add(pre + "attn.qkv_proj.to_q.bias", RAL_PARAM, b.bqkv, {C});
    L.add(pre + "attn.qkv_proj.to_kv.weight", RAL_PARAM, b.wqkv + C * C, {2 * C, C});
    L.add(pre + "attn.qkv_proj.to_kv.bias", RAL_PARAM, b.bqkv + C, {2 * C});
    L.add(pre + "attn.proj.weight", RAL_PARAM, b.wp, {C, C});
    L.add(pre + "attn.proj.bias", RAL_PARAM, b.bp, {C});
    L.add(pre + "norm1.weight", RAL_PARAM, b.ln1w, {C});
    L.add(pre + "norm1.bias", RAL_PARAM, b.ln1b, {C});
    L.add(pre + "norm2.weight", RAL_PARAM, b.ln2w, {C});
    L.add(pre + "norm2.bias", RAL_PARAM, b.ln2b, {C});
    L.add(pre + "mlp.fc1.weight", RAL_PARAM, b.w1, {4 * C, C});
    L.add(pre + "mlp.fc1.bias", RAL_PARAM, b.b1, {4 * C});
    L.add(pre + "mlp.fc2.weight", RAL_PARAM, b.w2, {C, 4 * C});
    L.add(pre + "mlp.fc2.bias", RAL_PARAM, b.b2, {C});
    if (O.le) L.add(pre + "mlp.leconv.partial_conv3.weight", RAL_PARAM, b.le, {1, 1, 3});
  };
  auto add_stage = [&](const RalNode& st) {
    for (int i = 0; i < 2; ++i) {
      const std::string pre = std::string(st.name) + (basic ? ".blocks." : ".") + std::to_string(i) + ".";
      add_block(st.idx * 2 + i, pre, CH[st.level]);
    }
  };
  auto add_res = [&](int ri, const std::string& name, int D) {
    ResOff& r = O.res[ri];
    r.D = D;
    r.w = alloc_f((int64_t)D * D); r.lnw = alloc_f(D); r.lnb = alloc_f(D);
    L.add(name + ".reduction.weight", RAL_PARAM, r.w, {D, D});
    L.add(name + ".norm.weight", RAL_PARAM, r.lnw, {D});
    L.add(name + ".norm.bias", RAL_PARAM, r.lnb, {D});
  };
  for (int i = 0; i < RAL_NODES; ++i) {
    const RalNode& nd = RAL_NET[i];
    if (i == RAL_DEC_NODE) O.dec_off = L.nparam;
    if (nd.kind == RN_STAGE) add_stage(nd); else add_res(nd.idx, nd.name, nd.D);
  }
  O.tc_w = alloc_f(ld * 8 * 3); O.tc_b = alloc_f(ld);
  L.add("transconv.0.weight", RAL_PARAM, O.tc_w, {ld, 8, 3});
  L.add("transconv.0.bias", RAL_PARAM, O.tc_b, {ld});
}
static void ralenet_layout(const ral_config& c, ParamLayout& L) { RalOff o; build_layout(c, L, o); }

static int check_cfg(const ral_config* c) {
  if (c->leads != 1 && c->leads != 2) return ral_fail("leads must be 1 or 2 (got %d); use the 12-lead adapter above it", c->leads);
  // the reference's own constraint (raletransformer.py:170,448-450): four PatchMerging halvings -> a multiple of 16 (its positional
  // table ends at 1000; 1024 is accepted here).  The R-wave variants also need their (32, 16, 8, 4)-token windows to fit.
  if (c->L <= 0 || c->L % 16 != 0 || c->L > 1024) return ral_fail("L must be a multiple of 16 and <= 1024 (got %d)", c->L);
  if (c->variant != RAL_NRA && c->L < 32) return ral_fail("L must be at least 32 for the R-wave variants (got %d)", c->L);
  if (c->max_batch <= 0) return ral_fail("max_batch must be positive");
  return 0;
}

// positional encoding in the reference's op order, fp32 (raletransformer.py:172-181)
static void fill_pe(float* P, int n, int C) {
  for (int i = 0; i < C / 2; ++i) {
    const float den = powf(10000.0f, (float)(2 * i) / (float)C);
    for (int p = 0; p < n; ++p) {
      const float X = (float)p / den;
      P[(size_t)p * C + 2 * i] = sinf(X);
      P[(size_t)p * C + 2 * i + 1] = cosf(X);
    }
  }
}

// ---------------------------------------------------------------------------------
// model
// ---------------------------------------------------------------------------------
struct BlockAct { float *in, *qkv, *o, *lse, *x1, *upre, *out; };

// Sets of per-block backward temporaries (dx1, do, dqkv, du_pre, ...): block i of a lane's chain may start once the
// weight-gradient kernels of block i - dw_sets() have finished with theirs.  At the wide levels a block's four
// weight-gradient launches take about as long as its chain, so with two sets the chain waits for them; with more it runs
// ahead and the side stream catches up under the narrow levels, whose weight gradients are fused into the chain kernels.
// Measured at batch 2048 (ms per step): 2 sets 17.09, 3: 17.08, 4: 17.04, 6: 17.00, 8: 16.99; a set is 9.6 E floats
// (0.32 GB at batch 2048).  RAL_DW_SETS overrides (2 .. MAX_SETS).
#define MAX_SETS 8
static int dw_sets() {
  static const int n = [] {
    int k = (int)ral_knob("DW_SETS", 6);
    return k < 2 ? 2 : (k > MAX_SETS ? MAX_SETS : k);
  }();
  return n;
}

// ---------------------------------------------------------------------------------
// lanes: the windows of a batch are independent through the whole transformer stack, so a batch is cut
// into NL contiguous micro-batches ("lanes") that run the same kernel chain on separate HIP streams.
// Kernels of different kinds (VALU-bound attention, MFMA/latency-bound projections) then share the CUs.
// Every tensor is batch-major, so a lane is just a pointer offset of w0 windows.
// ---------------------------------------------------------------------------------
struct Lane {
  int w0 = 0, B = 0;
  hipStream_t s = nullptr, s2 = nullptr;     // chain stream, weight-gradient side stream
  hipEvent_t ev_ready[MAX_SETS] = {}, ev_done[MAX_SETS] = {}, ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_dec_main = nullptr, ev_dec_side = nullptr;   // decoder half of the gradients complete (this lane)
  bool dw_pending[MAX_SETS] = {};
  int bwd_count = 0;
};
struct LaneSet { Lane l[MAX_LANES]; int n = 1; hipStream_t own[MAX_LANES] = {}; };

struct RalModel : ral_handle {
  ~RalModel() override;
  int init() override;
  int bind(float* params, float* grads, float* am, float* av, float* state, double* bn_sums) override;
  int forward(const float* x, float* y, int B, int training, hipStream_t s) override;
  int backward(const float* dy, float* dx, int B, hipStream_t s) override;
  int set_option(const char* key, int value) override;
  double* after_adam() override;
  RalOff off;
  int L, Lp, E1;  // L: samples per window; Lp: token slots per window at level 0 = L rounded up to a multiple of 256 (every level then
                  // has a multiple of 16 slots; the slots past L >> level do not exist for the model: masked keys, zero conv halos, no
                  // gradient); E1 = 8 * Lp floats per window per stage tensor
  size_t slab_bytes = 0;
  std::map<std::string, std::pair<float*, int64_t>> dbg;
  // workspace
  float* pe[5];
  float *xin, *a0, *ss;
  BlockAct act[RAL_NBLOCKS];
  float* ten[RT_COUNT];   // the named tensors of the node table (a stage output: the `out` of its second block)
  // backward temporaries
  // every gradient tensor has its own buffer (no ping-pong): the weight-gradient kernels run on a side
  // stream and read them long after the data-gradient chain has moved on
  float *gbuf[RG_COUNT], *dz0;   // (gbuf[gy9] stays null: ralenet_gy)
  float *dx1[MAX_SETS], *dohm[MAX_SETS], *dqkv[MAX_SETS], *dupre[MAX_SETS], *a2c0[MAX_SETS], *astat[MAX_SETS];   // per-block temporaries, dw_sets() sets (side-stream overlap)
  LaneSet* lanes = nullptr;
  int n_lanes = 2;
  bool side_stream = true;
  bool attn_f16 = true;      // attention score tiles (S, dP) as fp16-pair products - only while f16_split > 0 (option "attn_f16"; RAL_ATTN_F16=0)
  bool narrow_f16 = true;    // the strip kernel of the narrow levels' MLP forward on fp16-pair products - only while f16_split > 0 (option "narrow_f16")
  int f16_split = 64;         // narrowest width whose Linear layers (q/k/v projection, proj, fc1, fc2 of the forward) run as
                              // two-piece fp16 products on the f16 matrix cores (0 = none: fp32 MFMA everywhere)
  bool want_dw = true;      // false inside ral_backward_input: frozen weights, data gradients only
  int dec_lanes = 0; bool dec_side = false;   // lanes / side streams that carried the last backward (bucket events)
  hipEvent_t ev_bwd_done = nullptr;          // recorded at the end of ral_backward_end
  // weight preparation under the stem: the split planes of this forward (and, in training, the transposes + their planes for
  // its backward) are formed on lane 0's weight-gradient stream - idle during a forward - while the caller's stream runs the
  // stem conv / BatchNorm; fwd_end / bwd_begin wait for the events instead of launching the kernels (side_stream = 0: inline)
  hipEvent_t ev_prep_go = nullptr, ev_prep_fwd = nullptr, ev_prep_bwd = nullptr;
  bool prep_fwd = false, prep_bwd = false;
  // option "static_params" (the host mirror sets it in eval mode): the caller promises not to touch the parameters until it says so
  // again, so the activation scales and the weight planes an eval forward formed stay valid for the next one - a forward then has no
  // preparation kernels at all (they were ~0.1 ms of a 3.6 ms inference forward)
  bool static_params = false, planes_valid = false, skip_prep = false;
  bool sums_clean = false;   // bn_sums[0, 32) were zeroed by the optimiser kernel of the previous step (no fill kernel in front of the stem)
  bool prep_stale = false;   // parameters or arithmetic options changed after the preparation was queued: the backward re-builds its planes
  bool bwd_recorded = false;
  float* paramsT = nullptr;   // transposed copies of the weight matrices (same offsets), refreshed per backward
  unsigned short* wh = nullptr;             // tiled split planes of the wide levels' weight matrices (a matrix at twice its float
                                            // offset), re-written every forward from the descriptors below
  float* ascale = nullptr;                  // device: ASC_N activation scales per transformer block (k_act_scales, once per forward)
  int* adesc = nullptr;                     // device: 12 ints per block (its descriptor)
  int* wdesc = nullptr;                     // device: int4 {offset, rows, columns, first work item} per matrix
  int ndesc = 0, nwork = 0;
  unsigned* gmax = nullptr;                 // (18 blocks x 4 lanes x 4) largest-magnitude bits of dx2 / du / dx1 / dqkv per block and lane: scales of the split weight-gradient products; zeroed per backward
  unsigned short* whT = nullptr;            // the same for the transposed matrices of the backward (from paramsT), training only
  int* wdescT = nullptr;
  int ndescT = 0, nworkT = 0;
  void* tdesc = nullptr; int tn = 0, ttotal = 0;
  const float* last_x = nullptr;
  int last_B = 0;
  bool last_training = false;   // the last forward kept what a backward pass reads (lse, x1, u_pre, batch statistics)
  // option "bn_frozen": a training forward normalises with the running statistics and leaves them alone (fine-tuning; the
  // BatchNorm is a per-channel affine map, its backward has no mean terms).  fwd_frozen: what the last training forward did -
  // the backward must find the option as that forward left ss
  bool bn_frozen = false, fwd_frozen = false;
  int dw_ksplit[5] = {256, 256, 256, 256, 256};
  // optional in-library kernel timing (bench.py roofline leg): hipEvent pairs around the
  // launches of ONE selected kernel kind, on the stream the kernels run on
  int prof_kind = -1;                       // a kernel kind, -1 = off, K_ALL = every kind (ral_profile_timeline)
  std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev;
  std::vector<std::pair<int, hipStream_t>> prof_meta;   // (kind, stream) of each recorded pair
  size_t prof_used = 0;
};

enum { K_QKV_FWD = 0, K_ATTN_FWD, K_MLP_FWD, K_MLP_BWD, K_ATTN_BWD, K_QKV_BWD, K_DW, K_RES_FWD, K_RES_BWD, K_STEM, K_NKINDS };
static const char* KIND_NAMES[K_NKINDS] = {"qkv_fwd", "attn_fwd", "mlp_fwd", "mlp_bwd", "attn_bwd", "qkv_bwd",
                                           "dw", "resample_fwd", "resample_bwd", "stem"};

enum { K_ALL = 1000 };
struct ProfScope {
  RalModel* m; hipStream_t s; bool on;
  ProfScope(RalModel* m_, int kind, hipStream_t s_) : m(m_), s(s_), on(m_->prof_kind == kind || m_->prof_kind == K_ALL) {
    if (!on) return;
    if (m->prof_used == m->prof_ev.size()) {
      hipEvent_t a = nullptr, b = nullptr;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {   // no timing for this launch
        if (a) (void)hipEventDestroy(a);
        on = false;
        return;
      }
      m->prof_ev.push_back({a, b});
      m->prof_meta.push_back({kind, s});
    }
    m->prof_meta[m->prof_used] = {kind, s};
    EV(hipEventRecord(m->prof_ev[m->prof_used].first, s));
  }
  ~ProfScope() {
    if (!on) return;
    EV(hipEventRecord(m->prof_ev[m->prof_used].second, s));
    m->prof_used++;
  }
};

// Attention backward scratch of the workspace, floats per window (E1 = 8 Lp floats per window and tensor): the (H, N, 2) =
// E1 / 2 floats the scalar-path sweeps hand over, or rows of table-gradient partials (2048 floats cover the scalar-path tail at
// H <= 16 and one row of any table the model has).  ral_create checks it against the plans (check_attn_scratch).
static constexpr size_t attn_scratch_per_window(size_t E1) { return E1 / 2 + 2048; }

static size_t plan_workspace(const ral_config& c, RalModel* m /* may be null: size only */, char* base) {
  size_t cur = 0;
  const int Lp = (c.L + 255) / 256 * 256;      // token slots per window (RalModel::Lp)
  const size_t B = c.max_batch, E = (size_t)8 * Lp * B;
  auto take = [&](const char* name, size_t nfloat) -> float* {
    float* p = base ? reinterpret_cast<float*>(base + cur) : nullptr;
    if (m && base) m->dbg[name] = {p, (int64_t)nfloat};
    cur += ((nfloat * sizeof(float)) + 255) & ~size_t(255);
    return p;
  };
  RalModel tmp_;
  RalModel& M = m ? *m : tmp_;
  for (int l = 0; l < 5; ++l) M.pe[l] = take(("pe" + std::to_string(l)).c_str(), (size_t)(Lp >> l) * CH[l]);
  M.a0 = take("a0", E); M.ten[RT_X0] = take(ralenet_tensor_name(RT_X0), E); M.ss = take("bn_ss", 64);
  const bool tr = c.train != 0;
  float *sh_qkv = nullptr, *sh_o = nullptr;
  if (!tr) { sh_qkv = take("qkv", 3 * E); sh_o = take("o", E); }
  for (int b = 0; b < 18; ++b) {
    const std::string p = "blk" + std::to_string(b) + ".";
    BlockAct& a = M.act[b];
    a.qkv = tr ? take((p + "qkv").c_str(), 3 * E) : sh_qkv;
    a.o = tr ? take((p + "o").c_str(), E) : sh_o;
    a.lse = tr ? take((p + "lse").c_str(), E / 4) : nullptr;
    a.x1 = tr ? take((p + "x1").c_str(), E) : nullptr;
    // u_pre is kept only where the backward reads it (the plan's stores_upre: a function of width, slots and mode alone)
    const int lvl = ralenet_stage(b / 2).level;
    const bool upre = block_plan(BlockShape{CH[lvl], Lp >> lvl, 0, tr, false, true, false, false}).stores_upre;
    a.upre = upre ? take((p + "upre").c_str(), 4 * E) : nullptr;
    a.out = take((p + "out").c_str(), E);
    if (b % 2) M.ten[RT_S0 + b / 2] = a.out;
  }
  { ParamLayout L_; ralenet_layout(c, L_); M.wh = reinterpret_cast<unsigned short*>(take("wh", (size_t)L_.nparam)); }
  M.wdesc = reinterpret_cast<int*>(take("wdesc", 4 * 64));
  M.ascale = take("ascale", 18 * ASC_N);
  M.adesc = reinterpret_cast<int*>(take("adesc", 18 * 12));
  for (const RalNode& nd : RAL_NET)
    if (nd.kind == RN_RES) M.ten[nd.out] = take(ralenet_tensor_name(nd.out), E);
  M.ten[RT_XMID] = take(ralenet_tensor_name(RT_XMID), E);
  if (tr) {
    for (int g = 0; g < RG_COUNT; ++g) {
      // x_mid = transformer(x4) + x4: the gradient of the bottleneck's output IS g x_mid (gin5) - gy9 names no buffer
      char name[8];
      ralenet_grad_name(g, name);
      M.gbuf[g] = ralenet_grad_is_buffer(g) ? take(name, E) : nullptr;
    }
    for (int k = 0; k < dw_sets(); ++k) {
      M.dx1[k] = take(("dx1_" + std::to_string(k)).c_str(), E); M.dohm[k] = take(("do_" + std::to_string(k)).c_str(), E);
      M.dqkv[k] = take(("dqkv_" + std::to_string(k)).c_str(), 3 * E); M.dupre[k] = take(("dupre_" + std::to_string(k)).c_str(), 4 * E);
      M.a2c0[k] = take(("a2c0_" + std::to_string(k)).c_str(), E / 8);
      M.astat[k] = take(("astat_" + std::to_string(k)).c_str(), B * attn_scratch_per_window((size_t)8 * Lp));
    }
    M.dz0 = take("dz0", E);
    ParamLayout L_; ralenet_layout(c, L_);
    M.paramsT = take("paramsT", (size_t)L_.nparam);
    M.whT = reinterpret_cast<unsigned short*>(take("whT", (size_t)L_.nparam));
    M.wdescT = reinterpret_cast<int*>(take("wdescT", 4 * 64));
    M.gmax = reinterpret_cast<unsigned*>(take("gmax", 18 * 4 * 4));
    M.tdesc = take("tdesc", 4 * 128);
  }
  return cur;
}

// The attention backward of every level must find its scratch in the workspace for any lane batch: a plan's need is at most
// B times its need at B = 1 (linear, or min(ceil(B c), ATTN_ROWS_MAX) rows), so one window's share has to cover B = 1.
static int check_attn_scratch(const RalModel* m) {
  for (int l = 0; l < 5; ++l) {
    const int N = m->Lp >> l, H = CH[l] / 4, NE = m->L >> l;
    for (int tab = 0; tab < 2; ++tab)
      for (int f16 = 0; f16 < 2; ++f16) {
        const int Len = tab && l < 4 && m->off.rwave ? RWLEN[l] : 0;
        const AttnPlan p = attn_bwd_plan(N, H, Len, f16, NE, 1);
        if (p.scratch_floats > attn_scratch_per_window(m->E1))
          return ral_fail("attention backward at N=%d H=%d Len=%d f16=%d (%s) needs %zu floats of scratch per window, the workspace has %zu",
                      N, H, Len, f16, p.name, p.scratch_floats, attn_scratch_per_window(m->E1));
      }
  }
  return 0;
}

static void choose_ksplit(RalModel* m) {
  // split-K workgroups of a fully sliced weight-gradient product per channel width {8,16,32,64,128} (products with
  // fewer slices get more, up to RAL_DW_MINWG workgroups per launch - see ral_dw.hip for why that is 192)
  static const int KS_DEFAULT[5] = {128, 128, 128, 64, 32};
  for (int l = 0; l < 5; ++l) m->dw_ksplit[l] = KS_DEFAULT[l];
}

// the Linear-layer dispatch of a block at level l under the handle's options (ral_block_plan.hpp; computed per call: a few
// dozen integer operations)
static BlockPlan level_plan(const RalModel* m, int l, bool training, bool second_out) {
  const int C = CH[l];
  const bool f16 = m->f16_split > 0;
  return block_plan(BlockShape{C, m->Lp >> l, m->L >> l, training, second_out, m->want_dw, f16 && C >= m->f16_split, f16 && m->narrow_f16});
}

static BlockP block_ptrs(const BlockOff& o, float* base) {
  BlockP p;
  p.wqkv = base + o.wqkv; p.bqkv = base + o.bqkv; p.wp = base + o.wp; p.bp = base + o.bp;
  p.ln1w = base + o.ln1w; p.ln1b = base + o.ln1b; p.ln2w = base + o.ln2w; p.ln2b = base + o.ln2b;
  p.w1 = base + o.w1; p.b1 = base + o.b1; p.w2 = base + o.w2; p.b2 = base + o.b2;
  p.le = o.le >= 0 ? base + o.le : nullptr;
  p.asc = nullptr;
  return p;
}

template <class T> static inline T* woff(T* p, int w0, size_t per_window) { return p ? p + (size_t)w0 * per_window : p; }

// ---------------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------------
static void run_block_fwd(RalModel* m, int bi, const float* in, bool training, const Lane& ln, const float* addend = nullptr, float* sum_out = nullptr) {
  const RalNode& st = ralenet_stage(bi / 2);
  const int l = st.level, C = CH[l], N = m->Lp >> l, H = C / 4;
  const size_t E1 = m->E1;
  BlockP w = block_ptrs(m->off.blk[bi], m->params);
  w.asc = m->f16_split > 0 ? m->ascale + ASC_N * bi : nullptr;
  BlockAct& a = m->act[bi];
  a.in = const_cast<float*>(in);   // base pointer (window 0); lanes offset it
  const float* table = nullptr;
  int Len = 0;
  if (m->off.rwave && st.rw) {
    table = m->params + m->off.rw[st.rw - 1];
    Len = RWLEN[st.rw - 1];
  }
  const int w0 = ln.w0, B = ln.B;
  hipStream_t s = ln.s;
  const BlockPlan plan = level_plan(m, l, training, sum_out != nullptr);
  const float* x = woff(in, w0, E1);
  float* qkv = woff(a.qkv, w0, 3 * E1);
  float* o = woff(a.o, w0, E1);
  { ProfScope p(m, K_QKV_FWD, s); launch_qkv_fwd(plan.qkv_fwd, x, m->pe[l], w, m->wh + 2 * m->off.blk[bi].wqkv, qkv, N, B, s); }
  const int NE = m->L >> l;   // existing tokens of the N slots (NE < N: a window length that is not a multiple of 256)
  { ProfScope p(m, K_ATTN_FWD, s);
    launch_attn_fwd(attn_fwd_plan(N, H, Len, (m->f16_split > 0 && m->attn_f16) ? 1 : 0, NE), qkv, o,
                    training ? woff(a.lse, w0, E1 / 4) : nullptr, table, N, H, Len, B, s, NE); }
  { ProfScope p(m, K_MLP_FWD, s);
    launch_mlp_fwd(plan.mlp_fwd, x, o, w, m->params, m->wh, training ? woff(a.x1, w0, E1) : nullptr,
                   plan.stores_upre ? woff(a.upre, w0, 4 * E1) : nullptr,
                   woff(a.out, w0, E1), N, B, s, NE, woff(addend, w0, E1), woff(sum_out, w0, E1)); }
}

// a stage with an addend (the bottleneck: x_mid = transformer(x4) + x4, raletransformer.py:659) leaves the sum as the second
// output of its last MLP kernel
static void run_stage_fwd(RalModel* m, int si, const float* in, const float* addend, float* sum_out, bool training, const Lane& ln) {
  run_block_fwd(m, si * 2, in, training, ln);
  run_block_fwd(m, si * 2 + 1, m->act[si * 2].out, training, ln, addend, addend ? sum_out : nullptr);
}

static void run_res_fwd(RalModel* m, const RalNode& nd, const float* in, const float* skip, float* out, const Lane& ln) {
  const ResOff& r = m->off.res[nd.idx];
  const int T = m->E1 / r.D, Tv = 8 * m->L / r.D;  // output token slots per window, and how many of them exist
  ProfScope p(m, K_RES_FWD, ln.s);
  launch_resample_fwd(r.D, nd.up, woff(in, ln.w0, m->E1), m->params + r.w, m->params + r.lnw, m->params + r.lnb,
                      woff(skip, ln.w0, m->E1), woff(out, ln.w0, m->E1), T, Tv, ln.B, ln.s);
}

// split [0, B) over the lanes; lane 0 runs on the caller's stream
static int plan_lanes(RalModel* m, int B, hipStream_t s) {
  LaneSet* L = m->lanes;
  const RalLaneSplit sp = ralenet_lane_split(B, m->n_lanes);
  const int n = sp.n;
  for (int i = 0; i < n; ++i) {
    Lane& ln = L->l[i];
    ln.w0 = sp.w0[i]; ln.B = sp.B[i];
    ln.s = i == 0 ? s : L->own[i];
    ln.bwd_count = 0;
    for (int k = 0; k < MAX_SETS; ++k) ln.dw_pending[k] = false;
  }
  L->n = n;
  return n;
}

static void fork_lanes(RalModel* m, hipStream_t s) {     // lanes 1.. start after everything queued on s so far
  LaneSet* L = m->lanes;
  if (L->n < 2) return;
  EV(hipEventRecord(L->l[0].ev_fork, s));
  for (int i = 1; i < L->n; ++i) EV(hipStreamWaitEvent(L->l[i].s, L->l[0].ev_fork, 0));
}
static void join_lanes(RalModel* m, hipStream_t s) {     // s continues after every lane has finished
  LaneSet* L = m->lanes;
  for (int i = 1; i < L->n; ++i) {
    EV(hipEventRecord(L->l[i].ev_join, L->l[i].s));
    EV(hipStreamWaitEvent(s, L->l[i].ev_join, 0));
  }
}

static int fwd_begin(RalModel* m, const float* x, int B, int training, hipStream_t s) {
  sched_reset();
  if (!m->params || !m->state) return ral_fail("ral_bind was not called");
  if (B <= 0 || B > m->cfg.max_batch) return ral_fail("batch %d outside (0, max_batch=%d]", B, m->cfg.max_batch);
  if (training && !m->cfg.train) return ral_fail("handle was created with train=0");
  if (training && !m->bn_sums) return ral_fail("training forward needs bn_sums bound");
  const RalOff& Y = m->off;
  m->last_x = x; m->last_B = B; m->last_training = training != 0;
  m->fwd_frozen = training && m->bn_frozen;
  m->prep_fwd = m->prep_bwd = false;
  m->prep_stale = false;
  m->skip_prep = !training && m->static_params && m->planes_valid;
  if (training) m->planes_valid = false;                         // (an optimiser step will follow)
  else if (m->static_params) m->planes_valid = true;             // (what this forward prepares stays)
  if (!m->skip_prep && m->side_stream && m->ev_prep_go) {
    hipStream_t ps = m->lanes->l[0].s2;
    HIP_OK(hipEventRecord(m->ev_prep_go, s));            // (the parameters are final: everything queued on s so far has run)
    HIP_OK(hipStreamWaitEvent(ps, m->ev_prep_go, 0));
    if (m->f16_split > 0) {
      launch_act_scales(m->params, m->adesc, m->ascale, 18, ps);
      launch_tile_planes(m->params, m->wh, m->wdesc, m->ndesc, m->nwork, 0, ps);
    }
    HIP_OK(hipEventRecord(m->ev_prep_fwd, ps));
    m->prep_fwd = true;
    if (training) {
      launch_transpose_mats(m->params, m->paramsT, m->tdesc, m->tn, m->ttotal, ps);
      if (m->f16_split > 0) launch_tile_planes(m->paramsT, m->whT, m->wdescT, m->ndescT, m->nworkT, 1, ps);
      HIP_OK(hipEventRecord(m->ev_prep_bwd, ps));
      m->prep_bwd = true;
    }
  }
  if (training) {
    if (!m->sums_clean) HIP_OK(hipMemsetAsync(m->bn_sums, 0, 64 * sizeof(double), s));
    m->sums_clean = false;
    if (m->fwd_frozen)   // (nothing adds to the sums: they stay zero for whoever all-reduces them)
      launch_conv1_fwd(m->cfg.leads, 2, x, m->params + Y.conv1_w, m->params + Y.conv1_b, m->a0, nullptr, m->params + Y.bn_w,
                       m->params + Y.bn_b, m->state, m->state + 8, m->L, m->Lp, B, s, m->ten[RT_X0], m->ss);
    else
      launch_conv1_fwd(m->cfg.leads, 0, x, m->params + Y.conv1_w, m->params + Y.conv1_b, m->a0, m->bn_sums, nullptr,
                       nullptr, nullptr, nullptr, m->L, m->Lp, B, s);
  } else {
    launch_conv1_fwd(m->cfg.leads, 1, x, m->params + Y.conv1_w, m->params + Y.conv1_b, m->ten[RT_X0], nullptr,
                     m->params + Y.bn_w, m->params + Y.bn_b, m->state, m->state + 8, m->L, m->Lp, B, s);
  }
  return 0;
}

static int fwd_end(RalModel* m, float* y, int B, int64_t global_windows, int training, hipStream_t s) {
  sched_reset();
  const RalOff& Y = m->off;
  if (training && !m->fwd_frozen) {
    launch_bn_train8(m->bn_sums, (double)global_windows * m->L, m->params + Y.bn_w, m->params + Y.bn_b, m->ss,
                     m->state, m->state + 8, m->a0, m->ten[RT_X0], (size_t)B * m->Lp, s);
  }
  const bool tr = training != 0;
  // (the activation scales and the split planes of the wide levels' weights: formed under the stem on an idle stream.  ONE join, here,
  // in front of the fork: waiting for the planes only in front of the first wide level - an edge from the preparation stream into each
  // lane - gained nothing measurable on the eager step, and the hipGraph replay of the forward measured 457 k windows/s against 541 k
  // eager with it in the round-6 collection (572 k / 563 k without it))
  if (m->prep_fwd) { HIP_OK(hipStreamWaitEvent(s, m->ev_prep_fwd, 0)); m->prep_fwd = false; }
  else if (m->f16_split > 0 && !m->skip_prep) {
    launch_act_scales(m->params, m->adesc, m->ascale, 18, s);
    launch_tile_planes(m->params, m->wh, m->wdesc, m->ndesc, m->nwork, 0, s);
  }
  const int nl = plan_lanes(m, B, s);
  fork_lanes(m, s);
  LaneSet* LS = m->lanes;
  // issue node by node, alternating lanes, so that the lanes progress together
  for (int e = 0; e < RAL_NODES; ++e) {
    const RalNode& nd = RAL_NET[ralenet_pass(false, e).node];
    const RalBinding b = ralenet_bind(nd, false);
    const float *in = m->ten[b.in], *add = b.extra == RT_NONE ? nullptr : m->ten[b.extra];
    for (int k = 0; k < nl; ++k) {
      if (nd.kind == RN_STAGE) run_stage_fwd(m, nd.idx, in, add, m->ten[b.out], tr, LS->l[k]);
      else run_res_fwd(m, nd, in, add, m->ten[b.out], LS->l[k]);
    }
  }
  for (int k = 0; k < nl; ++k) {
    const Lane& ln = LS->l[k];
    launch_final_fwd(m->cfg.leads, woff(m->ten[RAL_HEAD_IN], ln.w0, m->E1), woff(m->ten[RAL_HEAD_ADD], ln.w0, m->E1), m->params + Y.tc_w, m->params + Y.tc_b,
                     woff(y, ln.w0, (size_t)m->cfg.leads * m->L), m->L, m->Lp, ln.B, ln.s);
  }
  join_lanes(m, s);
  HIP_OK(hipGetLastError());
  return sched_check();
}

// ---------------------------------------------------------------------------------
// backward
// ---------------------------------------------------------------------------------
// one block: dy (grad of block output) -> dx (grad of block input) [+ extra]; all pointers are window-0 bases
// (non-zero: the attention backward found the workspace scratch smaller than its plan needs - its gradients were not computed)
static int run_block_bwd(RalModel* m, int bi, const float* dy, const float* extra, float* dx, Lane& ln, int lane) {
  const RalNode& st = ralenet_stage(bi / 2);
  const int l = st.level, C = CH[l], N = m->Lp >> l, H = C / 4;
  const size_t E1 = m->E1;
  BlockP w = block_ptrs(m->off.blk[bi], m->params);
  w.asc = m->f16_split > 0 ? m->ascale + ASC_N * bi : nullptr;
  const BlockP g = block_ptrs(m->off.blk[bi], m->grads);
  const BlockP wt = block_ptrs(m->off.blk[bi], m->paramsT);
  BlockAct& a = m->act[bi];
  const float* table = nullptr;
  float* gtable = nullptr;
  int Len = 0;
  if (m->off.rwave && st.rw) {
    table = m->params + m->off.rw[st.rw - 1];
    gtable = m->grads + m->off.rw[st.rw - 1];
    Len = RWLEN[st.rw - 1];
  }
  const int w0 = ln.w0, B = ln.B;
  hipStream_t s = ln.s;
  const int k = ln.bwd_count++ % dw_sets();            // temporary set of this block
  const bool side = m->side_stream && m->want_dw;
  hipStream_t sd = side ? ln.s2 : s;                   // stream of the weight-gradient kernels
  if (side && ln.dw_pending[k]) EV(hipStreamWaitEvent(s, ln.ev_done[k], 0));   // set k free again?
  const float* dyw = woff(dy, w0, E1);
  float *dupre = woff(m->dupre[k], w0, 4 * E1), *dx1 = woff(m->dx1[k], w0, E1), *dohm = woff(m->dohm[k], w0, E1),
        *dqkv = woff(m->dqkv[k], w0, 3 * E1), *a2c0 = woff(m->a2c0[k], w0, m->Lp);   // (per-window stride L at every level: the lanes run different levels concurrently)
  const float *x1 = woff(a.x1, w0, E1), *upre = woff(a.upre, w0, 4 * E1), *qkv = woff(a.qkv, w0, 3 * E1),
              *o = woff(a.o, w0, E1), *lse = woff(a.lse, w0, E1 / 4), *xin = woff(a.in, w0, E1);
  const BlockPlan plan = level_plan(m, l, true, false);
  // maxima of this block's gradient tensors (this lane's windows), for the split weight-gradient products
  unsigned* gmax = plan.dw_split ? m->gmax + ((size_t)bi * 4 + lane) * 4 : nullptr;
  const int NE = m->L >> l;
  { ProfScope p(m, K_MLP_BWD, s);
    launch_mlp_bwd(plan.mlp_bwd, dyw, x1, upre, w, wt, m->paramsT, m->whT, gmax, g, dupre, dx1, dohm, a2c0, N, B, m->want_dw, s, NE); }
  // the R-wave table gradient leaves the one-sweep attention kernels as one row of partials per workgroup; the kernel that adds
  // the rows up runs with the block's weight-gradient kernels (side stream), not on the chain: nothing on the chain reads it
  AttnTabReduce tabred{nullptr, nullptr, 0, 0};
  static const bool tab_side = ral_knob("TABRED_SIDE", 1) != 0;
  int short_scratch;
  { ProfScope p(m, K_ATTN_BWD, s);
    const size_t per_window = attn_scratch_per_window(E1);   // (each lane's scratch: its windows' share)
    short_scratch = launch_attn_bwd(attn_bwd_plan(N, H, Len, (m->f16_split > 0 && m->attn_f16) ? 1 : 0, NE, B), qkv, o, dohm, lse, table,
                                    gtable, dqkv, m->astat[k] + (size_t)w0 * per_window, (size_t)B * per_window, N, H, Len, B, s, NE,
                                    side && tab_side ? &tabred : nullptr); }
  { ProfScope p(m, K_QKV_BWD, s);
    launch_qkv_bwd(plan.qkv_bwd, dqkv, xin, m->pe[l], dx1, woff(extra, w0, E1), w, wt, m->paramsT, m->whT, gmax, g, woff(dx, w0, E1), N, B, s); }
  if (!m->want_dw) return short_scratch;
  if (side) {
    EV(hipEventRecord(ln.ev_ready[k], s));
    EV(hipStreamWaitEvent(sd, ln.ev_ready[k], 0));
  }
  if (tabred.ntab > 0) launch_attn_tpart_reduce(tabred, sd);
  { ProfScope p(m, K_DW, sd);
    launch_block_dw(plan, dyw, upre, w.le ? a2c0 : nullptr, dupre, x1, dx1, o, dqkv, xin, m->pe[l], w, g, N, B, m->dw_ksplit[l], gmax, sd); }
  if (side) { EV(hipEventRecord(ln.ev_done[k], sd)); ln.dw_pending[k] = true; }
  return short_scratch;
}

// stage: grad of stage output `dy` -> grad of stage input written to `dx` (+extra). Uses `tmp` between blocks.
static int run_stage_bwd(RalModel* m, int si, const float* dy, const float* extra, float* tmp, float* dx, Lane& ln, int lane) {
  const int rc = run_block_bwd(m, si * 2 + 1, dy, nullptr, tmp, ln, lane);
  return run_block_bwd(m, si * 2, tmp, extra, dx, ln, lane) | rc;
}

static void run_res_bwd(RalModel* m, const RalNode& nd, const float* dy, const float* in, float* dx, Lane& ln) {
  const ResOff& r = m->off.res[nd.idx];
  const int T = m->E1 / r.D, Tv = 8 * m->L / r.D;
  const size_t E1 = m->E1;
  hipStream_t s = ln.s;
  { ProfScope p(m, K_RES_BWD, s);
    launch_resample_bwd(r.D, nd.up, woff(dy, ln.w0, E1), woff(in, ln.w0, E1), m->paramsT + r.w, m->params + r.lnw,
                        m->grads + r.lnw, m->grads + r.lnb, woff(dx, ln.w0, E1), T, Tv, ln.B, s); }
  if (!m->want_dw) return;
  int lvl = 0;
  while ((8 << lvl) < r.D) ++lvl;
  hipStream_t sd = s;
  if (m->side_stream) {   // dy was produced on s: fork the weight-gradient product to the side stream
    EV(hipEventRecord(ln.ev_fork, s));
    EV(hipStreamWaitEvent(ln.s2, ln.ev_fork, 0));
    sd = ln.s2;
  }
  launch_resample_dw(r.D, nd.up, woff(dy, ln.w0, E1), woff(in, ln.w0, E1), m->params + r.lnw, m->params + r.lnb,
                     m->grads + r.w, T, Tv, ln.B, m->dw_ksplit[lvl], sd);
}

static int bwd_begin(RalModel* m, const float* dy, int B, hipStream_t s) {
  sched_reset();
  if (!m->cfg.train) return ral_fail("handle was created with train=0");
  if (!m->grads || !m->bn_sums) return ral_fail("ral_bind: grads / bn_sums not bound");
  if (B != m->last_B) return ral_fail("backward batch %d != forward batch %d", B, m->last_B);
  if (!m->last_training) return ral_fail("RA-LENet backward must follow a training forward: the last forward was an eval one");
  if (m->fwd_frozen != m->bn_frozen) return ral_fail("RA-LENet backward: bn_frozen changed since the last forward (run the forward again)");
  const RalOff& Y = m->off;
  launch_zero_bwd(m->grads, (size_t)m->lay.nparam, m->bn_sums + 32, 32, m->gmax, 18 * 4 * 4, s);   // gradient buffer, backward BatchNorm sums, gradient maxima
  const bool prep_ok = m->prep_bwd && !m->prep_stale;
  if (m->prep_bwd) { HIP_OK(hipStreamWaitEvent(s, m->ev_prep_bwd, 0)); m->prep_bwd = false; }   // transposes + their planes: formed during the forward
  if (!prep_ok) {   // (... or formed from parameters / for options that have changed since: after them, again, from what is bound now)
    launch_transpose_mats(m->params, m->paramsT, m->tdesc, m->tn, m->ttotal, s);
    if (m->f16_split > 0) {
      launch_tile_planes(m->paramsT, m->whT, m->wdescT, m->ndescT, m->nworkT, 1, s);
      if (m->prep_stale) launch_act_scales(m->params, m->adesc, m->ascale, 18, s);   // (the weight-gradient products scale their activation operands)
    }
  }
  const int nl = plan_lanes(m, B, s);
  LaneSet* LS = m->lanes;
  fork_lanes(m, s);
  // output conv: dy -> d(u0 + x0), each lane its windows
  for (int k = 0; k < nl; ++k) {
    const Lane& ln = LS->l[k];
    launch_final_bwd(m->cfg.leads, woff(dy, ln.w0, (size_t)m->cfg.leads * m->L), woff(m->ten[RAL_HEAD_IN], ln.w0, m->E1), woff(m->ten[RAL_HEAD_ADD], ln.w0, m->E1),
                     m->params + Y.tc_w, m->grads + Y.tc_w, m->grads + Y.tc_b, woff(m->gbuf[ralenet_grad_of(RAL_HEAD_IN)], ln.w0, m->E1), m->L, m->Lp, ln.B, ln.s);
  }
  const bool side = m->side_stream && m->want_dw;
  if (side)   // side streams start after the gradient buffer has been zeroed
    for (int k = 0; k < nl; ++k) {
      EV(hipEventRecord(LS->l[k].ev_fork, LS->l[k].s));
      EV(hipStreamWaitEvent(LS->l[k].s2, LS->l[k].ev_fork, 0));
    }
  int short_scratch = 0;
  // node by node in reverse, every lane of a node before the next; a stage adds `extra`, the gradient its input tensor receives
  // as some node's addend (ralenet_extra_of), in its first block
  for (int e = 0; e < RAL_NODES; ++e) {
    const RalPassEntry pe = ralenet_pass(true, e);
    const RalNode& nd = RAL_NET[pe.node];
    const RalBinding b = ralenet_bind(nd, true);
    const float *gout = m->gbuf[b.in], *extra = b.extra == RG_NONE ? nullptr : m->gbuf[b.extra];
    float* tmp = nd.kind == RN_STAGE ? m->gbuf[ralenet_gy(nd.idx, 0)] : nullptr;
    for (int k = 0; k < nl; ++k) {
      Lane& ln = LS->l[k];
      if (nd.kind == RN_STAGE) short_scratch |= run_stage_bwd(m, nd.idx, gout, extra, tmp, m->gbuf[b.out], ln, k);
      else run_res_bwd(m, nd, gout, m->ten[b.fwd_in], m->gbuf[b.out], ln);
    }
    if (!pe.mark) continue;
    // the decoder's parameters (utransformer4 .. transconv: the upper half of the flat gradient buffer) have their
    // final gradients once every lane's chain and weight-gradient stream pass this point: gradient bucket 1
    for (int k = 0; k < nl; ++k) {
      Lane& ln = LS->l[k];
      EV(hipEventRecord(ln.ev_dec_main, ln.s));
      if (side) EV(hipEventRecord(ln.ev_dec_side, ln.s2));
    }
    m->dec_lanes = nl; m->dec_side = side;
  }
  if (side)   // join the side streams into their lanes, then the lanes into s
    for (int k = 0; k < nl; ++k) {
      EV(hipEventRecord(LS->l[k].ev_join, LS->l[k].s2));
      EV(hipStreamWaitEvent(LS->l[k].s, LS->l[k].ev_join, 0));
    }
  join_lanes(m, s);
  if (!m->fwd_frozen) launch_bn8_bwd_stats(m->gbuf[ralenet_grad_of(RT_X0)], m->a0, m->ss, m->bn_sums + 32, (size_t)B * m->Lp, s);
  HIP_OK(hipGetLastError());
  if (short_scratch) return ral_fail("attention backward: the workspace scratch is smaller than a plan needs (ral_create checks it: the ATTN_* switches changed since?)");
  return sched_check();
}

static int bwd_end(RalModel* m, float* dx, int B, int64_t global_windows, hipStream_t s) {
  sched_reset();
  const RalOff& Y = m->off;
  if (m->fwd_frozen)   // (per-window constants: the sums over this rank's windows are this rank's whole share)
    launch_conv1_bwd_frozen(m->cfg.leads, m->gbuf[ralenet_grad_of(RT_X0)], m->a0, m->last_x, m->ss, m->params + Y.bn_w,
                            m->grads + Y.conv1_w, m->grads + Y.conv1_b, dx ? m->dz0 : nullptr, m->L, m->Lp, B, s,
                            m->grads + Y.bn_w, m->grads + Y.bn_b);
  else
    launch_conv1_bwd(m->cfg.leads, m->gbuf[ralenet_grad_of(RT_X0)], m->a0, m->last_x, m->ss, m->params + Y.bn_w, m->bn_sums + 32,
                     (double)global_windows * m->L, m->grads + Y.conv1_w, m->grads + Y.conv1_b, dx ? m->dz0 : nullptr,
                     m->L, m->Lp, B, s, m->grads + Y.bn_w, m->grads + Y.bn_b, (double)B / (double)global_windows);
  if (dx) launch_conv1_bwd_dx(m->cfg.leads, m->dz0, m->params + Y.conv1_w, dx, m->L, m->Lp, B, s);
  HIP_OK(hipEventRecord(m->ev_bwd_done, s));
  m->bwd_recorded = true;
  HIP_OK(hipGetLastError());
  return sched_check();
}


RalModel* ralenet_model(ral_handle* h) { return dynamic_cast<RalModel*>(h); }

int ralenet_pe_table(const ral_config* cfg, int level, float* out_host, int64_t cap) {
  if (level < 0 || level > 4) return ral_fail("no PE table for this variant/level");
  const int n = cfg->L >> level, C = CH[level];
  if (cap < (int64_t)n * C) return ral_fail("buffer too small");
  fill_pe(out_host, n, C);
  return 0;
}

// every stream and event of a model is released here (the base releases the workspace after them): ral_destroy and the
// error paths of init() share it
RalModel::~RalModel() {
  RalModel* const m = this;
  if (m->lanes) {
    LaneSet* LS = m->lanes;
    for (int i = 0; i < MAX_LANES; ++i) {
      Lane& ln = LS->l[i];
      if (LS->own[i]) (void)hipStreamDestroy(LS->own[i]);
      if (ln.s2) (void)hipStreamDestroy(ln.s2);
      hipEvent_t evs[4] = {ln.ev_fork, ln.ev_join, ln.ev_dec_main, ln.ev_dec_side};
      for (hipEvent_t e : evs) if (e) (void)hipEventDestroy(e);
      for (int k = 0; k < MAX_SETS; ++k) {
        if (ln.ev_ready[k]) (void)hipEventDestroy(ln.ev_ready[k]);
        if (ln.ev_done[k]) (void)hipEventDestroy(ln.ev_done[k]);
      }
    }
    delete LS;
  }
  for (auto& pr : m->prof_ev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
  if (m->ev_bwd_done) (void)hipEventDestroy(m->ev_bwd_done);
  for (hipEvent_t e : {m->ev_prep_go, m->ev_prep_fwd, m->ev_prep_bwd}) if (e) (void)hipEventDestroy(e);
}

int RalModel::init() {
  RalModel* const m = this;
  m->L = cfg.L;
  m->Lp = (cfg.L + 255) / 256 * 256;
  m->E1 = 8 * m->Lp;
  build_layout(cfg, m->lay, m->off);
  if (cfg.train && check_attn_scratch(m)) return -1;
  m->slab_bytes = plan_workspace(cfg, nullptr, nullptr);
  hipError_t e = alloc_slab(m->slab_bytes);
  if (e != hipSuccess) return ral_fail("hipMalloc(%zu bytes) failed: %s", m->slab_bytes, hipGetErrorString(e));
  plan_workspace(cfg, m, m->slab);
  choose_ksplit(m);
  {
    LaneSet* LS = new LaneSet();
    m->lanes = LS;
    m->n_lanes = ral_env_int("RAL_LANES", 2, 1, MAX_LANES);        // one of the TWO environment variables the library reads
    // (the weight-gradient streams s2 run at the default priority, like the chains.)  A failed creation would leave a null stream (= the legacy default stream: the fork/join ordering would silently
    // change), so the first error fails the whole ral_create
    hipError_t first = hipSuccess;
    auto ok = [&](hipError_t r) { if (r != hipSuccess && first == hipSuccess) first = r; };
    for (int i = 0; i < MAX_LANES; ++i) {
      Lane& ln = LS->l[i];
      if (i > 0) ok(hipStreamCreateWithFlags(&LS->own[i], hipStreamNonBlocking));
      ok(hipStreamCreateWithFlags(&ln.s2, hipStreamNonBlocking));
      for (int k = 0; k < MAX_SETS; ++k) {
        ok(hipEventCreateWithFlags(&ln.ev_ready[k], hipEventDisableTiming));
        ok(hipEventCreateWithFlags(&ln.ev_done[k], hipEventDisableTiming));
      }
      ok(hipEventCreateWithFlags(&ln.ev_fork, hipEventDisableTiming));
      ok(hipEventCreateWithFlags(&ln.ev_join, hipEventDisableTiming));
      ok(hipEventCreateWithFlags(&ln.ev_dec_main, hipEventDisableTiming));
      ok(hipEventCreateWithFlags(&ln.ev_dec_side, hipEventDisableTiming));
    }
    ok(hipEventCreateWithFlags(&m->ev_bwd_done, hipEventDisableTiming));
    ok(hipEventCreateWithFlags(&m->ev_prep_go, hipEventDisableTiming));
    ok(hipEventCreateWithFlags(&m->ev_prep_fwd, hipEventDisableTiming));
    ok(hipEventCreateWithFlags(&m->ev_prep_bwd, hipEventDisableTiming));
    if (first != hipSuccess) return ral_fail("stream / event creation failed: %s", hipGetErrorString(first));
  }
  for (int l = 0; l < 5; ++l) {
    const int n = m->Lp >> l, C = CH[l];
    std::vector<float> P((size_t)n * C);
    fill_pe(P.data(), n, C);
    e = hipMemcpy(m->pe[l], P.data(), P.size() * sizeof(float), hipMemcpyHostToDevice);
    if (e != hipSuccess) return ral_fail("hipMemcpy(pe) failed: %s", hipGetErrorString(e));
  }
  {   // descriptors of the activation-scale kernel
    std::vector<int> d;
    for (int b = 0; b < 18; ++b) {
      const BlockOff& o = m->off.blk[b];
      const int v[12] = {CH[ralenet_stage(b / 2).level], (int)o.ln1w, (int)o.ln1b, (int)o.wqkv, (int)o.bqkv, (int)o.ln2w, (int)o.ln2b, (int)o.w1, (int)o.b1,
                         (int)o.le, 0, 0};
      d.insert(d.end(), v, v + 12);
    }
    e = hipMemcpy(m->adesc, d.data(), d.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return ral_fail("hipMemcpy(adesc) failed: %s", hipGetErrorString(e));
  }
  m->f16_split = (int)ral_knob("F16_SPLIT", m->f16_split);   // (a process-wide default for tests: ral_global_option; never the environment)
  if (m->L != m->Lp) m->f16_split = 0;   // padded windows run on the generic fp32-MFMA kernels (the ones that know where a window ends)
  m->attn_f16 = attn_f16_default() != 0;
  if (cfg.train) {
    m->side_stream = ral_env_int("RAL_NO_SIDE_STREAM", 0, 0, 1) == 0;   // ... and the other
    std::vector<int> d;
    const int run = ralenet_mat_descs(m->off, false, false, 1, true, d);
    m->tn = (int)d.size() / 4; m->ttotal = run;
    e = hipMemcpy(m->tdesc, d.data(), d.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e != hipSuccess) return ral_fail("hipMemcpy(tdesc) failed: %s", hipGetErrorString(e));
  }
  {   // weight matrices that are re-written as tiled split planes every forward (widths with a split-operand kernel)
    std::vector<int> d;
    const int run = ralenet_mat_descs(m->off, true, false, 8, false, d);
    m->ndesc = (int)d.size() / 4; m->nwork = run;
    if (cfg.train) {   // transposed matrices of the backward's data-gradient products (rows x columns as they sit in paramsT)
      std::vector<int> dt;
      const int runT = ralenet_mat_descs(m->off, true, true, 8, false, dt);
      m->ndescT = (int)dt.size() / 4; m->nworkT = runT;
      if (m->ndescT) {
        e = hipMemcpy(m->wdescT, dt.data(), dt.size() * sizeof(int), hipMemcpyHostToDevice);
        if (e != hipSuccess) return ral_fail("hipMemcpy(wdescT) failed: %s", hipGetErrorString(e));
      }
    }
    if (m->ndesc > 64) return ral_fail("too many split-plane descriptors");
    if (m->ndesc) {
      e = hipMemcpy(m->wdesc, d.data(), d.size() * sizeof(int), hipMemcpyHostToDevice);
      if (e != hipSuccess) return ral_fail("hipMemcpy(wdesc) failed: %s", hipGetErrorString(e));
    }
  }
  return 0;
}

int RalModel::bind(float* params_, float* grads_, float* am_, float* av_, float* state_, double* bn_sums_) {
  prep_stale = true;
  sums_clean = false;
  planes_valid = false;
  return ral_handle::bind(params_, grads_, am_, av_, state_, bn_sums_);
}

int RalModel::forward(const float* x, float* y, int B, int training, hipStream_t s) {
  if (fwd_begin(this, x, B, training, s)) return -1;
  return fwd_end(this, y, B, B, training, s);
}

int RalModel::backward(const float* dy, float* dx, int B, hipStream_t s) {
  if (!dy) return ral_fail("ral_backward: dy is NULL");
  if (bwd_begin(this, dy, B, s)) return -1;
  return bwd_end(this, dx, B, B, s);
}

int ralenet_forward_begin(RalModel* m, const float* x, int B, hipStream_t s) { return fwd_begin(m, x, B, 1, s); }
int ralenet_forward_end(RalModel* m, float* y, int B, int64_t global_windows, hipStream_t s) { return fwd_end(m, y, B, global_windows, 1, s); }
int ralenet_backward_begin(RalModel* m, const float* dy, int B, bool want_dw, hipStream_t s) {
  m->want_dw = want_dw;
  const int rc = bwd_begin(m, dy, B, s);
  m->want_dw = true;
  return rc;
}
int ralenet_backward_end(RalModel* m, float* dx, int B, int64_t global_windows, hipStream_t s) { return bwd_end(m, dx, B, global_windows, s); }

double* RalModel::after_adam() {
  prep_stale = true;
  planes_valid = false;
  if (bn_sums) sums_clean = true;   // (the next step's stem starts from cleared sums)
  return bn_sums;
}

int RalModel::set_option(const char* key, int value) {
  RalModel* const m = this;
  if (!strcmp(key, "bn_frozen")) {   // (no arithmetic of the transformer stack depends on it: the weight planes stay valid)
    if (value != 0 && value != 1) return ral_fail("option bn_frozen must be 0 or 1 (got %d)", value);
    m->bn_frozen = value != 0;
    return 0;
  }
  m->prep_stale = true;   // (weight planes queued by a forward were formed for the options of that moment)
  m->planes_valid = false;
  if (!strcmp(key, "static_params")) { m->static_params = value != 0; return 0; }   // (setting it again = "the parameters have changed")
  if (!strcmp(key, "lanes")) { m->n_lanes = value < 1 ? 1 : (value > MAX_LANES ? MAX_LANES : value); return 0; }
  if (!strcmp(key, "side_stream")) { m->side_stream = value != 0; return 0; }
  if (!strcmp(key, "f16_split")) {
    if (value > 0 && m->L != m->Lp) return ral_fail("f16_split > 0 needs a window length that is a multiple of 256 (L = %d runs on padded windows, fp32 MFMA)", m->L);
    m->f16_split = value; return 0;
  }
  if (!strcmp(key, "attn_f16")) { m->attn_f16 = value != 0; return 0; }
  if (!strcmp(key, "narrow_f16")) { m->narrow_f16 = value != 0; return 0; }
  return ral_fail("unknown option %s", key);
}

int ralenet_grad_bucket(RalModel* m, int k, int64_t* offset, int64_t* count) {
  if (k < 0 || k > 1 || !offset || !count) return ral_fail("gradient bucket index must be 0 or 1");
  *offset = k == 0 ? 0 : m->off.dec_off;
  *count = k == 0 ? m->off.dec_off : m->lay.nparam - m->off.dec_off;
  return 0;
}

int ralenet_grad_bucket_wait(RalModel* m, int k, hipStream_t s) {
  if (k == 1) {
    if (m->dec_lanes <= 0) return ral_fail("bucket 1 is available after ral_backward_begin");
    LaneSet* LS = m->lanes;
    for (int i = 0; i < m->dec_lanes; ++i) {
      HIP_OK(hipStreamWaitEvent(s, LS->l[i].ev_dec_main, 0));
      if (m->dec_side) HIP_OK(hipStreamWaitEvent(s, LS->l[i].ev_dec_side, 0));
    }
    return 0;
  }
  if (k == 0) {
    if (!m->bwd_recorded) return ral_fail("bucket 0 is available after ral_backward_end");
    HIP_OK(hipStreamWaitEvent(s, m->ev_bwd_done, 0));
    return 0;
  }
  return ral_fail("gradient bucket index must be 0 or 1");
}

int ralenet_profile_select(RalModel* m, const char* kind) {
  m->prof_used = 0;
  m->prof_kind = -1;
  if (!kind || !*kind) return 0;
  if (!strcmp(kind, "*")) { m->prof_kind = K_ALL; return 0; }
  for (int k = 0; k < K_NKINDS; ++k)
    if (!strcmp(kind, KIND_NAMES[k])) { m->prof_kind = k; return 0; }
  return ral_fail("unknown kernel kind %s", kind);
}

int ralenet_profile_read(RalModel* m, double* total_ms, int64_t* launches) {
  double tot = 0.0;
  for (size_t i = 0; i < m->prof_used; ++i) {
    float ms = 0.f;
    HIP_OK(hipEventSynchronize(m->prof_ev[i].second));
    HIP_OK(hipEventElapsedTime(&ms, m->prof_ev[i].first, m->prof_ev[i].second));
    tot += ms;
  }
  *total_ms = tot;
  *launches = (int64_t)m->prof_used;
  m->prof_used = 0;
  return 0;
}

int ralenet_profile_timeline(RalModel* m, double* rows, int64_t cap_rows, int64_t* nrows) {
  *nrows = (int64_t)m->prof_used;
  if ((int64_t)m->prof_used > cap_rows) return ral_fail("timeline: %zu rows, room for %lld", m->prof_used, (long long)cap_rows);
  std::vector<hipStream_t> streams;
  for (size_t i = 0; i < m->prof_used; ++i) {
    HIP_OK(hipEventSynchronize(m->prof_ev[i].second));
    float t0 = 0.f, t1 = 0.f;
    HIP_OK(hipEventElapsedTime(&t0, m->prof_ev[0].first, m->prof_ev[i].first));
    HIP_OK(hipEventElapsedTime(&t1, m->prof_ev[0].first, m->prof_ev[i].second));
    size_t si = 0;
    while (si < streams.size() && streams[si] != m->prof_meta[i].second) ++si;
    if (si == streams.size()) streams.push_back(m->prof_meta[i].second);
    rows[4 * i] = m->prof_meta[i].first; rows[4 * i + 1] = (double)si; rows[4 * i + 2] = t0; rows[4 * i + 3] = t1;
  }
  m->prof_used = 0;
  return 0;
}

int ralenet_debug_tensor(RalModel* m, const char* name, float** ptr, int64_t* numel) {
  auto it = m->dbg.find(name);
  if (it == m->dbg.end()) return ral_fail("unknown tensor %s", name);
  *ptr = it->second.first;
  *numel = it->second.second;
  return 0;
}

const RalKind* ralenet_kind() {
  static const RalKind k = {
      check_cfg,
      ralenet_layout,
      [](const ral_config& c) { return plan_workspace(c, nullptr, nullptr); },
      64,
      []() -> ral_handle* { return new RalModel(); },
      nullptr};
  return &k;
}
