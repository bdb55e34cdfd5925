// C ABI (include/ralenet.h): the error state, the library switches, the dispatch of the model interface (ral_model.hpp),
// the loss and Adam entry points, the plan and geometry queries and the attention entry points (their launchers are the
// model's).  Every other stateless entry point is defined in the file that holds its kernels.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <ctype.h>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/ralenet.h"
#include "ral_model.hpp"
#include "ral_kernels.hpp"
#include "ral_ralenet.hpp"
#include "ral_ralenet_plan.hpp"
#include "ral_unet.hpp"
#include "ral_unet_plan.hpp"
#include "ral_baseline_plan.hpp"

static thread_local char g_err[512] = "";
int ral_fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}
extern "C" const char* ral_last_error(void) { return g_err; }
// how the table entry points of the feature files end (ral_model.hpp)
int table_done(const char* name, int rc, const char* why, long long bad, const char* args_fmt, ...) {
  if (rc == 0) {
    HIP_OK(hipGetLastError());
    return 0;
  }
  if (rc != -1) return ral_fail("%s: copying the table to the device failed", name);
  char row[40] = "", args[sizeof(g_err)];
  if (bad >= 0) snprintf(row, sizeof(row), " in row %lld", bad);
  va_list ap;
  va_start(ap, args_fmt);
  vsnprintf(args, sizeof(args), args_fmt, ap);
  va_end(ap);
  return ral_fail("%s: need %s%s (%s)", name, why, row, args);
}

// ---------------------------------------------------------------------------------------------------------------------
// Switches.  A switch stays only while a test, a bench.py leg or a committed tool sets it to pick a kernel or a schedule;
// every other tuning choice is a named constant next to its launcher.  Each switch has a compile-time default and a name in
// the list below.  The product build reads NO environment variable for them: the only way to change one is
// ral_global_option() (C ABI; process-wide, to be called before the first use - most are read once).  The library reads
// exactly two environment variables, both validated: RAL_LANES (1 .. 4 micro-batch chains) and RAL_NO_SIDE_STREAM (0 / 1).
// A diagnostic build (-DRAL_DIAG) additionally takes RAL_<NAME> from the environment for every switch (tools/diag/*.sh).
static const char* const KNOB_NAMES[] = {
  "ATTN_BWD_M", "ATTN_BWD_MH", "ATTN_BWD_W", "ATTN_F16", "ATTN_FWD_H", "ATTN_FWD_T32", "ATTN_FWD_W", "DW_SETS", "F16_SPLIT", "FUSE_DW",
  "MLP_BWD_W", "MLP_BWD_W_F16", "MLP_FWD_W", "TABRED_SIDE", "UNET_EVAL_GRID", "UNET_FUSED"};
static std::mutex g_knob_mu;
static std::map<std::string, long long>& knob_table() { static std::map<std::string, long long> t; return t; }
static std::map<std::string, long long>& knob_read() { static std::map<std::string, long long> t; return t; }   // value each switch was read at
// grid caps and set counts: 0 would be a launch with no workgroup (a launch error), not "automatic"
static const char* const KNOB_MIN1[] = {"DW_SETS", "UNET_EVAL_GRID"};
long long ral_knob(const char* name, long long dflt) {
  long long v = dflt;
  std::lock_guard<std::mutex> lk(g_knob_mu);
  auto it = knob_table().find(name);
  if (it != knob_table().end()) v = it->second;
#ifdef RAL_DIAG
  else if (const char* e = getenv((std::string("RAL_") + name).c_str())) v = atoll(e);
#endif
  knob_read()[name] = v;
  return v;
}
// a validated integer environment variable (the product build has two): out-of-range or non-numeric text keeps the default
int ral_env_int(const char* name, int dflt, int lo, int hi) {
  const char* v = getenv(name);
  if (!v || !*v) return dflt;
  char* end = nullptr;
  const long x = strtol(v, &end, 10);
  if (end == v || *end != 0 || x < lo || x > hi) {
    fprintf(stderr, "libralenet: %s=\"%s\" ignored (an integer in [%d, %d] is expected)\n", name, v, lo, hi);
    return dflt;
  }
  return (int)x;
}
int ral_num_cus() {
  static std::mutex mu;
  static std::map<int, int> cus;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  std::lock_guard<std::mutex> lk(mu);
  auto it = cus.find(dev);
  if (it != cus.end()) return it->second;
  hipDeviceProp_t prop;
  const int n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  cus[dev] = n;
  return n;
}
int ral_occupancy(const void* kernel, int threads, size_t lds, int dflt) {
  static std::mutex mu;
  static std::map<std::tuple<const void*, int, size_t>, int> cache;
  const auto key = std::make_tuple(kernel, threads, lds);
  std::lock_guard<std::mutex> lk(mu);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  int occ = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, threads, lds) != hipSuccess || occ < 1) occ = dflt;
  cache[key] = occ;
  return occ;
}
extern "C" int ral_global_option(const char* key, long long value) {
  if (!key) return ral_fail("null key");
  std::string k(key);
  for (auto& c : k) c = (char)toupper((unsigned char)c);
  if (k.rfind("RAL_", 0) == 0) k = k.substr(4);
  bool known = false;
  for (const char* n : KNOB_NAMES) known = known || k == n;
  if (!known) return ral_fail("unknown switch %s", key);
  if (value < 0) return ral_fail("switch %s: negative value %lld", key, value);
  for (const char* n : KNOB_MIN1)
    if (k == n && value < 1) return ral_fail("switch %s: value %lld out of range (a grid / set count: >= 1)", key, value);
  std::lock_guard<std::mutex> lk(g_knob_mu);
  // most consumers read a switch once and keep it: a change after that first read would be ignored silently, so it is refused
  // (the value in force, default included, is fine: tests and tools set their switches at start-up, possibly more than once)
  auto rd = knob_read().find(k);
  if (rd != knob_read().end() && rd->second != value)
    return ral_fail("switch %s was already read by the library (switches are latched at first use): set it before the first model is created", key);
  knob_table()[k] = value;
  return 0;
}


// ---------------------------------------------------------------------------------
// the model interface: what the base provides, and the table of networks
// ---------------------------------------------------------------------------------
int ParamLayout::copy_out(int idx, char* name, int name_cap, int32_t* kind, int64_t* offset, int32_t* ndim, int64_t shape[4]) const {
  if (idx < 0 || idx >= (int)entries.size()) return ral_fail("entry %d out of range", idx);
  const ParamEntry& e = entries[idx];
  if ((int)e.name.size() + 1 > name_cap) return ral_fail("name buffer too small");
  strcpy(name, e.name.c_str());
  *kind = e.kind; *offset = e.offset; *ndim = e.ndim;
  for (int i = 0; i < 4; ++i) shape[i] = e.shape[i];
  return 0;
}

ral_handle::~ral_handle() { if (slab) (void)hipFree(slab); }
hipError_t ral_handle::alloc_slab(size_t bytes) {
  const hipError_t e = hipMalloc(reinterpret_cast<void**>(&slab), bytes);
  if (e != hipSuccess) slab = nullptr;
  return e;
}
int ral_handle::bind(float* params_, float* grads_, float* am_, float* av_, float* state_, double* bn_sums_) {
  params = params_; grads = grads_; am = am_; av = av_; state = state_; bn_sums = bn_sums_;
  return 0;
}
int ral_handle::set_option(const char*, int) { return ral_fail("no options for this handle"); }


// the network of a configuration that its network accepts; null (and the message) otherwise
static const RalKind* kind_of(const ral_config* c) {
  if (!c) { ral_fail("null config"); return nullptr; }
  if (c->variant < 0 || c->variant > RAL_DANET) { ral_fail("unknown variant %d", c->variant); return nullptr; }
  static const RalKind* const KINDS[] = {ralenet_kind(), ralenet_kind(), ralenet_kind(), unet_kind(), acdae_kind(), danet_kind()};   // by variant
  const RalKind* k = KINDS[c->variant];
  return k->check_cfg(c) ? nullptr : k;
}

extern "C" {

int ral_layout_count(const ral_config* cfg) {
  const RalKind* k = kind_of(cfg);
  if (!k) return -1;
  ParamLayout L;
  k->layout(*cfg, L);
  return (int)L.entries.size();
}

int ral_layout_entry(const ral_config* cfg, int idx, char* name, int name_cap, int32_t* kind, int64_t* offset,
                     int32_t* ndim, int64_t shape[4]) {
  const RalKind* k = kind_of(cfg);
  if (!k) return -1;
  ParamLayout L;
  k->layout(*cfg, L);
  return L.copy_out(idx, name, name_cap, kind, offset, ndim, shape);
}

int64_t ral_param_floats(const ral_config* cfg) {
  const RalKind* k = kind_of(cfg);
  if (!k) return -1;
  ParamLayout L;
  k->layout(*cfg, L);
  return L.nparam;
}

int64_t ral_state_floats(const ral_config* cfg) {
  const RalKind* k = kind_of(cfg);
  if (!k) return -1;
  ParamLayout L;
  k->layout(*cfg, L);
  return L.nstate;
}

int64_t ral_bn_sums_doubles(const ral_config* cfg) {
  const RalKind* k = kind_of(cfg);
  return k ? k->bn_sums_doubles : -1;
}

int64_t ral_workspace_bytes(const ral_config* cfg) {
  const RalKind* k = kind_of(cfg);
  return k ? (int64_t)k->workspace_bytes(*cfg) : -1;
}

int ral_pe_table(const ral_config* cfg, int level, float* out_host, int64_t cap) {
  const RalKind* k = kind_of(cfg);
  if (!k) return -1;
  if (k != ralenet_kind()) return ral_fail("no PE table for this variant/level");
  return ralenet_pe_table(cfg, level, out_host, cap);
}

int ral_create(const ral_config* cfg, ral_handle** out) {
  const RalKind* k = kind_of(cfg);
  if (!k) return -1;
  if (!out) return ral_fail("null out");
  ral_handle* h = k->create();
  h->kind = k;
  h->cfg = *cfg;
  if (h->init()) { delete h; return -1; }
  *out = h;
  return 0;
}

int ral_destroy(ral_handle* h) {
  delete h;
  return 0;
}

int ral_bind(ral_handle* h, float* params, float* grads, float* adam_m, float* adam_v, float* state, double* bn_sums) {
  if (!h) return ral_fail("null handle");
  return h->bind(params, grads, adam_m, adam_v, state, bn_sums);
}

// the RA-LENet model behind h, or null and `refusal` as the message
static RalModel* ralenet_only(ral_handle* h, const char* refusal) {
  RalModel* m = ralenet_model(h);
  if (!m) ral_fail("%s", refusal);
  return m;
}

int ral_forward_begin(ral_handle* h, const float* x, int B, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, h->kind->no_forward_begin);
  return m ? ralenet_forward_begin(m, x, B, (hipStream_t)s) : -1;
}

int ral_forward_end(ral_handle* h, float* y, int B, int64_t global_windows, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, h->kind->no_forward_begin);
  return m ? ralenet_forward_end(m, y, B, global_windows, (hipStream_t)s) : -1;
}

int ral_forward(ral_handle* h, const float* x, float* y, int B, int training, ral_stream s) {
  if (!h) return ral_fail("null handle");
  return h->forward(x, y, B, training, (hipStream_t)s);
}

int ral_loss(ral_handle* h, const float* pred, const float* target, int B, int64_t global_windows, float* dy,
             float* snr, float* rmse, double* loss_sum, ral_stream s) {
  if (!h) return ral_fail("null handle");
  const int n = h->cfg.leads * h->cfg.L;
  const float gscale = (float)(2.0 / ((double)global_windows * n));
  launch_loss(pred, target, dy, snr, rmse, loss_sum, n, B, gscale, (hipStream_t)s);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_loss_mean(const float* pred, const float* target, int n, int B, int64_t global_windows, float* dy, float* snr,
                  float* rmse, double* loss_mean, double* scratch2, ral_stream s) {
  if (!pred || !target || !loss_mean || !scratch2) return ral_fail("ral_loss_mean: null pointer");
  if (n <= 0 || B <= 0 || global_windows <= 0) return ral_fail("ral_loss_mean: n, B and global_windows must be positive");
  launch_loss(pred, target, dy, snr, rmse, scratch2, n, B, (float)(2.0 / ((double)global_windows * n)), (hipStream_t)s, loss_mean,
              1.0 / (double)global_windows);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_loss_means(const float* pred, const float* target, int n, int B, int64_t global_windows, float* dy, float* snr,
                   float* rmse, double* means3, double* scratch64, ral_stream s) {
  if (!pred || !target || !means3 || !scratch64) return ral_fail("ral_loss_means: null pointer");
  if (n <= 0 || B <= 0 || global_windows <= 0) return ral_fail("ral_loss_means: n, B and global_windows must be positive");
  launch_loss(pred, target, dy, snr, rmse, scratch64, n, B, (float)(2.0 / ((double)global_windows * n)), (hipStream_t)s, means3,
              1.0 / (double)global_windows, 1);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_forward_loss_means(ral_handle* h, const float* x, const float* target, float* y, int B, float* dy, float* snr,
                           float* rmse, double* means3, double* scratch64, ral_stream s) {
  if (!h) return ral_fail("null handle");
  if (!x || !target || !y || !means3 || !scratch64) return ral_fail("ral_forward_loss_means: null pointer");
  if (UNetModel* u = (dy && h->cfg.train) ? unet_model(h) : nullptr)      // U-Net: the output BatchNorm, the loss and the backward's first sums in one kernel
    return unet_forward_loss(u, x, target, y, B, dy, snr, rmse, scratch64, means3, 1.0 / (double)B, 1, (hipStream_t)s);
  if (ral_forward(h, x, y, B, 1, s)) return -1;
  return ral_loss_means(y, target, h->cfg.leads * h->cfg.L, B, B, dy, snr, rmse, means3, scratch64, s);
}

int ral_loss_flat(const float* pred, const float* target, int n, int B, int64_t global_windows, float* dy, float* snr,
                  float* rmse, double* loss_sum, ral_stream s) {
  if (!pred || !target) return ral_fail("ral_loss_flat: null pointer");
  if (n <= 0 || B <= 0 || global_windows <= 0) return ral_fail("ral_loss_flat: n, B and global_windows must be positive");
  launch_loss(pred, target, dy, snr, rmse, loss_sum, n, B, (float)(2.0 / ((double)global_windows * n)), (hipStream_t)s);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_backward_begin(ral_handle* h, const float* dy, int B, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, "ral_backward_begin: RA-LENet handles only (the other networks: ral_backward)");
  return m ? ralenet_backward_begin(m, dy, B, true, (hipStream_t)s) : -1;
}

int ral_backward_end(ral_handle* h, float* dx, int B, int64_t global_windows, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, "ral_backward_end: RA-LENet handles only (the other networks: ral_backward)");
  return m ? ralenet_backward_end(m, dx, B, global_windows, (hipStream_t)s) : -1;
}

// ---- U-Net, one stage at a time (sync-BatchNorm under data parallelism) ----
int ral_unet_stage_bn(int si) { return unet_stage_bn(si); }
#define UNET_ONLY                                  \
  if (!h) return ral_fail("null handle");          \
  UNetModel* u = unet_model(h);                    \
  if (!u) return ral_fail("U-Net handles only")
int ral_unet_forward_stage(ral_handle* h, const float* x, int B, int training, int si, int64_t global_windows, ral_stream s) {
  UNET_ONLY;
  return unet_forward_stage(u, x, B, training, si, global_windows, (hipStream_t)s);
}
int ral_unet_forward_finish(ral_handle* h, float* y, int B, int training, int64_t global_windows, ral_stream s) {
  UNET_ONLY;
  return unet_forward_finish(u, y, B, training, global_windows, (hipStream_t)s);
}
int ral_unet_backward_start(ral_handle* h, const float* dy, int B, int64_t global_windows, ral_stream s) {
  UNET_ONLY;
  return unet_backward_start(u, dy, B, global_windows, (hipStream_t)s);
}
int ral_unet_backward_stage(ral_handle* h, int B, int si, int64_t global_windows, ral_stream s) {
  UNET_ONLY;
  return unet_backward_stage(u, B, si, global_windows, (hipStream_t)s);
}
int ral_unet_backward_finish(ral_handle* h, int B, int64_t global_windows, ral_stream s) {
  UNET_ONLY;
  return unet_backward_finish(u, B, global_windows, (hipStream_t)s);
}
#undef UNET_ONLY

int ral_grad_bucket(ral_handle* h, int k, int64_t* offset, int64_t* count) {
  RalModel* m = ralenet_only(h, "gradient buckets: RA-LENet handles only");
  return m ? ralenet_grad_bucket(m, k, offset, count) : -1;
}

int ral_grad_bucket_wait(ral_handle* h, int k, ral_stream s) {
  RalModel* m = ralenet_only(h, "gradient buckets: RA-LENet handles only");
  return m ? ralenet_grad_bucket_wait(m, k, (hipStream_t)s) : -1;
}

int ral_backward(ral_handle* h, const float* dy, float* dx, int B, ral_stream s) {
  if (!h) return ral_fail("null handle");
  return h->backward(dy, dx, B, (hipStream_t)s);
}

int ral_backward_input(ral_handle* h, const float* dy, float* dx, int B, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, "ral_backward_input: RA-LENet handles only");
  if (!m) return -1;
  if (!dx) return ral_fail("ral_backward_input: dx is the only result, it cannot be NULL");
  if (ralenet_backward_begin(m, dy, B, false, (hipStream_t)s)) return -1;
  return ralenet_backward_end(m, dx, B, B, (hipStream_t)s);
}

int ral_backward_input_begin(ral_handle* h, const float* dy, int B, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, "ral_backward_input_begin: RA-LENet handles only");
  return m ? ralenet_backward_begin(m, dy, B, false, (hipStream_t)s) : -1;
}

int ral_backward_input_end(ral_handle* h, float* dx, int B, int64_t global_windows, ral_stream s) {
  if (!h) return ral_fail("null handle");
  RalModel* m = ralenet_only(h, "ral_backward_input_end: RA-LENet handles only");
  if (!m) return -1;
  if (!dx) return ral_fail("ral_backward_input_end: dx is the only result, it cannot be NULL");
  return ralenet_backward_end(m, dx, B, global_windows, (hipStream_t)s);
}

int ral_adam_step(ral_handle* h, double lr, double beta1, double beta2, double eps, int step, float grad_scale,
                  ral_stream s) {
  if (!h) return ral_fail("null handle");
  if (!h->params || !h->grads || !h->am || !h->av) return ral_fail("ral_bind: params/grads/adam buffers not bound");
  if (step < 1) return ral_fail("step is 1-based");
  launch_adam(h->params, h->grads, h->am, h->av, (size_t)h->lay.nparam, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)s,
              h->after_adam());
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_set_option(ral_handle* h, const char* key, int value) {
  if (!h || !key) return ral_fail("null handle or key");
  return h->set_option(key, value);
}

int ral_profile_select(ral_handle* h, const char* kind) {
  RalModel* m = ralenet_only(h, "profiling is available for RA-LENet handles only");
  return m ? ralenet_profile_select(m, kind) : -1;
}

int ral_profile_read(ral_handle* h, double* total_ms, int64_t* launches) {
  RalModel* m = ralenet_only(h, "profiling is available for RA-LENet handles only");
  return m ? ralenet_profile_read(m, total_ms, launches) : -1;
}

int ral_profile_timeline(ral_handle* h, double* rows, int64_t cap_rows, int64_t* nrows) {
  RalModel* m = ralenet_only(h, "profiling is available for RA-LENet handles only");
  return m ? ralenet_profile_timeline(m, rows, cap_rows, nrows) : -1;
}

int ral_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, int step, float grad_scale, ral_stream s) {
  if (n % 4) return ral_fail("flat Adam needs a multiple of 4 floats");
  launch_adam(p, g, m, v, (size_t)n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)s);
  HIP_OK(hipGetLastError());
  return 0;
}

static int check_attn_args(int N, int H, int Len, int B) {
  if (N < 16 || N % 16 != 0 || N > 1024) return ral_fail("attention: N must be a multiple of 16 in [16, 1024] (got %d)", N);
  if (H < 1 || (H & (H - 1)) != 0 || H > 32) return ral_fail("attention: H must be a power of two <= 32 (got %d)", H);
  if (Len < 0 || Len > N || ((N - Len) & 1)) return ral_fail("attention: the R-wave window (Len=%d) must fit N=%d and be centred", Len, N);
  if (B < 1) return ral_fail("attention: B must be positive");
  return 0;
}

int ral_attention_forward(const float* qkv, float* o, float* lse, const float* table, int N, int H, int Len, int B,
                          ral_stream s) {
  if (!qkv || !o) return ral_fail("attention: null pointer");
  if (!table || Len == 0) { table = nullptr; Len = 0; }
  if (check_attn_args(N, H, Len, B)) return -1;
  launch_attn_fwd(attn_fwd_plan(N, H, Len, attn_f16_default(), 0), qkv, o, lse, table, N, H, Len, B, (hipStream_t)s);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_attention_plan(int backward, int N, int H, int Len, int has_table, int f16, int NE, int B, char* kernel_name, int name_cap,
                       int32_t* hg, int32_t* threads, int64_t* lds_bytes, int64_t* scratch_floats) {
  if (!has_table) Len = 0;
  if (check_attn_args(N, H, Len, B)) return -1;
  if (NE < 0 || NE > N) return ral_fail("attention: NE=%d existing tokens of N=%d slots", NE, N);
  if (f16 < 0) f16 = attn_f16_default();
  const AttnPlan p = backward ? attn_bwd_plan(N, H, Len, f16, NE, B) : attn_fwd_plan(N, H, Len, f16, NE);
  if (kernel_name && name_cap > 0) snprintf(kernel_name, (size_t)name_cap, "%s", p.name);
  if (hg) *hg = p.hg;
  if (threads) *threads = p.threads;
  if (lds_bytes) *lds_bytes = (int64_t)p.lds;
  if (scratch_floats) *scratch_floats = (int64_t)p.scratch_floats;
  return 0;
}

int ral_block_plan(int launch, int C, int N, int NE, int training, int second_out, int want_dw, int f16_split, int narrow_f16,
                   char* kernel_name, int name_cap, int32_t* threads, int64_t* lds_bytes, int32_t* chunks, int32_t* split,
                   int32_t* stores_upre, int32_t* mlp_dw_fused, int32_t* dw_split) {
  if (launch < 0 || launch > 7) return ral_fail("block plan: launch must be 0 .. 7 (qkv_fwd, mlp_fwd, mlp_bwd, qkv_bwd, dw fc2, fc1, proj, qkv; got %d)", launch);
  if (C != 8 && C != 16 && C != 32 && C != 64 && C != 128) return ral_fail("block plan: C must be 8, 16, 32, 64 or 128 (got %d)", C);
  if (N < 16 || N % 16 != 0 || N > 1024) return ral_fail("block plan: N must be a multiple of 16 in [16, 1024] (got %d)", N);
  if (C * N > 8 * 1024) return ral_fail("block plan: C N = %d: a level of a model holds C N = 8 Lp <= 8192 floats per window", C * N);
  if (NE < 0 || NE > N) return ral_fail("block plan: NE=%d existing tokens of N=%d slots", NE, N);
  if (f16_split < 0) return ral_fail("block plan: f16_split must not be negative (got %d)", f16_split);
  if (f16_split > 0 && NE > 0 && NE < N) return ral_fail("block plan: f16_split > 0 needs whole windows (NE=%d of N=%d: padded windows run on fp32 MFMA)", NE, N);
  const BlockPlan p = block_plan(BlockShape{C, N, NE, training != 0, second_out != 0, want_dw != 0, f16_split > 0 && C >= f16_split,
                                            f16_split > 0 && narrow_f16 != 0});
  const BlockLaunch* const all[8] = {&p.qkv_fwd, &p.mlp_fwd, &p.mlp_bwd, &p.qkv_bwd, &p.dw[0], &p.dw[1], &p.dw[2], &p.dw[3]};
  const BlockLaunch& l = *all[launch];
  if (kernel_name && name_cap > 0) snprintf(kernel_name, (size_t)name_cap, "%s", l.name);
  if (threads) *threads = l.threads;
  if (lds_bytes) *lds_bytes = (int64_t)l.lds;
  if (chunks) *chunks = l.chunks;
  if (split) *split = l.split ? 1 : 0;
  if (stores_upre) *stores_upre = p.stores_upre ? 1 : 0;
  if (mlp_dw_fused) *mlp_dw_fused = p.mlp_dw_fused ? 1 : 0;
  if (dw_split) *dw_split = p.dw_split ? 1 : 0;
  return 0;
}

int ral_unet_stage_geom(int leads, int si, int32_t* row, int cap) {
  if (leads != 1 && leads != 2) return ral_fail("leads must be 1 or 2 (got %d)", leads);
  if (si < 0 || si > 10) return ral_fail("U-Net stage %d outside [0, 10]", si);
  const UStageGeom& g = unet_stages(leads)[si];
  const int v[19] = {g.cin, g.cout, g.ks, g.mode, g.stride, g.pad, g.type, g.post_lrelu, g.bn, g.a.z, g.a.act, g.a.accumulate,
                     g.b.z, g.b.act, g.b.accumulate, g.r.z, g.r.act, g.r.accumulate, g.len_shift};
  if (!row || cap < 19) return ral_fail("U-Net stage row: room for 19 values is needed (got %d)", row ? cap : 0);
  for (int i = 0; i < 19; ++i) row[i] = v[i];
  return 0;
}

int ral_unet_stage_plan(int backward, int leads, int L, int B, int training, int si, int unet_fused, char* kernel_name, int name_cap,
                        int32_t* grid, int32_t* threads, int32_t* windows_per_pass, int64_t* lds_bytes, int32_t* fold, int32_t* fused_eval) {
  ral_config c;
  memset(&c, 0, sizeof(c));
  c.leads = leads; c.L = L; c.max_batch = B; c.train = 1;
  if (unet_kind()->check_cfg(&c)) return -1;
  if (si < -1 || si > 10) return ral_fail("U-Net stage %d outside [0, 10]", si);
  const UPassPlan pp = unet_pass_plan(leads, L, true, unet_fused < 0 ? unet_fused_default() : unet_fused != 0);
  const bool eval_forward = !backward && !training;
  const UStageLaunch l = si >= 0 ? unet_stage_plan(leads, L, B, training != 0, backward != 0, si)
                                 : (eval_forward ? pp.fused : unet_pass_plan(leads, L, true, false).fused);
  if (kernel_name && name_cap > 0) snprintf(kernel_name, (size_t)name_cap, "%s", l.name);
  if (grid) *grid = l.grid;
  if (threads) *threads = l.threads;
  if (windows_per_pass) *windows_per_pass = l.windows_per_pass;
  if (lds_bytes) *lds_bytes = (int64_t)l.lds;
  if (fold) *fold = pp.fold ? 1 : 0;
  if (fused_eval) *fused_eval = pp.fused_eval ? 1 : 0;
  return 0;
}

// the baseline queries refuse a (variant, leads, L) a model of that network refuses, in its words
static int baseline_refused(int variant, int leads, int L) {
  if (variant != RAL_ACDAE && variant != RAL_DANET) return ral_fail("baseline plan: variant must be ACDAE (%d) or DANet (%d), got %d", RAL_ACDAE, RAL_DANET, variant);
  ral_config c;
  memset(&c, 0, sizeof(c));
  c.variant = variant; c.leads = leads; c.L = L;
  const std::string why = variant == RAL_ACDAE ? acdae_legal(c) : danet_legal(c);
  return why.empty() ? 0 : ral_fail("%s", why.c_str());
}

int ral_baseline_layer_geom(int variant, int leads, int i, int32_t* row, int cap) {
  if (baseline_refused(variant, leads, 64)) return -1;      // (the rows do not depend on L: any length both networks take)
  if (i < 0 || i >= BASELINE_LAYERS) return ral_fail("baseline row %d outside [0, %d]", i, BASELINE_LAYERS - 1);
  int v[9], n;
  if (variant == RAL_ACDAE) {
    const AcdaeLayer& r = acdae_layers()[i];
    const int a[7] = {r.cin, r.cout, r.ks, r.convt, r.in_shift, r.out_shift, r.skip};
    n = 7; memcpy(v, a, sizeof(a));
  } else {
    const DanetCell& r = danet_cells(leads)[i];
    const int a[9] = {r.cin, r.c, r.k, r.p, r.tr, r.in_shift, r.out_shift, r.in1, r.dam};
    n = 9; memcpy(v, a, sizeof(a));
  }
  if (!row || cap < n) return ral_fail("baseline row: room for %d values is needed (got %d)", n, row ? cap : 0);
  for (int j = 0; j < n; ++j) row[j] = v[j];
  return 0;
}

int ral_baseline_pass_plan(int variant, int leads, int L, int B, int training, int backward, int k, char* kernel_name, int name_cap,
                           int32_t* layer, int32_t* grid_x, int32_t* grid_y, int32_t* threads, int64_t* lds_bytes, int32_t* extra) {
  if (baseline_refused(variant, leads, L)) return -1;
  if (B < 1) return ral_fail("baseline plan: B must be positive (got %d)", B);
  (void)training;      // a training and an eval forward launch the same: the kernels take the mode as an argument
  const BPass pass = variant == RAL_ACDAE ? acdae_pass(L, B, backward != 0) : danet_pass(leads, L, B, backward != 0);
  if (k < 0) return pass.n;
  if (k >= pass.n) return ral_fail("baseline plan: launch %d outside [0, %d)", k, pass.n);
  const BLaunch& l = pass.e[k];
  if (kernel_name && name_cap > 0) snprintf(kernel_name, (size_t)name_cap, "%s", l.name);
  if (layer) *layer = l.layer;
  if (grid_x) *grid_x = l.gx;
  if (grid_y) *grid_y = l.gy;
  if (threads) *threads = l.threads;
  if (lds_bytes) *lds_bytes = (int64_t)l.lds;
  if (extra) *extra = l.extra;
  return 0;
}

int ral_ralenet_node_geom(int i, int32_t* row, int cap) {
  if (i < 0 || i >= RAL_NODES) return ral_fail("RA-LENet node %d outside [0, %d]", i, RAL_NODES - 1);
  if (!row || cap < 9) return ral_fail("RA-LENet node row: room for 9 values is needed (got %d)", row ? cap : 0);
  const RalNode& n = RAL_NET[i];
  const int v[9] = {n.kind, n.idx, n.level, n.rw, n.D, n.up, n.in, n.add, n.out};
  for (int j = 0; j < 9; ++j) row[j] = v[j];
  return RAL_NODES;
}

int ral_ralenet_pass_plan(int backward, int B, int lanes, int k, int32_t* row, int cap) {
  if (B < 1) return ral_fail("RA-LENet pass: B must be positive (got %d)", B);
  if (lanes < 1 || lanes > MAX_LANES) return ral_fail("RA-LENet pass: lanes must be in [1, %d] (got %d)", MAX_LANES, lanes);
  const RalLaneSplit sp = ralenet_lane_split(B, lanes);
  const int n = RAL_NODES * sp.n;
  if (k < 0 || k >= n) return ral_fail("RA-LENet pass: entry %d outside [0, %d)", k, n);
  if (!row || cap < 9) return ral_fail("RA-LENet pass row: room for 9 values is needed (got %d)", row ? cap : 0);
  const RalPassEntry e = ralenet_pass(backward != 0, k / sp.n);
  const int lane = k % sp.n;
  const RalBinding b = ralenet_bind(RAL_NET[e.node], backward != 0);
  const int v[9] = {e.node, lane, sp.w0[lane], sp.B[lane], b.in, b.extra, b.out, b.fwd_in, e.mark && lane == sp.n - 1 ? 1 : 0};
  for (int j = 0; j < 9; ++j) row[j] = v[j];
  return n;
}

int64_t ral_attention_backward_scratch_floats(int N, int H, int Len, int has_table, int B) {
  if (!has_table) Len = 0;
  if (check_attn_args(N, H, Len, B)) return -1;
  return (int64_t)attn_bwd_plan(N, H, Len, attn_f16_default(), 0, B).scratch_floats;
}

int ral_attention_backward(const float* qkv, const float* o, const float* d_o, const float* lse, const float* table,
                           float* gtable, float* dqkv, float* scratch, int64_t scratch_floats, int N, int H, int Len,
                           int B, ral_stream s) {
  if (!qkv || !o || !d_o || !lse || !dqkv || (table && !gtable)) return ral_fail("attention: null pointer");
  if (!table || Len == 0) { table = nullptr; Len = 0; }
  if (check_attn_args(N, H, Len, B)) return -1;
  // scratch of the kernels that hand partial results from one launch to the next: owned by the caller, so the entry point
  // holds no state, never allocates and can be captured into a hipGraph
  const AttnPlan p = attn_bwd_plan(N, H, Len, attn_f16_default(), 0, B);
  if (launch_attn_bwd(p, qkv, o, d_o, lse, table, gtable, dqkv, scratch, scratch && scratch_floats > 0 ? (size_t)scratch_floats : 0, N, H, Len, B,
                      (hipStream_t)s))
    return ral_fail("attention backward: this shape needs %lld floats of scratch (ral_attention_backward_scratch_floats), got %lld",
                (long long)p.scratch_floats, (long long)(scratch ? scratch_floats : 0));
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_debug_tensor(ral_handle* h, const char* name, float** ptr, int64_t* numel) {
  RalModel* m = ralenet_only(h, "no debug tensors for this handle");
  return m ? ralenet_debug_tensor(m, name, ptr, numel) : -1;
}

}  // extern "C"
