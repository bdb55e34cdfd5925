// C ABI (include/ralenet.h): the error state, the library switches, the dispatch of the model interface (ral_model.hpp)
// and the stateless entry points.
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

int ral_conv13_forward(const float* x, const float* w, const float* b, float* y, int B, int cin, int cout, int L,
                       int lrelu, ral_stream s) {
  const char* why = nullptr;
  if (launch_conv13_fwd(x, w, b, y, B, cin, cout, L, lrelu, (hipStream_t)s, &why))
    return ral_fail("ral_conv13_forward: %s (B=%d, channels %d -> %d, L=%d)", why, B, cin, cout, L);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_conv13_backward(const float* x, const float* y, const float* dy, const float* w, float* gw, float* gb,
                        float* dx, int B, int cin, int cout, int L, int lrelu, ral_stream s) {
  const char* why = nullptr;
  if (launch_conv13_bwd(x, y, dy, w, gw, gb, dx, B, cin, cout, L, lrelu, (hipStream_t)s, &why))
    return ral_fail("ral_conv13_backward: %s (B=%d, channels %d -> %d, L=%d)", why, B, cin, cout, L);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_adam_flat(float* p, const float* g, float* m, float* v, int64_t n, double lr, double beta1, double beta2,
                  double eps, int step, float grad_scale, ral_stream s) {
  if (n % 4) return ral_fail("flat Adam needs a multiple of 4 floats");
  launch_adam(p, g, m, v, (size_t)n, lr, beta1, beta2, eps, step, grad_scale, (hipStream_t)s);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_prep_windows(const float* sig, const float* noise, int64_t T, int leads, int L, double snr_db, double* sums,
                     float* noisy, float* clean, ral_stream s) {
  if (!sig || !noise || !sums || !noisy || !clean) return ral_fail("prep_windows: null pointer");
  if (launch_prep_windows(sig, noise, (long long)T, leads, L, snr_db, sums, noisy, clean, (hipStream_t)s))
    return ral_fail("prep_windows: need 1 <= leads <= 16 and T a positive multiple of L (T=%lld leads=%d L=%d)", (long long)T, leads, L);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_stream_windows(const float* rec, int64_t R, int64_t T, int leads, int L, int hop, int64_t w0, int nw, float* win,
                       float* stats, ral_stream s) {
  if (!rec || !win || !stats) return ral_fail("stream_windows: null pointer");
  if (launch_stream_windows(rec, (long long)R, (long long)T, leads, L, hop, (long long)w0, nw, win, stats, (hipStream_t)s))
    return ral_fail("stream_windows: need R >= 1, T >= L, 1 <= hop <= L, L a multiple of 64 and <= 2048, a window range inside the records "
                "(R=%lld T=%lld leads=%d L=%d hop=%d w0=%lld nw=%d)", (long long)R, (long long)T, leads, L, hop, (long long)w0, nw);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_stream_stitch(const float* y, const float* stats, int64_t R, int64_t T, int leads, int L, int hop, float* out,
                      ral_stream s) {
  if (!y || !stats || !out) return ral_fail("stream_stitch: null pointer");
  if (launch_stream_stitch(y, stats, (long long)R, (long long)T, leads, L, hop, out, (hipStream_t)s))
    return ral_fail("stream_stitch: need R >= 1, T >= L, 1 <= hop <= L with L - hop even (R=%lld T=%lld leads=%d L=%d hop=%d)",
                (long long)R, (long long)T, leads, L, hop);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_live_windows(const float* hist, const float* x, float* hist_out, int64_t S, int leads, int L, int hop, int C, int64_t base,
                     int64_t k0, int nw, int64_t T, int64_t w0, int nb, float* win, float* stats, ral_stream s) {
  if (!hist || !x || !win || !stats) return ral_fail("live_windows: null pointer");
  if (launch_live_windows(hist, x, hist_out, (long long)S, leads, L, hop, C, (long long)base, (long long)k0, nw, (long long)T,
                          (long long)w0, nb, win, stats, (hipStream_t)s))
    return ral_fail("live_windows: need S >= 1, leads >= 1, L a multiple of 64 and <= 2048, 1 <= hop <= L with L - hop even, C >= 0, "
                "T < 0 or T >= L, windows k0 .. k0 + nw - 1 of the stream inside samples [base, base + L + C), a window range "
                "inside the S * nw windows, and nb >= 1 or a history to write (S=%lld leads=%d L=%d hop=%d C=%d base=%lld k0=%lld "
                "nw=%d T=%lld w0=%lld nb=%d)", (long long)S, leads, L, hop, C, (long long)base, (long long)k0, nw, (long long)T,
                (long long)w0, nb);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_live_emit(const float* y, const float* stats, int64_t S, int leads, int L, int hop, int64_t k0, int nw, int64_t T,
                  int64_t w0, int nb, int64_t lo, int m, float* out, float* last_y, float* last_stats, ral_stream s) {
  if (!y || !stats || !out) return ral_fail("live_emit: null pointer");
  if (launch_live_emit(y, stats, (long long)S, leads, L, hop, (long long)k0, nw, (long long)T, (long long)w0, nb, (long long)lo, m,
                       out, last_y, last_stats, (hipStream_t)s))
    return ral_fail("live_emit: need S >= 1, leads >= 1, L a multiple of 64 and <= 2048, 1 <= hop <= L with L - hop even, "
                "T < 0 or T >= L with windows k0 .. k0 + nw - 1 in the stream, a window range of nb >= 1 windows inside the "
                "S * nw, lo >= 0, m >= 0, and last_y and last_stats both given or both null (S=%lld leads=%d L=%d hop=%d "
                "k0=%lld nw=%d T=%lld w0=%lld nb=%d lo=%lld m=%d)", (long long)S, leads, L, hop, (long long)k0, nw, (long long)T,
                (long long)w0, nb, (long long)lo, m);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_newrale_stream_front(const float* rec, int64_t R, int64_t T, int L, int hop, int64_t w0, int nw,
                             const float* adapter_params, float* inner_x, float* stats, ral_stream s) {
  if (!rec || !adapter_params || !inner_x || !stats) return ral_fail("newrale_stream_front: null pointer");
  if (launch_newrale_front(rec, (long long)R, (long long)T, L, hop, (long long)w0, nw, adapter_params, inner_x, stats, (hipStream_t)s))
    return ral_fail("newrale_stream_front: need R >= 1, T >= L, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, "
                "a window range inside the records (R=%lld T=%lld L=%d hop=%d w0=%lld nw=%d)", (long long)R, (long long)T, L, hop,
                (long long)w0, nw);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_newrale_stream_back(const float* inner_y, const float* stats, const float* adapter_params, int64_t R, int64_t T, int L,
                            int hop, int64_t w0, int nw, float* out, ral_stream s) {
  if (!inner_y || !stats || !adapter_params || !out) return ral_fail("newrale_stream_back: null pointer");
  if (launch_newrale_back(inner_y, stats, adapter_params, (long long)R, (long long)T, L, hop, (long long)w0, nw, out, (hipStream_t)s))
    return ral_fail("newrale_stream_back: need R >= 1, T >= L, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, "
                "a window range inside the records (R=%lld T=%lld L=%d hop=%d w0=%lld nw=%d)", (long long)R, (long long)T, L, hop,
                (long long)w0, nw);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_newrale_live_front(const float* hist, const float* x, float* hist_out, int64_t S, int L, int hop, int C, int64_t base,
                           int64_t k0, int nw, int64_t T, int64_t w0, int nb, const float* adapter_params, float* inner_x,
                           float* stats, ral_stream s) {
  if (!hist || !x || !adapter_params || !inner_x || !stats) return ral_fail("newrale_live_front: null pointer");
  if (launch_newrale_live_front(hist, x, hist_out, (long long)S, L, hop, C, (long long)base, (long long)k0, nw, (long long)T,
                                (long long)w0, nb, adapter_params, inner_x, stats, (hipStream_t)s))
    return ral_fail("newrale_live_front: need S >= 1, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, C >= 0, "
                "T < 0 or T >= L, windows k0 .. k0 + nw - 1 of the stream inside samples [base, base + L + C), a window range "
                "inside the S * nw windows, and nb >= 1 or a history to write (another buffer than hist) (S=%lld L=%d hop=%d "
                "C=%d base=%lld k0=%lld nw=%d T=%lld w0=%lld nb=%d)", (long long)S, L, hop, C, (long long)base, (long long)k0,
                nw, (long long)T, (long long)w0, nb);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_newrale_live_back(const float* inner_y, const float* stats, const float* adapter_params, int64_t S, int L, int hop,
                          int64_t k0, int nw, int64_t T, int64_t w0, int nb, int64_t lo, int m, float* out, float* last_y,
                          float* last_stats, ral_stream s) {
  if (!inner_y || !stats || !adapter_params || !out) return ral_fail("newrale_live_back: null pointer");
  if (launch_newrale_live_back(inner_y, stats, adapter_params, (long long)S, L, hop, (long long)k0, nw, (long long)T,
                               (long long)w0, nb, (long long)lo, m, out, last_y, last_stats, (hipStream_t)s))
    return ral_fail("newrale_live_back: need S >= 1, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, "
                "T < 0 or T >= L with windows k0 .. k0 + nw - 1 in the stream, a window range of nb >= 1 windows inside the "
                "S * nw, lo >= 0, m >= 0, and last_y and last_stats both given or both null (S=%lld L=%d hop=%d k0=%lld nw=%d "
                "T=%lld w0=%lld nb=%d lo=%lld m=%d)", (long long)S, L, hop, (long long)k0, nw, (long long)T, (long long)w0, nb,
                (long long)lo, m);
  HIP_OK(hipGetLastError());
  return 0;
}

// How an entry point that takes a table ends.  rc = 0: launched; what the launches left behind is the result.  rc = -1,
// refused: the one rule that is broken and, if it is a row's, which row, then the call's arguments as args_fmt words them.
// Any other rc: the table did not reach the device.
static int table_done(const char* name, int rc, const char* why, long long bad, const char* args_fmt, ...) {
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
static const char POOL_ARGS[] = "rows=%d capacity=%lld L=%d hop=%d packed=%lld w0=%lld nb=%d";

int ral_pool_windows(float* hist, const float* x, int64_t x_total, const ral_pool_row* table, int rows, ral_pool_row* table_dev,
                     int upload, int64_t capacity, int leads, int L, int hop, int write_hist, int64_t w0, int nb, float* win,
                     float* stats, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !win || !stats) return ral_fail("pool_windows: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_pool_windows(hist, x, (long long)x_total, table, rows, table_dev, upload, (long long)capacity, leads, L, hop,
                                     write_hist, (long long)w0, nb, win, stats, (hipStream_t)s, &why, &bad);
  return table_done("pool_windows", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)x_total, (long long)w0,
                    nb);
}

int ral_pool_emit(const float* y, const float* stats, const ral_pool_row* table, int rows, ral_pool_row* table_dev, int upload,
                  int64_t capacity, int leads, int L, int hop, int64_t w0, int nb, int from_last, float* out, int64_t out_total,
                  float* last_y, float* last_stats, ral_stream s) {
  if (!y || !stats || !table || !table_dev || !out) return ral_fail("pool_emit: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_pool_emit(y, stats, table, rows, table_dev, upload, (long long)capacity, leads, L, hop, (long long)w0, nb,
                                  from_last, out, (long long)out_total, last_y, last_stats, (hipStream_t)s, &why, &bad);
  return table_done("pool_emit", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)out_total, (long long)w0,
                    nb);
}

int ral_newrale_pool_front(float* hist, const float* x, int64_t x_total, const ral_pool_row* table, int rows,
                           ral_pool_row* table_dev, int upload, int64_t capacity, int L, int hop, int write_hist, int64_t w0,
                           int nb, const float* adapter_params, float* inner_x, float* stats, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !adapter_params || !inner_x || !stats) return ral_fail("newrale_pool_front: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_newrale_pool_front(hist, x, (long long)x_total, table, rows, table_dev, upload, (long long)capacity, L, hop,
                                           write_hist, (long long)w0, nb, adapter_params, inner_x, stats, (hipStream_t)s, &why, &bad);
  return table_done("newrale_pool_front", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)x_total,
                    (long long)w0, nb);
}

int ral_newrale_pool_back(const float* inner_y, const float* stats, const float* adapter_params, const ral_pool_row* table,
                          int rows, ral_pool_row* table_dev, int upload, int64_t capacity, int L, int hop, int64_t w0, int nb,
                          int from_last, float* out, int64_t out_total, float* last_y, float* last_stats, ral_stream s) {
  if (!inner_y || !stats || !adapter_params || !table || !table_dev || !out) return ral_fail("newrale_pool_back: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_newrale_pool_back(inner_y, stats, adapter_params, table, rows, table_dev, upload, (long long)capacity, L,
                                          hop, (long long)w0, nb, from_last, out, (long long)out_total, last_y, last_stats,
                                          (hipStream_t)s, &why, &bad);
  return table_done("newrale_pool_back", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)out_total,
                    (long long)w0, nb);
}

int64_t ral_mix_records_scratch_bytes(int64_t R, int leads, int64_t T) {
  const long long n = mix_records_scratch_bytes((long long)R, leads, (long long)T);
  if (n < 0) return ral_fail("mix_records_scratch_bytes: need R >= 1, 1 <= leads <= 16, T >= 1 (R=%lld leads=%d T=%lld)", (long long)R, leads, (long long)T);
  return n;
}

int ral_mix_records(const float* rec, const float* noise, int64_t R, int leads, int64_t T, int64_t Tn, const int64_t* offsets,
                    const double* snr_db, void* scratch, float* noisy, float* clean, ral_stream s) {
  if (!rec || !noise || !offsets || !snr_db || !scratch || !noisy || !clean) return ral_fail("mix_records: need no null pointer");
  const char* why = nullptr;
  long long bad = -1;
  const int rc = launch_mix_records(rec, noise, (long long)R, leads, (long long)T, (long long)Tn, offsets, snr_db, scratch, noisy,
                                    clean, (hipStream_t)s, &why, &bad);
  if (rc == -1) {
    char at[96] = "";
    if (bad >= 0) snprintf(at, sizeof(at), " in record %lld (offset=%lld snr_db=%g)", bad, (long long)offsets[bad], snr_db[bad]);
    return ral_fail("mix_records: need %s%s (R=%lld leads=%d T=%lld Tn=%lld)", why, at, (long long)R, leads, (long long)T, (long long)Tn);
  }
  if (rc) return ral_fail("mix_records: copying offsets / snr_db to the device failed");
  HIP_OK(hipGetLastError());
  return 0;
}

int64_t ral_score_records_scratch_bytes(int64_t R, int leads, int64_t T, int64_t W) {
  const long long n = score_records_scratch_bytes((long long)R, leads, (long long)T, (long long)W);
  if (n < 0)
    return ral_fail("score_records_scratch_bytes: need R >= 1, 1 <= leads <= 16, T >= 1, 1 <= W <= T (R=%lld leads=%d T=%lld W=%lld)",
                (long long)R, leads, (long long)T, (long long)W);
  return n;
}

int ral_score_records(const float* clean, const float* out, const float* noisy, int64_t R, int leads, int64_t T, int64_t W,
                      void* scratch, double* per_lead, double* per_record, double* per_window, double* window_mean, ral_stream s) {
  if (!clean || !out || !scratch || !per_lead || !per_record || !per_window || !window_mean)
    return ral_fail("score_records: need no null pointer (only noisy may be null)");
  const char* why = nullptr;
  if (launch_score_records(clean, out, noisy, (long long)R, leads, (long long)T, (long long)W, scratch, per_lead, per_record,
                           per_window, window_mean, (hipStream_t)s, &why))
    return ral_fail("score_records: need %s (R=%lld leads=%d T=%lld W=%lld)", why, (long long)R, leads, (long long)T, (long long)W);
  HIP_OK(hipGetLastError());
  return 0;
}

static MixBatchGeom mix_geom(int64_t N, int leads, int64_t Lsrc, int L, int K, int64_t Tn, const uint32_t* cum, double snr_lo,
                             double snr_hi, uint64_t seed, uint64_t first) {
  MixBatchGeom G;
  G.N = (long long)N; G.Lsrc = (long long)Lsrc; G.Tn = (long long)Tn;
  G.leads = leads; G.L = L; G.K = K;
  for (int k = 0; k < RAL_MIX_MAX_KINDS; ++k) G.cum[k] = (cum && k < K) ? cum[k] : 0xffffffffu;
  G.snr_lo = snr_lo; G.snr_hi = snr_hi;
  G.seed = seed; G.first = first;
  return G;
}
#define MIX_ARGS "(N=%lld leads=%d Lsrc=%lld L=%d K=%d Tn=%lld B=%lld snr_db=[%g, %g])"

int ral_mix_batch(const float* bank, const float* noise, const int64_t* rows, int64_t N, int leads, int64_t Lsrc, int L, int K,
                  int64_t Tn, const uint32_t* cum, double snr_lo, double snr_hi, uint64_t seed, uint64_t first, int64_t B,
                  float* noisy, float* clean, int32_t* draws, double* snr_db, ral_stream s) {
  const char* why = nullptr;
  int rc = -1;
  if (!bank || !noise || !cum || !noisy || !clean || !draws || !snr_db) why = "no null pointer (only rows may be null)";
  else rc = launch_mix_batch(bank, noise, rows, mix_geom(N, leads, Lsrc, L, K, Tn, cum, snr_lo, snr_hi, seed, first), (long long)B,
                             noisy, clean, draws, snr_db, (hipStream_t)s, &why);
  if (rc)
    return ral_fail("mix_batch: need %s " MIX_ARGS, why, (long long)N, leads, (long long)Lsrc, L, K, (long long)Tn, (long long)B,
                    snr_lo, snr_hi);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_mix_draw(int64_t N, int64_t Lsrc, int L, int K, int64_t Tn, const uint32_t* cum, double snr_lo, double snr_hi,
                 uint64_t seed, uint64_t g, int32_t* draw, double* snr_db) {
  const MixBatchGeom G = mix_geom(N, 1, Lsrc, L, K, Tn, cum, snr_lo, snr_hi, seed, 0);
  const char* why = (!cum || !draw || !snr_db) ? "no null pointer" : mix_batch_check(G);
  if (why)
    return ral_fail("mix_draw: need %s " MIX_ARGS, why, (long long)N, 1, (long long)Lsrc, L, K, (long long)Tn, 1LL, snr_lo, snr_hi);
  mix_batch_draw(G, g, draw, snr_db);
  return 0;
}

int ral_rate_records(const float* x, int64_t R, int leads, int64_t T, int up, int down, const float* bank, int ntaps, float* y,
                     int64_t T_out, ral_stream s) {
  if (!x || !bank || !y) return ral_fail("rate_records: null pointer");
  const char* why = nullptr;
  if (launch_rate_records(x, (long long)R, leads, (long long)T, up, down, bank, ntaps, y, (long long)T_out, (hipStream_t)s, &why))
    return ral_fail("rate_records: need %s (R=%lld leads=%d T=%lld up=%d down=%d ntaps=%d T_out=%lld)", why, (long long)R, leads,
                (long long)T, up, down, ntaps, (long long)T_out);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_rate_pool(float* hist, const float* x, int64_t x_total, const ral_rate_row* table, int rows, ral_rate_row* table_dev,
                  int upload, int64_t capacity, int leads, int up, int down, const float* bank, int ntaps, int hist_len, float* out,
                  int64_t out_total, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !bank || !out) return ral_fail("rate_pool: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_rate_pool(hist, x, (long long)x_total, table, rows, table_dev, upload, (long long)capacity, leads, up, down,
                                  bank, ntaps, hist_len, out, (long long)out_total, (hipStream_t)s, &why, &bad);
  return table_done("rate_pool", rc, why, bad, "rows=%d capacity=%lld leads=%d up=%d down=%d ntaps=%d hist_len=%d x_total=%lld "
                    "out_total=%lld", rows, (long long)capacity, leads, up, down, ntaps, hist_len, (long long)x_total,
                    (long long)out_total);
}

static void beat_geom_text(const ral_beat_geom* g, char* buf, size_t n) {
  if (g) snprintf(buf, n, "half=%d Wi=%d Wt=%d Rf=%d Rw=%d alpha=%g floor=%g", g->half, g->wi, g->wt, g->rf, g->rw, g->alpha, g->floor);
  else snprintf(buf, n, "no geometry");
}

int64_t ral_beat_records_scratch_bytes(int64_t R, int leads, int64_t T, const ral_beat_geom* geom) {
  const char* why = nullptr;
  const long long n = beat_records_scratch_bytes((long long)R, leads, (long long)T, geom, &why);
  if (n < 0) {
    char gt[160];
    beat_geom_text(geom, gt, sizeof(gt));
    return ral_fail("beat_records_scratch_bytes: need %s (R=%lld leads=%d T=%lld %s)", why, (long long)R, leads, (long long)T, gt);
  }
  return n;
}

int ral_beat_records(const float* x, int64_t R, int leads, int64_t T, const ral_beat_geom* geom, const float* bank, int ntaps,
                     void* scratch, int64_t scratch_bytes, int32_t* peaks, int64_t cap, int32_t* count, ral_stream s) {
  if (!x || !geom || !bank || !scratch || !peaks || !count) return ral_fail("beat_records: null pointer");
  const char* why = nullptr;
  if (launch_beat_records(x, (long long)R, leads, (long long)T, geom, bank, ntaps, scratch, (long long)scratch_bytes, peaks,
                          (long long)cap, count, (hipStream_t)s, &why)) {
    char gt[160];
    beat_geom_text(geom, gt, sizeof(gt));
    return ral_fail("beat_records: need %s (R=%lld leads=%d T=%lld ntaps=%d cap=%lld scratch_bytes=%lld %s)", why, (long long)R, leads,
                (long long)T, ntaps, (long long)cap, (long long)scratch_bytes, gt);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_beat_pool(float* hist, const float* x, int64_t x_total, const ral_beat_row* table, int rows, ral_beat_row* table_dev,
                  int upload, int64_t capacity, int leads, const ral_beat_geom* geom, const float* bank, int ntaps, int hist_len,
                  void* scratch, int64_t scratch_bytes, int64_t* peaks, int64_t peaks_total, int32_t* count, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !geom || !bank || !scratch || !peaks || !count) return ral_fail("beat_pool: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_beat_pool(hist, x, (long long)x_total, table, rows, table_dev, upload, (long long)capacity, leads, geom, bank,
                                  ntaps, hist_len, scratch, (long long)scratch_bytes, (long long*)peaks, (long long)peaks_total, count,
                                  (hipStream_t)s, &why, &bad);
  char gt[160] = "";
  if (rc) beat_geom_text(geom, gt, sizeof(gt));
  return table_done("beat_pool", rc, why, bad, "rows=%d capacity=%lld leads=%d ntaps=%d hist_len=%d x_total=%lld "
                    "peaks_total=%lld scratch_bytes=%lld %s", rows, (long long)capacity, leads, ntaps, hist_len, (long long)x_total,
                    (long long)peaks_total, (long long)scratch_bytes, gt);
}

int ral_beat_match(const int32_t* ref, const int32_t* ref_count, int64_t ref_cap, const int32_t* det, const int32_t* det_count,
                   int64_t det_cap, int64_t R, int64_t tol, int64_t* out, ral_stream s) {
  if (!ref || !ref_count || !det || !det_count || !out) return ral_fail("beat_match: null pointer");
  const char* why = nullptr;
  if (launch_beat_match(ref, ref_count, (long long)ref_cap, det, det_count, (long long)det_cap, (long long)R, (long long)tol,
                        (long long*)out, (hipStream_t)s, &why))
    return ral_fail("beat_match: need %s (R=%lld ref_cap=%lld det_cap=%lld tol=%lld)", why, (long long)R, (long long)ref_cap,
                (long long)det_cap, (long long)tol);
  HIP_OK(hipGetLastError());
  return 0;
}

static void rhythm_geom_text(const ral_rhythm_geom* g, char* buf, size_t n) {
  if (g) snprintf(buf, n, "Wb=%d Sa=%d c0=%g r0=%g", g->wb, g->sa, g->c0, g->r0);
  else snprintf(buf, n, "no geometry");
}

int64_t ral_rhythm_pool_scratch_bytes(int64_t beats, int leads, const ral_rhythm_geom* geom) {
  const char* why = nullptr;
  const long long n = rhythm_pool_scratch_bytes((long long)beats, leads, geom, &why);
  if (n < 0) {
    char gt[96];
    rhythm_geom_text(geom, gt, sizeof(gt));
    return ral_fail("rhythm_pool_scratch_bytes: need %s (beats=%lld leads=%d %s)", why, (long long)beats, leads, gt);
  }
  return n;
}

int ral_rhythm_records(const float* x, int64_t R, int leads, int64_t T, const ral_rhythm_geom* geom, const int32_t* peaks,
                       const int32_t* count, int64_t cap, int32_t* label, float* corr, float* rr_ratio, ral_stream s) {
  if (!x || !geom || !peaks || !count || !label || !corr || !rr_ratio) return ral_fail("rhythm_records: null pointer");
  const char* why = nullptr;
  if (launch_rhythm_records(x, (long long)R, leads, (long long)T, geom, peaks, count, (long long)cap, label, corr, rr_ratio,
                            (hipStream_t)s, &why)) {
    char gt[96];
    rhythm_geom_text(geom, gt, sizeof(gt));
    return ral_fail("rhythm_records: need %s (R=%lld leads=%d T=%lld cap=%lld %s)", why, (long long)R, leads, (long long)T,
                (long long)cap, gt);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_rhythm_pool(const float* hist, const float* x, int64_t x_total, const ral_rhythm_row* table, int rows,
                    ral_rhythm_row* table_dev, int upload, int64_t capacity, int leads, const ral_rhythm_geom* geom, int hist_len,
                    float* ring, int64_t* ring_pos, const int64_t* new_pos, int64_t new_total, void* scratch,
                    int64_t scratch_bytes, int64_t* out_pos, int32_t* label, float* corr, float* rr_ratio, int64_t out_total,
                    ral_stream s) {
  if (!hist || !x || !table || !table_dev || !geom || !ring || !ring_pos || !new_pos || !scratch || !out_pos || !label || !corr ||
      !rr_ratio)
    return ral_fail("rhythm_pool: null pointer");
  const char* why = nullptr;
  int bad = -1;
  const int rc = launch_rhythm_pool(hist, x, (long long)x_total, table, rows, table_dev, upload, (long long)capacity, leads, geom,
                                    hist_len, ring, (long long*)ring_pos, (const long long*)new_pos, (long long)new_total, scratch,
                                    (long long)scratch_bytes, (long long*)out_pos, label, corr, rr_ratio, (long long)out_total,
                                    (hipStream_t)s, &why, &bad);
  char gt[96] = "";
  if (rc) rhythm_geom_text(geom, gt, sizeof(gt));
  return table_done("rhythm_pool", rc, why, bad, "rows=%d capacity=%lld leads=%d hist_len=%d x_total=%lld new_total=%lld "
                    "out_total=%lld scratch_bytes=%lld %s", rows, (long long)capacity, leads, hist_len, (long long)x_total,
                    (long long)new_total, (long long)out_total, (long long)scratch_bytes, gt);
}

int ral_delineate_records(const float* x, int64_t R, int leads, int64_t T, const ral_delin_geom* geom, const int32_t* peaks,
                          const int32_t* count, int64_t cap, int32_t* on, int32_t* off, int32_t* tpeak, int32_t* tend, ral_stream s) {
  if (!x || !geom || !peaks || !count || !on || !off || !tpeak || !tend) return ral_fail("delineate_records: null pointer");
  const char* why = nullptr;
  if (launch_delineate_records(x, (long long)R, leads, (long long)T, geom, peaks, count, (long long)cap, on, off, tpeak, tend,
                               (hipStream_t)s, &why))
    return ral_fail("delineate_records: need %s (R=%lld leads=%d T=%lld cap=%lld h=%d m=%d Wq=%d g=%d m2=%d gt=%d Wt=%d q0=%g)", why,
                    (long long)R, leads, (long long)T, (long long)cap, geom->h, geom->m, geom->wq, geom->g, geom->m2, geom->gt,
                    geom->wt, geom->q0);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_pst_records(const float* x, int64_t R, int leads, int64_t T, const ral_pst_geom* geom, const int32_t* peaks,
                    const int32_t* count, int64_t cap, const int32_t* on, const int32_t* off, int32_t* pon, int32_t* ppeak,
                    int32_t* poff, float* st, ral_stream s) {
  if (!x || !geom || !peaks || !count || !on || !off || !pon || !ppeak || !poff || !st) return ral_fail("pst_records: null pointer");
  const char* why = nullptr;
  if (launch_pst_records(x, (long long)R, leads, (long long)T, geom, peaks, count, (long long)cap, on, off, pon, ppeak, poff, st,
                         (hipStream_t)s, &why))
    return ral_fail("pst_records: need %s (R=%lld leads=%d T=%lld cap=%lld m2=%d g=%d Wp=%d j=%d w=%g p0=%g)", why, (long long)R,
                    leads, (long long)T, (long long)cap, geom->m2, geom->g, geom->wp, geom->j, geom->w, geom->p0);
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_template_records(const float* x, int64_t R, int leads, int64_t T, const ral_template_geom* geom, const int32_t* peaks,
                         const int32_t* label_or_null, const int32_t* count, int64_t cap, int64_t nw, float* tpl, int32_t* used,
                         int32_t* total, int32_t* rr, ral_stream s) {
  const char* why = nullptr;
  if (launch_template_records(x, (long long)R, leads, (long long)T, geom, peaks, label_or_null, count, (long long)cap,
                              (long long)nw, tpl, used, total, rr, (hipStream_t)s, &why)) {
    const ral_template_geom none = {0, 0, 0, 0, 0}, *g = geom ? geom : &none;
    return ral_fail("ral_template_records: %s (R=%lld leads=%d T=%lld cap=%lld nw=%lld wpre=%d wpost=%d w=%d h=%d kmax=%d)", why,
                    (long long)R, leads, (long long)T, (long long)cap, (long long)nw, g->wpre, g->wpost, g->w, g->h, g->kmax);
  }
  HIP_OK(hipGetLastError());
  return 0;
}

int ral_hrv_windows(const int32_t* pos, const int32_t* label_or_null, const int32_t* count, int64_t R, int64_t cap,
                    const ral_hrv_row* table, int64_t rows, ral_hrv_row* table_dev, int upload, const ral_hrv_geom* geom,
                    const int32_t* band, int32_t* counts, float* stats, float* psd_or_null, ral_stream s) {
  if (!pos || !count || !table_dev || (upload && !table) || !geom || !band || !counts || !stats)
    return ral_fail("hrv_windows: null pointer");
  const char* why = nullptr;
  long long bad = -1;
  const int rc = launch_hrv_windows(pos, label_or_null, count, (long long)R, (long long)cap, table, (long long)rows, table_dev,
                                    upload, geom, band, counts, stats, psd_or_null, (hipStream_t)s, &why, &bad);
  return table_done("hrv_windows", rc, why, bad, "R=%lld cap=%lld rows=%lld W=%d lo_n=%d hi_n=%d t50=%d F=%d min_nn=%d fs=%g",
                    (long long)R, (long long)cap, (long long)rows, geom->W, geom->lo_n, geom->hi_n, geom->t50, geom->F,
                    geom->min_nn, geom->fs);
}

int ral_arrhythmia_windows(const int32_t* peaks, const int32_t* label_or_null, const int32_t* count, const int32_t* on_or_null,
                           const int32_t* ppeak_or_null, int64_t R, int64_t cap, const ral_hrv_row* table, int64_t rows,
                           ral_hrv_row* table_dev, int upload, const ral_arrhythmia_geom* geom, int32_t* counts, float* stats,
                           int32_t* flags, ral_stream s) {
  static const char NAME[] = "ral_arrhythmia_windows";
  // (the host table is read only when it is uploaded: without upload NAME stands in for it as something non-null)
  const struct { const void* p; const char* name; } need[] = {{peaks, "peaks"}, {count, "count"}, {table_dev, "table_dev"},
      {upload ? (const void*)table : (const void*)NAME, "table"}, {geom, "geom"}, {counts, "counts"}, {stats, "stats"}, {flags, "flags"}};
  for (const auto& a : need)
    if (!a.p) return ral_fail("%s: need a non-null %s", NAME, a.name);
  if (!on_or_null != !ppeak_or_null)
    return ral_fail("%s: need on and ppeak together or neither (%s is null)", NAME, on_or_null ? "ppeak" : "on");
  const char* why = nullptr;
  long long bad = -1;
  const int rc = launch_arrhythmia_windows(peaks, label_or_null, count, on_or_null, ppeak_or_null, (long long)R, (long long)cap, table,
                                           (long long)rows, table_dev, upload, geom, counts, stats, flags, (hipStream_t)s, &why, &bad);
  return table_done(NAME, rc, why, bad, "R=%lld cap=%lld rows=%lld W=%d lo_n=%d hi_n=%d bin=%d G=%d lock_n=%d prmax=%d pause_n=%d "
                    "min_m=%d vrun_min=%d n0=%g c0=%g pl0=%g tachy=%g brady=%g fs=%g", (long long)R, (long long)cap, (long long)rows,
                    geom->W, geom->lo_n, geom->hi_n, geom->bin, geom->G, geom->lock_n, geom->prmax, geom->pause_n, geom->min_m,
                    geom->vrun_min, geom->n0, geom->c0, geom->pl0, geom->tachy, geom->brady, geom->fs);
}

int ral_wavelet_denoise(const float* x, float* y, int64_t rows, int L, float threshold, ral_stream s) {
  if (!x || !y) return ral_fail("wavelet_denoise: null pointer");
  if (!(threshold >= 0.f)) return ral_fail("wavelet_denoise: the threshold factor must be non-negative (got %g)", (double)threshold);
  if (launch_wavelet_denoise(x, y, (long long)rows, L, threshold, (hipStream_t)s))
    return ral_fail("wavelet_denoise: need rows >= 0 and an even record length <= 8192 (rows=%lld L=%d)", (long long)rows, L);
  HIP_OK(hipGetLastError());
  return 0;
}

static int fft_denoise_counts(const char* who, int64_t groups, int rows_per_group, int L) {
  if (groups < 0 || rows_per_group < 1)
    return ral_fail("%s: need groups >= 0 and rows_per_group >= 1 (groups=%lld rows_per_group=%d)", who, (long long)groups, rows_per_group);
  if (groups > 0x7fffffffLL / rows_per_group)
    return ral_fail("%s: need groups * rows_per_group < 2^31 (groups=%lld rows_per_group=%d)", who, (long long)groups, rows_per_group);
  if (fft_denoise_scratch_bytes(0, 1, L) < 0) return ral_fail("%s: L=%d is not supported: need %s", who, L, fft_denoise_rule());
  return 0;
}

int64_t ral_fft_denoise_scratch_bytes(int64_t groups, int rows_per_group, int L) {
  if (fft_denoise_counts("fft_denoise_scratch_bytes", groups, rows_per_group, L)) return -1;
  return (int64_t)fft_denoise_scratch_bytes((long long)groups, rows_per_group, L);
}

int ral_fft_denoise(const float* x, float* y, int32_t* kept, int64_t groups, int rows_per_group, int L, float threshold,
                    void* scratch, ral_stream s) {
  if (!x || !y) return ral_fail("fft_denoise: null pointer (x=%p y=%p)", (const void*)x, (void*)y);
  if (fft_denoise_counts("fft_denoise", groups, rows_per_group, L)) return -1;
  if (!(threshold >= 0.f)) return ral_fail("fft_denoise: the threshold factor must be non-negative (got %g)", (double)threshold);
  const long long need = fft_denoise_scratch_bytes((long long)groups, rows_per_group, L);
  if (need > 0 && !scratch)
    return ral_fail("fft_denoise: null scratch, %lld bytes are needed (groups=%lld rows_per_group=%d L=%d)", need, (long long)groups,
                rows_per_group, L);
  const int rc = launch_fft_denoise(x, y, kept, (long long)groups, rows_per_group, L, threshold, scratch, (hipStream_t)s);
  if (rc == -2) return ral_fail("fft_denoise: %s", hipGetErrorString(hipGetLastError()));
  if (rc) return ral_fail("fft_denoise: refused (groups=%lld rows_per_group=%d L=%d)", (long long)groups, rows_per_group, L);
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
