// The model interface behind ral_handle: what ral_api.hip drives and what each network (RA-LENet, U-Net, ACDAE, DANet)
// provides.  DESIGN.md, "Model interface", says what a further network has to bring.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>
#include "../../include/ralenet.h"

// writes the thread-local message ral_last_error() returns; always -1, so that `return ral_fail(...)` reports an error
int ral_fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));

#define HIP_OK(expr)                                                                         \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess) return ral_fail("%s failed: %s", #expr, hipGetErrorString(e_));    \
  } while (0)

// How an entry point that takes a table ends (ral_api.hip).  rc = 0: launched; what the launches left behind is the result.
// rc = -1, refused: `why` is the one rule that is broken and `bad`, if it is a row's, which row (else -1), then the call's
// arguments as args_fmt words them.  Any other rc: the table did not reach the device.
int table_done(const char* name, int rc, const char* why, long long bad, const char* args_fmt, ...)
    __attribute__((format(printf, 5, 6)));

// ---- the flat parameter / state layout (the state_dict contract of ral_layout_entry) ----
struct ParamEntry {
  std::string name;
  int kind;          // RAL_PARAM, RAL_STATE_F32, RAL_COUNTER_I64, RAL_INDEX_I64
  int64_t offset;    // floats, in the parameter or the state buffer
  int ndim;
  int64_t shape[4];
};

struct ParamLayout {
  std::vector<ParamEntry> entries;
  int64_t nparam = 0, nstate = 0;

  // n floats at the end of the parameter buffer, rounded up to `granule` floats (a power of two)
  int64_t alloc(int64_t n, int granule) {
    const int64_t o = nparam;
    nparam += (n + granule - 1) & ~int64_t(granule - 1);
    return o;
  }
  void add(const std::string& name, int kind, int64_t offset, const std::vector<int64_t>& shape) {
    ParamEntry e;
    e.name = name; e.kind = kind; e.offset = offset; e.ndim = (int)shape.size();
    for (int i = 0; i < 4; ++i) e.shape[i] = i < e.ndim ? shape[i] : 1;
    entries.push_back(e);
  }
  int copy_out(int idx, char* name, int name_cap, int32_t* kind, int64_t* offset, int32_t* ndim, int64_t shape[4]) const;
};

// ---- the model base: a ral_handle IS one of these ----
struct RalKind;
struct ral_handle {
  const RalKind* kind = nullptr;   // kind and cfg: set by ral_create, before init()
  ral_config cfg;
  ParamLayout lay;
  // the caller's buffers (ral_bind)
  float *params = nullptr, *grads = nullptr, *am = nullptr, *av = nullptr, *state = nullptr;
  double* bn_sums = nullptr;
  char* slab = nullptr;            // the workspace: one device allocation, released by the destructor

  ral_handle() = default;          // (a model is made by `new T()`: members without an initialiser start as zero)
  ral_handle(const ral_handle&) = delete;
  ral_handle& operator=(const ral_handle&) = delete;
  virtual ~ral_handle();
  hipError_t alloc_slab(size_t bytes);

  // everything that can fail while a model is set up: layout, workspace, descriptors.  ral_create deletes the model when
  // it returns non-zero, so a failure is a plain `return ral_fail(...)`
  virtual int init() = 0;
  virtual int bind(float* params, float* grads, float* am, float* av, float* state, double* bn_sums);
  virtual int forward(const float* x, float* y, int B, int training, hipStream_t s) = 0;
  virtual int backward(const float* dy, float* dx, int B, hipStream_t s) = 0;
  virtual int set_option(const char* key, int value);
  // ral_adam_step is about to overwrite the parameters; returns 64 doubles for the optimiser kernel to zero, or null
  virtual double* after_adam() { return nullptr; }
};

// ---- what is known about a network before a model exists; ral_api.hip keeps one table of these, indexed by variant
// (a function-local static per network: a namespace-scope constant would also be emitted for the device) ----
struct RalKind {
  int (*check_cfg)(const ral_config* c);
  void (*layout)(const ral_config& c, ParamLayout& L);
  size_t (*workspace_bytes)(const ral_config& c);
  int64_t bn_sums_doubles;
  ral_handle* (*create)();                      // `new T()` of the network's model, nothing else: init() does the work
  const char* no_forward_begin;                 // why ral_forward_begin / _end refuse this network (null: they apply)
};
const RalKind *ralenet_kind(), *unet_kind(), *acdae_kind(), *danet_kind();
