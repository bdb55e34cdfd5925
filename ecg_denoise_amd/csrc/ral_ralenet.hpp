// RA-LENet: the entry points only it has (the rest is the model interface of ral_model.hpp).
#pragma once
#include "ral_model.hpp"

struct RalModel;
RalModel* ralenet_model(ral_handle* h);   // null unless h is an RA-LENet model
int ralenet_pe_table(const ral_config* cfg, int level, float* out_host, int64_t cap);
// the forward and the backward in two halves, around the all-reduce of the stem's BatchNorm sums (training; global_windows =
// windows of the global batch); want_dw = 0: frozen weights, data gradients only
int ralenet_forward_begin(RalModel* m, const float* x, int B, hipStream_t s);
int ralenet_forward_end(RalModel* m, float* y, int B, int64_t global_windows, hipStream_t s);
int ralenet_backward_begin(RalModel* m, const float* dy, int B, bool want_dw, hipStream_t s);
int ralenet_backward_end(RalModel* m, float* dx, int B, int64_t global_windows, hipStream_t s);
int ralenet_grad_bucket(RalModel* m, int k, int64_t* offset, int64_t* count);
int ralenet_grad_bucket_wait(RalModel* m, int k, hipStream_t s);
int ralenet_profile_select(RalModel* m, const char* kind);
int ralenet_profile_read(RalModel* m, double* total_ms, int64_t* launches);
int ralenet_profile_timeline(RalModel* m, double* rows, int64_t cap_rows, int64_t* nrows);
int ralenet_debug_tensor(RalModel* m, const char* name, float** ptr, int64_t* numel);
