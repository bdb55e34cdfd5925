// U-Net baseline (model/UNet.py): the entry points only it has (the rest is the model interface of ral_model.hpp).
#pragma once
#include "ral_model.hpp"

struct UNetModel;
UNetModel* unet_model(ral_handle* h);   // null unless h is a U-Net model
// training forward + MSE loss / SNR / RMSE sums + dy in one pass over the output (see unet_forward_loss, ral_unet.hip)
int unet_forward_loss(UNetModel* u, const float* x, const float* target, float* y, int B, float* dy, float* snr, float* rmse,
                      double* loss_sum, double* fin, double fin_scale, int fin3, hipStream_t s);
// staged execution (data-parallel sync-BatchNorm): gwin = windows of the global batch.  nrep: replicas of the BatchNorm records
// the pass adds to - 1: straight into the caller's bn_sums, which a data-parallel caller all-reduces between stages; the
// model's own one-call forward / backward pass UNET_MAXREP.  The same for every call of one pass.
int unet_forward_stage(UNetModel* u, const float* x, int B, int training, int si, int64_t gwin, hipStream_t s, int nrep = 1);
int unet_forward_finish(UNetModel* u, float* y, int B, int training, int64_t gwin, hipStream_t s, int nrep = 1);
int unet_backward_start(UNetModel* u, const float* dy, int B, int64_t gwin, hipStream_t s, int nrep = 1);
int unet_backward_stage(UNetModel* u, int B, int si, int64_t gwin, hipStream_t s, int nrep = 1);
int unet_backward_finish(UNetModel* u, int B, int64_t gwin, hipStream_t s, int nrep = 1);
int unet_stage_bn(int si);
