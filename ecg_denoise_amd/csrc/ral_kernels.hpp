// Host-side launch interface of the model kernels (internal to libralenet): the launchers that another translation unit
// calls - the networks' passes and the handle entry points of ral_api.hip.  A stateless entry point of the C ABI has no
// launcher here: it is defined in the file that holds its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "ral_device.hpp"
#include "ral_attn_plan.hpp"
#include "ral_block_plan.hpp"

// ---- forward (ral_fwd.hip)
// ---- the Linear layers of a transformer block: ral_block_plan.hpp chooses the kernel, the launchers execute the plan entry they
// are given (each family's launch code sits with its kernel: ral_fwd.hip, ral_bwd.hip, ral_mlpw.hip (strips), ral_dw.hip).  The
// LDS formulas below sit beside their kernels too; the plan calls them.
// Linear layers of the wide levels on the f16 matrix cores (two fp16 pieces per operand, three products per term): the
// weight matrices are re-written once per forward as tiled split planes (launch_tile_planes: desc = int4 {float offset, rows,
// columns, first work item} per matrix, nwork = sum of rows * columns / 8; a matrix's planes sit at twice its float offset
// in `wt`).
void launch_tile_planes(const float* params, void* wt, const void* desc, int ndesc, int nwork, int unscaled_residual, hipStream_t s);
// the activation scales of the nblk transformer blocks (ASC_N floats each; desc: 12 ints per block - see k_act_scales)
void launch_act_scales(const float* params, const void* desc, float* asc, int nblk, hipStream_t s);
size_t qkv_fwd_lds(int C, int N);
size_t qkv_fwd_h_lds(int C, int bufs);
void launch_qkv_fwd(const BlockLaunch& p, const float* x, const float* pe, const BlockP& w, const void* wt /* planes of Wqkv */, float* qkv, int N, int B, hipStream_t s);
size_t mlp_fwd_lds(int C, int N, int nch);
size_t mlp_fwd_h_lds(int C, int T, int nch);
size_t mlp_fwd_w_lds(int C, bool f16);
// pbase / wt: the parameter buffer and the tiled-plane buffer (read by the split-operand kernels only)
void launch_mlp_fwd(const BlockLaunch& p, const float* x, const float* o, const BlockP& w, const float* pbase, const void* wt,
                    float* x1, float* upre, float* x2, int N, int B, hipStream_t s, int NE = 0 /* existing tokens; see launch_attn_fwd */,
                    const float* addend = nullptr, float* sum_out = nullptr /* optional second output: block output + addend */);
void launch_mlp_fwd_w(const BlockLaunch& p, const float* x, const float* o, const BlockP& w, float* x1, float* x2, int N, int B, hipStream_t s);
size_t mlp_bwd_w_lds(int C, bool h16, int* threads);
void launch_mlp_bwd_w(const BlockLaunch& p, const float* dx2, const float* x1, const BlockP& w, const BlockP& gr, float* dx1, float* do_hm, int N, int B,
                      bool want_dw, hipStream_t s);
void launch_resample_fwd(int D, bool sep, const float* x, const float* wred, const float* lnw, const float* lnb,
                         const float* skip, float* y, int T, int Tv /* existing output tokens (<= T slots) */, int B, hipStream_t s);
void launch_add(const float* a, const float* b, float* y, size_t n, hipStream_t s);

// ---- stem / head / loss / optimiser (ral_misc.hip)
// mode 0: training (a0 + statistics sums), 1: eval (x0 from the running statistics), 2: training with frozen BatchNorm (a0 to
// out, x0 to out2, [scale, shift, mean, rstd] of the running statistics to ss; no sums)
void launch_conv1_fwd(int leads, int mode, const float* x, const float* w, const float* b, float* out, double* stats,
                      const float* bnw, const float* bnb, const float* rmean, const float* rvar, int L, int Lp /* token slots per window (>= L) */, int B,
                      hipStream_t s, float* out2 = nullptr, float* ss = nullptr);
// the stem BatchNorm of a training forward: scale / shift / mean / rstd into ss, running statistics updated, x0 = a0 * scale + shift
void launch_bn_train8(const double* stats, double count, const float* bnw, const float* bnb, float* ss, float* rmean, float* rvar,
                      const float* a0, float* x0, size_t ntok, hipStream_t s);
void launch_final_fwd(int leads, const float* u0, const float* x0, const float* w, const float* b, float* y, int L, int Lp,
                      int B, hipStream_t s);
// fin != nullptr: loss_sum is a {double, counter} scratch that is zero on entry and left zero; fin[0] = sum * fin_scale
// fin3: the scratch has 64 doubles (sum [0], counter [16], SNR sum [32], RMSE sum [48]: a cache line each); fin[1], fin[2] = the sums of the windows' SNR / RMSE * fin_scale
void launch_loss(const float* pred, const float* target, float* dy, float* snr, float* rmse, double* loss_sum,
                 int n, int B, float gscale, hipStream_t s, double* fin = nullptr, double fin_scale = 1.0, int fin3 = 0);
// grads[0, nfloat) (nfloat % 4 == 0), sums[0, nsums) and gmax[0, ngmax) = 0 in one launch (nsums, ngmax <= 131072)
void launch_zero_bwd(float* grads, size_t nfloat, double* sums, int nsums, unsigned* gmax, int ngmax, hipStream_t s);
void launch_adam(float* p, const float* g, float* m, float* v, size_t n, double lr, double b1, double b2, double eps,
                 int step, float gscale, hipStream_t s, double* zero64 = nullptr /* optional: 64 doubles cleared by the same launch */);

void launch_transpose_mats(const float* src, float* dst, const void* desc, int nmat, int total, hipStream_t s);

// ---- backward (ral_bwd.hip)
size_t mlp_bwd_lds(int C, int N, int nch);
size_t mlp_bwd_s_lds(int C, int N);
size_t mlp_bwd_s_flush_lds(int C);
size_t mlp_bwd_h_lds(int C, int N, int nch, bool small);
// ptbase / wtt: the transposed-parameter buffer and the tiled split planes of its weight matrices (launch_tile_planes over it)
// gmax (4 unsigned, zeroed by the caller; nullptr unless the plan says dw_split): the split kernels raise it to the bits of the
// largest |dx2|, |du|, |dx1| (mlp) and |dqkv| (qkv) of the launch - the scales of the split weight-gradient products
void launch_mlp_bwd(const BlockLaunch& p, const float* dx2, const float* x1, const float* upre, const BlockP& w,
                    const BlockP& wt, const float* ptbase, const void* wtt, unsigned* gmax, const BlockP& gr, float* dupre, float* dx1, float* do_hm,
                    float* a2c0, int N, int B, bool want_dw, hipStream_t s, int NE = 0 /* existing tokens; see launch_attn_fwd */);
// ---- attention: ral_attn_plan.hpp chooses the kernel, these execute the plan (each family's launch code sits with its kernel:
// ral_fwd.hip, ral_bwd.hip, ral_attn.hip (_w), ral_attnm.hip (_m, _mh))
void launch_attn_fwd(const AttnPlan& p, const float* qkv, float* o_hm, float* lse, const float* table, int N, int H, int Len,
                     int B, hipStream_t s, int NE = 0);
void launch_attn_fwd_w(const AttnPlan& p, const float* qkv, float* o_hm, float* lse, const float* table, int N, int H, int Len, int B, hipStream_t s);
// the reduction of a plan's table partials: recorded into *defer for the caller to launch on the stream of its choice, or
// (defer == nullptr) launched on s behind the kernel
struct AttnTabReduce { const float* tpart; float* gtable; int ntab, nrow; };
void launch_attn_tpart_reduce(const AttnTabReduce& r, hipStream_t s);
// scratch: caller-owned, at least p.scratch_floats floats; non-zero return (nothing launched): it is smaller
int launch_attn_bwd(const AttnPlan& p, const float* qkv, const float* o_hm, const float* do_hm, const float* lse, const float* table,
                    float* gtable, float* dqkv, float* scratch, size_t scratch_floats, int N, int H, int Len, int B, hipStream_t s,
                    int NE = 0, AttnTabReduce* defer = nullptr);
// (_w, _m, _mh: tpart = the scratch; they return the rows of partials they wrote = their grid)
int launch_attn_bwd_w(const AttnPlan& p, const float* qkv, const float* o_hm, const float* do_hm, const float* lse, const float* table,
                      float* dqkv, float* tpart, int N, int H, int Len, int B, hipStream_t s);
int launch_attn_bwd_m(const AttnPlan& p, const float* qkv, const float* o_hm, const float* do_hm, const float* lse, const float* table,
                      float* dqkv, float* tpart, int N, int H, int Len, int B, hipStream_t s);
int launch_attn_bwd_mh(const AttnPlan& p, const float* qkv, const float* o_hm, const float* do_hm, const float* lse, const float* table,
                       float* dqkv, float* tpart, int N, int H, int Len, int B, hipStream_t s);
// grid of a persistent wave-per-head kernel (256 threads, four tasks per workgroup): whole resident rounds, at most max_rows
int attn_wave_grid(const void* kernel, size_t lds, int ntask, int occ_cap, int max_rows);
size_t qkv_bwd_lds(int C, int N);
size_t qkv_bwd_h_lds(int C, int N);
void launch_qkv_bwd(const BlockLaunch& p, const float* dqkv, const float* x, const float* pe, const float* dx1, const float* extra,
                    const BlockP& w, const BlockP& wt, const float* ptbase, const void* wtt /* as launch_mlp_bwd */, unsigned* gmax,
                    const BlockP& gr, float* dx, int N, int B, hipStream_t s);
void launch_resample_bwd(int D, bool sep, const float* dy, const float* x, const float* wred, const float* lnw,
                         float* g_lnw, float* g_lnb, float* dx, int T, int Tv, int B, hipStream_t s);
void launch_final_bwd(int leads, const float* dy, const float* u0, const float* x0, const float* w, float* gw,
                      float* gb, float* dz, int L, int Lp, int B, hipStream_t s);
void launch_bn8_bwd_stats(const float* dy, const float* a0, const float* ss, double* out, size_t ntok, hipStream_t s);
void launch_conv1_bwd(int leads, const float* dy, const float* a0, const float* x, const float* ss, const float* bnw,
                      const double* bst, double count, float* gw, float* gb, float* dz, int L, int Lp, int B, hipStream_t s,
                      float* gbnw, float* gbnb /* BatchNorm affine gradients += the backward sums x share */, double share);
// the same under frozen BatchNorm (ss from launch_conv1_fwd mode 2): d a0 = gamma rstd dy, no sums to read; the affine
// gradients are reduced with the conv gradients
void launch_conv1_bwd_frozen(int leads, const float* dy, const float* a0, const float* x, const float* ss, const float* bnw,
                             float* gw, float* gb, float* dz, int L, int Lp, int B, hipStream_t s, float* gbnw, float* gbnb);
void launch_conv1_bwd_dx(int leads, const float* dz, const float* w, float* dx, int L, int Lp, int B, hipStream_t s);

// ---- weight gradients (ral_dw.hip)
bool dw_chunk(int C, int prod /* DW_FC2 .. DW_QKV */, int N, bool split, int* tc, size_t* lds);   // token chunk and LDS of a product; false: no split chunk fits
void launch_block_dw(const BlockPlan& p, const float* dx2, const float* upre, const float* a2c0, const float* dupre, const float* x1,
                     const float* dx1, const float* o_hm, const float* dqkv, const float* x, const float* pe,
                     const BlockP& w, const BlockP& gr, int N, int B, int ksplit, const unsigned* gmax, hipStream_t s);
void launch_resample_dw(int D, bool sep, const float* dy, const float* x, const float* lnw, const float* lnb,
                        float* dW, int T, int Tv, int B, int ksplit, hipStream_t s);
