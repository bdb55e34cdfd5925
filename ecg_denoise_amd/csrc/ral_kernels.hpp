// Host-side launch interface of the RA-LENet / U-Net kernels (internal to libralenet).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "ral_device.hpp"
#include "ral_attn_plan.hpp"
#include "ral_block_plan.hpp"
#include "../../include/ralenet.h"   // ral_pool_row

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
void launch_conv1_fwd(int leads, int mode, const float* x, const float* w, const float* b, float* out, double* stats,
                      const float* bnw, const float* bnb, const float* rmean, const float* rvar, int L, int Lp /* token slots per window (>= L) */, int B,
                      hipStream_t s);
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

int launch_prep_windows(const float* sig, const float* noise, long long T, int leads, int L, double snr_db, double* sums,
                        float* noisy, float* clean, hipStream_t s);
int launch_stream_windows(const float* rec, long long R, long long T, int leads, int L, int hop, long long w0, int nw,
                          float* win, float* stats, hipStream_t s);
int launch_stream_stitch(const float* y, const float* stats, long long R, long long T, int leads, int L, int hop, float* out,
                         hipStream_t s);
// live streams (ral_live_windows / ral_live_emit); -1: bad arguments
int launch_live_windows(const float* hist, const float* x, float* hist_out, long long S, int leads, int L, int hop, int C,
                        long long base, long long k0, int nw, long long T, long long w0, int nb, float* win, float* stats,
                        hipStream_t s);
int launch_live_emit(const float* y, const float* stats, long long S, int leads, int L, int hop, long long k0, int nw, long long T,
                     long long w0, int nb, long long lo, int m, float* out, float* last_y, float* last_stats, hipStream_t s);
// the 12-lead adapter around the inner model of a streamed record group (ral_newrale_stream_front / _back); -1: bad arguments
int launch_newrale_front(const float* rec, long long R, long long T, int L, int hop, long long w0, int nw, const float* prm,
                         float* inner, float* stats, hipStream_t s);
int launch_newrale_back(const float* iy, const float* stats, const float* prm, long long R, long long T, int L, int hop,
                        long long w0, int nw, float* out, hipStream_t s);
// the same kernels on live 12-lead streams (ral_newrale_live_front / _back; the geometry of launch_live_*); -1: bad arguments
int launch_newrale_live_front(const float* hist, const float* x, float* hist_out, long long S, int L, int hop, int C,
                              long long base, long long k0, int nw, long long T, long long w0, int nb, const float* prm,
                              float* inner, float* stats, hipStream_t s);
int launch_newrale_live_back(const float* iy, const float* stats, const float* prm, long long S, int L, int hop, long long k0,
                             int nw, long long T, long long w0, int nb, long long lo, int m, float* out, float* last_y,
                             float* last_stats, hipStream_t s);
// the stream pool (ral_pool_windows / ral_pool_emit, ral_newrale_pool_front / _back): the host table is checked, then copied to
// tab_dev on s (upload != 0), then the kernel is launched; -1: bad arguments (*why: the rule that is broken, *bad: the row that breaks it or -1), -2: the copy failed
int launch_pool_windows(float* hist, const float* x, long long x_total, const ral_pool_row* tab, int rows, ral_pool_row* tab_dev,
                        int upload, long long cap, int leads, int L, int hop, int write_hist, long long w0, int nb, float* win,
                        float* stats, hipStream_t s, const char** why, int* bad);
int launch_pool_emit(const float* y, const float* stats, const ral_pool_row* tab, int rows, ral_pool_row* tab_dev, int upload,
                     long long cap, int leads, int L, int hop, long long w0, int nb, int from_last, float* out,
                     long long out_total, float* last_y, float* last_stats, hipStream_t s, const char** why, int* bad);
int launch_newrale_pool_front(float* hist, const float* x, long long x_total, const ral_pool_row* tab, int rows,
                              ral_pool_row* tab_dev, int upload, long long cap, int L, int hop, int write_hist, long long w0,
                              int nb, const float* prm, float* inner, float* stats, hipStream_t s, const char** why, int* bad);
int launch_newrale_pool_back(const float* iy, const float* stats, const float* prm, const ral_pool_row* tab, int rows,
                             ral_pool_row* tab_dev, int upload, long long cap, int L, int hop, long long w0, int nb, int from_last,
                             float* out, long long out_total, float* last_y, float* last_stats, hipStream_t s, const char** why,
                             int* bad);
// noise-stress evaluation of record groups (ral_eval.hip; ral_mix_records / ral_score_records): the arguments are checked, then
// (mix) the host arrays copied into the scratch on s, then the kernels launched; -1: bad arguments (*why: the rule that is
// broken, *bad: the record that breaks it or -1), -2: the copy failed.  *_scratch_bytes: -1 for a shape the call would refuse
long long mix_records_scratch_bytes(long long R, int leads, long long T);
int launch_mix_records(const float* rec, const float* noise, long long R, int leads, long long T, long long Tn,
                       const int64_t* offsets, const double* snr_db, void* scratch, float* noisy, float* clean, hipStream_t s,
                       const char** why, long long* bad);
long long score_records_scratch_bytes(long long R, int leads, long long T, long long W);
int launch_score_records(const float* clean, const float* out, const float* noisy, long long R, int leads, long long T, long long W,
                         void* scratch, double* per_lead, double* per_record, double* per_window, double* window_mean,
                         hipStream_t s, const char** why);
// on-the-fly noise mixing of training batches (ral_augment.hip; ral_mix_batch / ral_mix_draw).  The geometry travels by value, as
// a kernel argument (thresholds included: no copy).  mix_batch_check: the broken rule, or nullptr; launch_mix_batch checks, then
// launches one kernel; -1: bad arguments (*why: the rule that is broken).  mix_batch_draw: the draw of ordinal g on the host, by
// the code the kernel runs (the geometry must have passed the check)
struct MixBatchGeom {
  long long N, Lsrc, Tn;
  int leads, L, K;
  uint32_t cum[RAL_MIX_MAX_KINDS];
  double snr_lo, snr_hi;
  uint64_t seed, first;
};
const char* mix_batch_check(const MixBatchGeom& G);
void mix_batch_draw(const MixBatchGeom& G, uint64_t g, int32_t* draw, double* snr_db);
int launch_mix_batch(const float* bank, const float* noise, const int64_t* rows, const MixBatchGeom& G, long long B, float* noisy,
                     float* clean, int32_t* draws, double* snr_db, hipStream_t s, const char** why);
// sample-rate conversion (ral_rate.hip; ral_rate_records / ral_rate_pool): the arguments (and, with upload != 0, the host table)
// are checked, the table copied to tab_dev on s, the kernel launched; -1: bad arguments (*why: the rule that is broken, *bad:
// the row that breaks it or -1), -2: the copy failed
int launch_rate_records(const float* x, long long R, int leads, long long T, int up, int down, const float* bank, int ntaps,
                        float* y, long long T_out, hipStream_t s, const char** why);
int launch_rate_pool(float* hist, const float* x, long long x_total, const ral_rate_row* tab, int rows, ral_rate_row* tab_dev,
                     int upload, long long cap, int leads, int up, int down, const float* bank, int ntaps, int hist_len,
                     float* out, long long out_total, hipStream_t s, const char** why, int* bad);
// beat detection (ral_beats.hip; ral_beat_records / ral_beat_pool / ral_beat_match): the arguments (and, with upload != 0, the host
// table) are checked, the table copied to tab_dev on s, the kernels launched; -1: bad arguments (*why: the rule that is broken,
// *bad: the row that breaks it or -1), -2: the copy failed.  beat_records_scratch_bytes: -1 for a shape the call would refuse
long long beat_records_scratch_bytes(long long R, int leads, long long T, const ral_beat_geom* geom, const char** why);
int launch_beat_records(const float* x, long long R, int leads, long long T, const ral_beat_geom* geom, const float* bank, int ntaps,
                        void* scratch, long long scratch_bytes, int* peaks, long long cap, int* count, hipStream_t s,
                        const char** why);
int launch_beat_pool(float* hist, const float* x, long long x_total, const ral_beat_row* tab, int rows, ral_beat_row* tab_dev,
                     int upload, long long cap, int leads, const ral_beat_geom* geom, const float* bank, int ntaps, int hist_len,
                     void* scratch, long long scratch_bytes, long long* peaks, long long peaks_total, int* count, hipStream_t s,
                     const char** why, int* bad);
int launch_beat_match(const int* ref, const int* nref, long long ref_cap, const int* det, const int* ndet, long long det_cap,
                      long long R, long long tol, long long* out, hipStream_t s, const char** why);
// heart-rate variability (ral_hrv.hip; ral_hrv_windows): -1 with *why (and *bad, the table row, or -1) for a refusal, -2 when the
// table's copy failed
int launch_hrv_windows(const int* pos, const int* label, const int* count, long long R, long long cap, const ral_hrv_row* tab,
                       long long rows, ral_hrv_row* tab_dev, int upload, const ral_hrv_geom* geom, const int* band, int* counts,
                       float* stats, float* psd, hipStream_t s, const char** why, long long* bad);
// rhythm findings (ral_arrhythmia.hip; ral_arrhythmia_windows): the conventions of launch_hrv_windows
int launch_arrhythmia_windows(const int* peaks, const int* label, const int* count, const int* on, const int* ppeak, long long R,
                              long long cap, const ral_hrv_row* tab, long long rows, ral_hrv_row* tab_dev, int upload,
                              const ral_arrhythmia_geom* geom, int* counts, float* stats, int* flags, hipStream_t s,
                              const char** why, long long* bad);
// beat classes (ral_rhythm.hip;ral_rhythm_records / ral_rhythm_pool): the same conventions as beat detection above
long long rhythm_pool_scratch_bytes(long long beats, int leads, const ral_rhythm_geom* geom, const char** why);
int launch_rhythm_records(const float* x, long long R, int leads, long long T, const ral_rhythm_geom* geom, const int* peaks,
                          const int* count, long long cap, int* label, float* corr, float* rr, hipStream_t s, const char** why);
int launch_rhythm_pool(const float* hist, const float* x, long long x_total, const ral_rhythm_row* tab, int rows,
                       ral_rhythm_row* tab_dev, int upload, long long cap, int leads, const ral_rhythm_geom* geom, int hist_len,
                       float* ring, long long* ring_pos, const long long* new_pos, long long new_total, void* scratch,
                       long long scratch_bytes, long long* out_pos, int* label, float* corr, float* rr, long long out_total,
                       hipStream_t s, const char** why, int* bad);
// beat delineation (ral_delineate.hip; ral_delineate_records): -1 with *why for a refusal, before any launch
int launch_delineate_records(const float* x, long long R, int leads, long long T, const ral_delin_geom* geom, const int* peaks,
                             const int* count, long long cap, int* on, int* off, int* tpeak, int* tend, hipStream_t s,
                             const char** why);
// P wave and ST level (ral_pst.hip; ral_pst_records): -1 with *why for a refusal, before any launch
int launch_pst_records(const float* x, long long R, int leads, long long T, const ral_pst_geom* geom, const int* peaks,
                       const int* count, long long cap, const int* on, const int* off, int* pon, int* ppeak, int* poff, float* st,
                       hipStream_t s, const char** why);
// median beats (ral_template.hip; ral_template_records): -1 with *why, which names the argument, before any HIP call
int launch_template_records(const float* x, long long R, int leads, long long T, const ral_template_geom* geom, const int* peaks,
                            const int* label, const int* count, long long cap, long long nw, float* tpl, int* used, int* total,
                            int* rr, hipStream_t s, const char** why);
int launch_conv13_fwd(const float* x, const float* w, const float* b, float* y, int B, int cin, int cout, int L,
                      int lrelu, hipStream_t s, const char** why);   // -1: refused before any HIP call, *why names the argument
int launch_conv13_bwd(const float* x, const float* y, const float* dy, const float* w, float* gw, float* gb,
                      float* dx, int B, int cin, int cout, int L, int lrelu, hipStream_t s, const char** why);

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
void launch_conv1_bwd_dx(int leads, const float* dz, const float* w, float* dx, int L, int Lp, int B, hipStream_t s);

// ---- weight gradients (ral_dw.hip)
bool dw_chunk(int C, int prod /* DW_FC2 .. DW_QKV */, int N, bool split, int* tc, size_t* lds);   // token chunk and LDS of a product; false: no split chunk fits
void launch_block_dw(const BlockPlan& p, const float* dx2, const float* upre, const float* a2c0, const float* dupre, const float* x1,
                     const float* dx1, const float* o_hm, const float* dqkv, const float* x, const float* pe,
                     const BlockP& w, const BlockP& gr, int N, int B, int ksplit, const unsigned* gmax, hipStream_t s);
void launch_resample_dw(int D, bool sep, const float* dy, const float* x, const float* lnw, const float* lnb,
                        float* dW, int T, int Tv, int B, int ksplit, hipStream_t s);

// db8 wavelet-threshold baseline (ral_wavelet.hip); non-zero = rejected arguments
int launch_wavelet_denoise(const float* x, float* y, long long rows, int L, float threshold, hipStream_t s);
// FFT-threshold baseline (ral_fft.hip).  scratch bytes: 0 = one launch, -1 = refused length or counts; launch: -1 = refused
// arguments (fft_denoise_rule names the lengths), -2 = a HIP error
const char* fft_denoise_rule();
long long fft_denoise_scratch_bytes(long long groups, int rows_per_group, int L);
int launch_fft_denoise(const float* x, float* y, int32_t* kept, long long groups, int rows_per_group, int L, float threshold,
                       void* scratch, hipStream_t s);
