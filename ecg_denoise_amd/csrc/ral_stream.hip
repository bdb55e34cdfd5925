// Streaming around the inference forward: records, live streams, the 12-lead adapter and the stream pools.  Kernels, the
// host checks of their arguments and tables, and the entry points of the C ABI (ral_stream_*, ral_live_*, ral_newrale_*,
// ral_pool_*): no model calls any of this.  (gfx950)
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_slots.hpp"

#define K13 13   // taps of the adapter convolutions (as ral_misc.hip's k_conv13_*)

// =================================================================================
// Streaming of long records around the inference forward (BASELINE config 5).  The reference cuts the
// 650 000-sample MIT-BIH records into fixed chunks and z-scores them (local_utils/local_utils.py:116-130, np_norm
// :261-266); here a group of R records (R, leads, T) is cut into windows of L samples every `hop` samples (the last
// window of a record is right-aligned), every window is z-scored per lead, and after the model the windows are
// de-normalised and stitched back: overlapping regions keep the centre of each window, the record edges keep the
// whole window.  One wave per (window, lead); mean and standard deviation go to a side buffer for the way back.
// =================================================================================
RAL_DEV void stream_geom(long long T, int L, int hop, int& n_reg, int& n) {
  n_reg = (int)((T - L) / hop) + 1;
  n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
}

// The stitch rule: which window keeps which samples of its record.  h = (L - hop) / 2; window 0 keeps [0, hop + h), window k
// [k hop + h, (k + 1) hop + h), the last window [last_begin, T) (a single window keeps the whole record).  The kept ranges are
// disjoint and cover [0, T): k_stream_stitch maps a sample to its window (stream_owner), k_newrale_back and k_live_emit a window
// to its samples (stream_kept).
struct StreamKeep {
  int n_reg, n, h;
  long long last_begin;   // first sample the last window keeps
};
RAL_DEV StreamKeep stream_keep(long long T, int L, int hop) {
  StreamKeep s;
  stream_geom(T, L, hop, s.n_reg, s.n);
  s.h = (L - hop) >> 1;
  s.last_begin = s.n > 1 ? (long long)(s.n - 2) * hop + L - s.h : 0;
  return s;
}
// A live stream whose end T is not known yet: every window is regular and none is the last (n = n_reg = INT_MAX), so
// stream_start and stream_kept answer for window k < INT_MAX - 1 without reading T.
RAL_DEV StreamKeep stream_keep_open(int L, int hop) {
  StreamKeep s;
  s.n_reg = s.n = 0x7fffffff;
  s.h = (L - hop) >> 1;
  s.last_begin = 0;
  return s;
}
RAL_DEV long long stream_start(const StreamKeep& s, int k, long long T, int L, int hop) {   // first sample of window k
  return k < s.n_reg ? (long long)k * hop : T - L;
}
RAL_DEV int stream_owner(const StreamKeep& s, long long t, int hop) {
  if (s.n == 1 || t >= s.last_begin) return s.n - 1;
  return t < s.h ? 0 : (int)((t - s.h) / hop);
}
RAL_DEV void stream_kept(const StreamKeep& s, int k, long long T, int hop, long long& b, long long& e) {
  b = k == 0 ? 0 : (k == s.n - 1 ? s.last_begin : (long long)k * hop + s.h);
  e = k == s.n - 1 ? T : (long long)(k + 1) * hop + s.h;
}

// The z-score of one lead of one window by one wave (lane = threadIdx.x & 63), src(l) its samples l in [0, L): mean, population
// std with a floor of 1e-6 (as np_norm; constant leads stay finite), dst[l] = (src(l) - mean) / std.  src may read dst.  Every
// window gather (k_stream_windows, k_live_windows, k_newrale_front) runs these sums, so they all produce the same bits.
template <class Src>
RAL_DEV void zscore_wave(const Src& src, float* dst, int L, float& mean, float& sd) {
  const int lane = threadIdx.x & 63;
  float sum = 0.f;
  for (int l = lane; l < L; l += 64) sum += src(l);
  mean = group_sum<64>(sum) / (float)L;
  float ss = 0.f;
  for (int l = lane; l < L; l += 64) { const float d = src(l) - mean; ss = fmaf(d, d, ss); }   // (second pass: L1 hits)
  sd = fmaxf(sqrtf(group_sum<64>(ss) / (float)L), 1e-6f);
  const float inv = 1.0f / sd;
  for (int l = lane; l < L; l += 64) dst[l] = (src(l) - mean) * inv;
}

__global__ __launch_bounds__(64) void k_stream_windows(const float* __restrict__ rec, long long T, int leads, int L, int hop,
                                                       long long w0, float* __restrict__ win, float* __restrict__ stats) {
  int n_reg, n;
  stream_geom(T, L, hop, n_reg, n);
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;   // window of this launch, lead
  const long long gw = w0 + i;
  const long long r = gw / n;
  const int k = (int)(gw - r * n);
  const long long start = k < n_reg ? (long long)k * hop : T - L;
  const float* src = rec + (r * leads + c) * T + start;
  float mean, sd;
  zscore_wave([=](int l) { return src[l]; }, win + ((size_t)i * leads + c) * L, L, mean, sd);
  if (threadIdx.x == 0) { stats[(gw * leads + c) * 2] = mean; stats[(gw * leads + c) * 2 + 1] = sd; }
}

__global__ __launch_bounds__(256) void k_stream_stitch(const float* __restrict__ y, const float* __restrict__ stats, long long R,
                                                       long long T, int leads, int L, int hop, float* __restrict__ out) {
  const StreamKeep sk = stream_keep(T, L, hop);
  const long long total = R * leads * T;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long rc = e / T, t = e - rc * T;
    const long long r = rc / leads;
    const int c = (int)(rc - r * leads);
    const int k = stream_owner(sk, t, hop);
    const long long off = t - stream_start(sk, k, T, L, hop);
    const long long gw = r * sk.n + k;
    const float mean = stats[(gw * leads + c) * 2], sd = stats[(gw * leads + c) * 2 + 1];
    out[e] = fmaf(y[(gw * leads + c) * L + off], sd, mean);
  }
}

static bool stream_windows_args_ok(long long R, long long T, int leads, int L, int hop, long long w0, int nw) {
  if (R < 1 || leads < 1 || L < 64 || L % 64 != 0 || L > 2048 || T < L || hop < 1 || hop > L || nw < 1 || w0 < 0) return false;
  const long long n_reg = (T - L) / hop + 1, n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
  return w0 + nw <= R * n;
}

extern "C" int ral_stream_windows(const float* rec, int64_t R, int64_t T, int leads, int L, int hop, int64_t w0, int nw, float* win,
                                  float* stats, ral_stream s) {
  if (!rec || !win || !stats) return ral_fail("stream_windows: null pointer");
  if (!stream_windows_args_ok(R, T, leads, L, hop, w0, nw))
    return ral_fail("stream_windows: need R >= 1, T >= L, 1 <= hop <= L, L a multiple of 64 and <= 2048, a window range inside the records "
                "(R=%lld T=%lld leads=%d L=%d hop=%d w0=%lld nw=%d)", (long long)R, (long long)T, leads, L, hop, (long long)w0, nw);
  k_stream_windows<<<nw * leads, 64, 0, (hipStream_t)s>>>(rec, T, leads, L, hop, w0, win, stats);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_stream_stitch(const float* y, const float* stats, int64_t R, int64_t T, int leads, int L, int hop, float* out,
                                 ral_stream s) {
  if (!y || !stats || !out) return ral_fail("stream_stitch: null pointer");
  if (R < 1 || leads < 1 || T < L || hop < 1 || hop > L || ((L - hop) & 1))
    return ral_fail("stream_stitch: need R >= 1, T >= L, 1 <= hop <= L with L - hop even (R=%lld T=%lld leads=%d L=%d hop=%d)",
                (long long)R, (long long)T, leads, L, hop);
  const long long total = R * leads * T;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  k_stream_stitch<<<grid, 256, 0, (hipStream_t)s>>>(y, stats, R, T, leads, L, hop, out);
  HIP_OK(hipGetLastError());
  return 0;
}

// =================================================================================
// Live streams (LiveDenoiser, infer.py): S streams advance in lockstep by a chunk of C samples.  A stream keeps the last L
// samples it has received, `hist` (S, leads, L); with the chunk `x` (S, leads, C) they form V = hist ++ x, samples
// [base, base + L + C) of the stream (base = samples received before the chunk - L; positions below 0 are never read).  The
// windows are those of the offline path (stream_keep: T >= 0, the stream ends at T; stream_keep_open: T < 0, the end is not
// known), numbered as there: the windows k0 .. k0 + nw - 1 of every stream, all inside V, are window gw = s nw + j of a call.
// k_live_windows gathers them straight from hist and x and z-scores them (zscore_wave); its workgroups past the windows
// write the last L samples of V to hist_out (another buffer than hist: no workgroup reads what another one writes).
// k_live_emit de-normalises the model output and writes the samples [lo, lo + m) of the stream that the windows keep
// (stream_kept) into out (S, leads, m).  Both take absolute positions; with T < 0 and k0 > 0 their results depend only on
// positions relative to base, so a captured push serves every later push that advances by a multiple of hop.
// =================================================================================
__global__ __launch_bounds__(64) void k_live_windows(const float* __restrict__ hist, const float* __restrict__ x,
                                                     float* __restrict__ hist_out, int leads, int L, int hop, int C,
                                                     long long base, int k0, int nw, long long T, long long w0, int nb,
                                                     float* __restrict__ win, float* __restrict__ stats) {
  const int nwl = nb * leads;
  if ((int)blockIdx.x >= nwl) {   // the history of one (stream, lead): V[C, C + L)
    const size_t sc = blockIdx.x - nwl;
    const float* hr = hist + sc * L;
    const float* xr = x + sc * C;
    float* dst = hist_out + sc * L;
    for (int l = threadIdx.x; l < L; l += 64) dst[l] = C + l < L ? hr[C + l] : xr[C + l - L];
    return;
  }
  const StreamKeep sk = T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop);
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;   // window of this launch, lead
  const long long gw = w0 + i;
  const long long s = gw / nw;
  const int j = (int)(gw - s * nw);
  const int o = (int)(stream_start(sk, k0 + j, T, L, hop) - base);   // the window is V[o, o + L)
  const float* hr = hist + (s * leads + c) * L;
  const float* xr = x + (s * leads + c) * C - L;
  float mean, sd;
  zscore_wave([=](int l) { const int v = o + l; return v < L ? hr[v] : xr[v]; }, win + ((size_t)i * leads + c) * L, L, mean, sd);
  if (threadIdx.x == 0) { stats[(gw * leads + c) * 2] = mean; stats[(gw * leads + c) * 2 + 1] = sd; }
}

// y (nb, leads, L): the model output for windows [w0, w0 + nb) of the call; last_y / last_stats (optional): window j = nw - 1
// of every stream is also kept whole, (S, leads, L) and (S, leads, 2), for a later call with T known.
__global__ __launch_bounds__(64) void k_live_emit(const float* __restrict__ y, const float* __restrict__ stats, int leads, int L,
                                                  int hop, int k0, int nw, long long T, long long w0, long long lo, int m,
                                                  float* __restrict__ out, float* __restrict__ last_y,
                                                  float* __restrict__ last_stats) {
  const StreamKeep sk = T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop);
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;
  const long long gw = w0 + i;
  const long long s = gw / nw;
  const int j = (int)(gw - s * nw), k = k0 + j;
  const long long start = stream_start(sk, k, T, L, hop);
  long long b, e;
  stream_kept(sk, k, T, hop, b, e);
  b = b > lo ? b : lo;                   // (the kept range lies inside the window: stream_kept; clipped to it all the same)
  b = b > start ? b : start;
  e = e < lo + m ? e : lo + m;
  e = e < start + L ? e : start + L;
  const float mean = stats[(gw * leads + c) * 2], sd = stats[(gw * leads + c) * 2 + 1];
  const float* yr = y + ((size_t)i * leads + c) * L;
  float* dst = out + (s * leads + c) * m - lo;
  for (long long t = b + threadIdx.x; t < e; t += 64) dst[t] = fmaf(yr[t - start], sd, mean);
  if (last_y && j == nw - 1) {
    float* ly = last_y + (s * leads + c) * L;
    for (int l = threadIdx.x; l < L; l += 64) ly[l] = yr[l];
    if (threadIdx.x == 0) { last_stats[(s * leads + c) * 2] = mean; last_stats[(s * leads + c) * 2 + 1] = sd; }
  }
}

// The host side of the same geometry (stream_geom / stream_start), for argument checks: window k of a stream ending at T (T < 0:
// open) starts at *start; false if there is no window k.
static bool live_window_start(long long T, int L, int hop, long long k, long long& start) {
  if (T < 0) { start = k * hop; return k < 0x7ffffffeLL; }
  const long long n_reg = (T - L) / hop + 1, n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
  start = k < n_reg ? k * hop : T - L;
  return k < n && n < 0x7fffffffLL;
}

// lmul / lmax: the window lengths of the caller's kernels (L a multiple of lmul in [lmul, lmax])
static bool live_geom_ok(long long S, int leads, int L, int hop, long long k0, int nw, long long T, long long w0, int nb,
                         int lmul = 64, int lmax = 2048) {
  if (S < 1 || leads < 1 || L < lmul || L % lmul != 0 || L > lmax || hop < 1 || hop > L || ((L - hop) & 1)) return false;
  if (nw < 0 || k0 < 0 || nb < 0 || w0 < 0 || (T >= 0 && T < L) || w0 + nb > S * nw) return false;
  long long st;
  return nw == 0 || live_window_start(T, L, hop, k0 + nw - 1, st);
}

// every window k0 .. k0 + nw - 1 inside V: the first one starts at or after base, the last one ends at or before base + L + C
static bool live_windows_in_v(int L, int hop, int C, long long base, long long k0, int nw, long long T) {
  if (nw == 0) return true;
  long long first, last;
  live_window_start(T, L, hop, k0, first);
  live_window_start(T, L, hop, k0 + nw - 1, last);
  return first >= base && last + L <= base + L + C;
}

extern "C" int ral_live_windows(const float* hist, const float* x, float* hist_out, int64_t S, int leads, int L, int hop, int C,
                                int64_t base, int64_t k0, int nw, int64_t T, int64_t w0, int nb, float* win, float* stats,
                                ral_stream s) {
  if (!hist || !x || !win || !stats) return ral_fail("live_windows: null pointer");
  long long grid = 0;
  if (!live_geom_ok(S, leads, L, hop, k0, nw, T, w0, nb) || C < 0 || (nb == 0 && !hist_out) ||
      !live_windows_in_v(L, hop, C, base, k0, nw, T) || (grid = (long long)nb * leads + (hist_out ? S * leads : 0)) > 0x7fffffffLL)
    return ral_fail("live_windows: need S >= 1, leads >= 1, L a multiple of 64 and <= 2048, 1 <= hop <= L with L - hop even, C >= 0, "
                "T < 0 or T >= L, windows k0 .. k0 + nw - 1 of the stream inside samples [base, base + L + C), a window range "
                "inside the S * nw windows, and nb >= 1 or a history to write (S=%lld leads=%d L=%d hop=%d C=%d base=%lld k0=%lld "
                "nw=%d T=%lld w0=%lld nb=%d)", (long long)S, leads, L, hop, C, (long long)base, (long long)k0, nw, (long long)T,
                (long long)w0, nb);
  k_live_windows<<<(int)grid, 64, 0, (hipStream_t)s>>>(hist, x, hist_out, leads, L, hop, C, base, (int)k0, nw, T, w0, nb, win, stats);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_live_emit(const float* y, const float* stats, int64_t S, int leads, int L, int hop, int64_t k0, int nw, int64_t T,
                             int64_t w0, int nb, int64_t lo, int m, float* out, float* last_y, float* last_stats, ral_stream s) {
  if (!y || !stats || !out) return ral_fail("live_emit: null pointer");
  if (!live_geom_ok(S, leads, L, hop, k0, nw, T, w0, nb) || nb < 1 || lo < 0 || m < 0 || (!last_y != !last_stats) ||
      (long long)nb * leads > 0x7fffffffLL)
    return ral_fail("live_emit: need S >= 1, leads >= 1, L a multiple of 64 and <= 2048, 1 <= hop <= L with L - hop even, "
                "T < 0 or T >= L with windows k0 .. k0 + nw - 1 in the stream, a window range of nb >= 1 windows inside the "
                "S * nw, lo >= 0, m >= 0, and last_y and last_stats both given or both null (S=%lld leads=%d L=%d hop=%d "
                "k0=%lld nw=%d T=%lld w0=%lld nb=%d lo=%lld m=%d)", (long long)S, leads, L, hop, (long long)k0, nw, (long long)T,
                (long long)w0, nb, (long long)lo, m);
  k_live_emit<<<nb * leads, 64, 0, (hipStream_t)s>>>(y, stats, leads, L, hop, (int)k0, nw, T, w0, lo, m, out, last_y, last_stats);
  HIP_OK(hipGetLastError());
  return 0;
}

// =================================================================================
// Record streaming through the 12-lead adapter (NewRALE, reference model/ralenet_12leads.py:698-709): the steps around the
// inner RA-LENet as two kernels.  k_newrale_front: window gather + per-lead z-score (k_stream_windows' arithmetic) + conv1
// (12 -> 6) + conv2 (6 -> 2) -> the inner model's input (nw, 2, L).  k_newrale_back: conv3 (2 -> 6) + conv4 (6 -> 12) +
// de-normalisation, written straight into the record for the samples the window keeps (k_stream_stitch's rule).
// One workgroup per window, the whole window staged in LDS with a 6-sample zero halo on each row (the Conv1d padding of
// every adapter conv): at L = 1024 the front kernel holds 12 + 6 rows of 1036 floats (75 KB, two workgroups per CU), the
// back kernel 2 + 6 rows (33 KB).  Every thread computes 4 consecutive samples of every output channel from a 16-sample
// register window per input row; the weights are wave-uniform loads from the parameter buffer.  The sums run in
// k_conv13_fwd's order (bias, then input channel, then tap), so the results equal the unfused launches.
// =================================================================================
#define NR_LEADS 12
#define NR_MID 6
#define NR_PT 4   // consecutive output samples per thread
// offsets in the adapter's flat parameter buffer (NewRALE.SHAPES, every tensor padded to a multiple of 4 floats)
#define NR_C1W 0
#define NR_C1B 936
#define NR_C2W 944
#define NR_C2B 1100
#define NR_C3W 1104
#define NR_C3B 1260
#define NR_C4W 1268
#define NR_C4B 2204

// acc[co][p] = b[co] + sum_ci sum_k w[(co CIN + ci) 13 + k] * xs[ci LP + l0 + p + k]: output samples l0 .. l0 + 3 of a
// Conv1d(CIN, COUT, k13, p6) whose input rows (stride LP) carry a 6-sample halo in front (l0 % 4 == 0, LP % 4 == 0)
template <int CIN, int COUT>
RAL_DEV void conv13_tile(const float* __restrict__ xs, int LP, int l0, const float* __restrict__ w, const float* __restrict__ b,
                         float (&acc)[COUT][NR_PT]) {
#pragma unroll
  for (int co = 0; co < COUT; ++co)
#pragma unroll
    for (int p = 0; p < NR_PT; ++p) acc[co][p] = b[co];
  for (int ci = 0; ci < CIN; ++ci) {
    float xr[NR_PT + 12];
    const float4* xv = reinterpret_cast<const float4*>(xs + ci * LP + l0);
#pragma unroll
    for (int j = 0; j < (NR_PT + 12) / 4; ++j) {
      const float4 v = xv[j];
      xr[4 * j] = v.x; xr[4 * j + 1] = v.y; xr[4 * j + 2] = v.z; xr[4 * j + 3] = v.w;
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
      for (int k = 0; k < K13; ++k) {
        const float wk = w[(co * CIN + ci) * K13 + k];
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) acc[co][p] = fmaf(wk, xr[p + k], acc[co][p]);
      }
  }
}

RAL_DEV float lrelu001(float v) { return v > 0.f ? v : 0.01f * v; }

// zero the halo columns [0, 6) and [L + 6, L + 12) of `rows` rows of stride L + 12 (the window loops write the interiors only)
RAL_DEV void zero_halos(float* xs, int rows, int L) {
  for (int i = threadIdx.x; i < rows * 12; i += blockDim.x) {
    const int row = i / 12, j = i - row * 12;
    xs[row * (L + 12) + (j < 6 ? j : L + j)] = 0.f;
  }
}

// The record kernels and the live ones are ONE body each, templated on where a window comes from (k_newrale_front) and where
// its kept samples go (k_newrale_back): the live bits equal the record bits by construction.
// Window sources: window(sk, i, src) returns the number gw of window i of the launch (its stats slot) and sets the reader
// src(c, l) of its sample l of lead c; write_history is what the workgroups past the windows do (live calls only).
struct NrRecordWindows {   // windows [w0, w0 + nw) of a record group (R, 12, T), numbered as in k_stream_windows
  const float* rec;
  long long T, w0;
  int L, hop;
  struct Reader {
    const float* p;
    long long T;
    RAL_DEV float operator()(int c, int l) const { return p[c * T + l]; }
  };
  RAL_DEV StreamKeep keep() const { return stream_keep(T, L, hop); }
  RAL_DEV long long window(const StreamKeep& sk, int i, Reader& src) const {
    const long long gw = w0 + i, r = gw / sk.n;
    const int k = (int)(gw - r * sk.n);
    src.p = rec + r * NR_LEADS * T + stream_start(sk, k, T, L, hop);
    src.T = T;
    return gw;
  }
  RAL_DEV void write_history(int, int) const {}
};

struct NrLiveWindows {     // a live call (k_live_windows' geometry, 12 leads): window gw = s nw + j is window k0 + j of stream s
  const float* hist;       // (S, 12, L)
  const float* x;          // (S, 12, C)
  float* hist_out;         // (S, 12, L) or null
  long long S, base, T, w0;
  int L, hop, C, k0, nw;
  struct Reader {          // the window is V[o, o + L) of V = hist ++ x
    const float* hr;
    const float* xr;
    int o, L, C;
    RAL_DEV float operator()(int c, int l) const { const int v = o + l; return v < L ? hr[c * L + v] : xr[c * C + v]; }
  };
  RAL_DEV StreamKeep keep() const { return T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop); }
  RAL_DEV long long window(const StreamKeep& sk, int i, Reader& src) const {
    const long long gw = w0 + i, s = gw / nw;
    const int j = (int)(gw - s * nw);
    src.o = (int)(stream_start(sk, k0 + j, T, L, hop) - base);
    src.hr = hist + s * NR_LEADS * L;
    src.xr = x + s * NR_LEADS * C - L;
    src.L = L;
    src.C = C;
    return gw;
  }
  // workgroup g of ng writes V[C, C + L) of the (stream, lead) rows g, g + ng, ... into hist_out (another buffer than hist)
  RAL_DEV void write_history(int g, int ng) const {
    for (long long r = g; r < S * NR_LEADS; r += ng) {
      const float* hr = hist + r * L;
      const float* xr = x + r * C;
      float* dst = hist_out + r * L;
      for (int l = threadIdx.x; l < L; l += blockDim.x) dst[l] = C + l < L ? hr[C + l] : xr[C + l - L];
    }
  }
};

// Where the kept samples of a window of k_newrale_back go: window(sk, i) -> its number gw, the samples [ob, oe) of the window
// it keeps, and the element out[dst + c * stride + l] that takes its sample l of lead c; src: where its inner output is read
// (window i of the launch at i * 2 L, a pool's kept window at its slot); ly: where the inner output of the window is kept
// whole (live calls, the last window of every stream), or null.
struct NrKept {
  long long gw, dst, stride;
  long long src;           // the window's inner output is iy[src, src + 2 L)
  int ob, oe;
  float* ly;
};

struct NrRecordKeep {      // into the record group (R, 12, T): k_stream_stitch's rule
  float* out;
  long long T, w0;
  int L, hop;
  RAL_DEV StreamKeep keep() const { return stream_keep(T, L, hop); }
  RAL_DEV NrKept window(const StreamKeep& sk, int i) const {
    NrKept kp;
    kp.gw = w0 + i;
    const long long r = kp.gw / sk.n;
    const int k = (int)(kp.gw - r * sk.n);
    const long long start = stream_start(sk, k, T, L, hop);
    long long kb, ke;
    stream_kept(sk, k, T, hop, kb, ke);
    kp.ob = (int)(kb - start);
    kp.oe = (int)(ke - start);
    kp.dst = r * NR_LEADS * T + start;
    kp.stride = T;
    kp.src = (long long)i * 2 * L;
    kp.ly = nullptr;
    return kp;
  }
  RAL_DEV void keep_stats(const NrKept&, const float*) const {}
};

struct NrLiveKeep {        // into a live call's out (S, 12, m): the samples in [lo, lo + m), sample t at t - lo (k_live_emit)
  float* out;
  float* last_y;           // (S, 2, L) or null
  float* last_stats;       // (S, 12, 2) or null (with last_y)
  long long T, w0, lo;
  int L, hop, k0, nw, m;
  RAL_DEV StreamKeep keep() const { return T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop); }
  RAL_DEV NrKept window(const StreamKeep& sk, int i) const {
    NrKept kp;
    kp.gw = w0 + i;
    const long long s = kp.gw / nw;
    const int j = (int)(kp.gw - s * nw), k = k0 + j;
    const long long start = stream_start(sk, k, T, L, hop);
    long long b, e;
    stream_kept(sk, k, T, hop, b, e);
    b = b > lo ? b : lo;                 // (clipped to the window as in k_live_emit)
    b = b > start ? b : start;
    e = e < lo + m ? e : lo + m;
    e = e < start + L ? e : start + L;
    kp.ob = (int)(b - start);
    kp.oe = e > b ? (int)(e - start) : kp.ob;
    kp.dst = s * NR_LEADS * m + start - lo;   // (negative for start < lo: only l >= ob, t >= lo, is written)
    kp.stride = m;
    kp.src = (long long)i * 2 * L;
    kp.ly = last_y && j == nw - 1 ? last_y + s * 2 * L : nullptr;
    return kp;
  }
  RAL_DEV void keep_stats(const NrKept& kp, const float* stats) const {   // (mean, std) of the 12 leads of a kept window
    if (kp.ly && threadIdx.x < 2 * NR_LEADS)
      last_stats[(kp.gw / nw) * 2 * NR_LEADS + threadIdx.x] = stats[kp.gw * 2 * NR_LEADS + threadIdx.x];
  }
};

// nwg workgroups take the windows [0, nw) of the launch in turn; workgroups nwg .. gridDim.x - 1 write the history
template <class Win>
__global__ __launch_bounds__(256) void k_newrale_front(Win win, int nw, int nwg, const float* __restrict__ prm,
                                                       float* __restrict__ inner, float* __restrict__ stats) {
  if ((int)blockIdx.x >= nwg) {
    win.write_history((int)blockIdx.x - nwg, (int)gridDim.x - nwg);
    return;
  }
  extern __shared__ float4 smem4[];
  const int L = win.L, LP = L + 12;
  float* xs = reinterpret_cast<float*>(smem4);   // 12 x LP: the window, z-scored in place
  float* a1 = xs + NR_LEADS * LP;                // 6 x LP: conv1's output
  zero_halos(xs, NR_LEADS + NR_MID, L);
  const StreamKeep sk = win.keep();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x; i < nw; i += nwg) {
    typename Win::Reader src;
    const long long gw = win.window(sk, i, src);
    __syncthreads();   // (the previous window's readers are done; the halos are written)
    for (int e = threadIdx.x; e < NR_LEADS * L; e += blockDim.x) {
      const int c = e / L, l = e - c * L;
      xs[c * LP + 6 + l] = src(c, l);
    }
    __syncthreads();
    // z-score, one wave per lead (zscore_wave: k_stream_windows' bits)
    for (int c = wave; c < NR_LEADS; c += blockDim.x >> 6) {
      float* row = xs + c * LP + 6;
      float mean, sd;
      zscore_wave([=](int l) { return row[l]; }, row, L, mean, sd);
      if (lane == 0) { stats[(gw * NR_LEADS + c) * 2] = mean; stats[(gw * NR_LEADS + c) * 2 + 1] = sd; }
    }
    __syncthreads();
    for (int l0 = NR_PT * threadIdx.x; l0 < L; l0 += NR_PT * blockDim.x) {   // conv1 + LeakyReLU -> a1
      float acc[NR_MID][NR_PT];
      conv13_tile<NR_LEADS, NR_MID>(xs, LP, l0, prm + NR_C1W, prm + NR_C1B, acc);
#pragma unroll
      for (int co = 0; co < NR_MID; ++co)
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) a1[co * LP + 6 + l0 + p] = lrelu001(acc[co][p]);
    }
    __syncthreads();
    for (int l0 = NR_PT * threadIdx.x; l0 < L; l0 += NR_PT * blockDim.x) {   // conv2 + LeakyReLU -> inner (nw, 2, L)
      float acc[2][NR_PT];
      conv13_tile<NR_MID, 2>(a1, LP, l0, prm + NR_C2W, prm + NR_C2B, acc);
#pragma unroll
      for (int co = 0; co < 2; ++co)
        *reinterpret_cast<float4*>(inner + ((size_t)i * 2 + co) * L + l0) =
            make_float4(lrelu001(acc[co][0]), lrelu001(acc[co][1]), lrelu001(acc[co][2]), lrelu001(acc[co][3]));
    }
  }
}

template <class Dst>
__global__ __launch_bounds__(256) void k_newrale_back(Dst dst, int nw, const float* __restrict__ iy,
                                                      const float* __restrict__ stats, const float* __restrict__ prm) {
  extern __shared__ float4 smem4[];
  const int L = dst.L, LP = L + 12;
  float* ys = reinterpret_cast<float*>(smem4);   // 2 x LP: the inner model's output
  float* a3 = ys + 2 * LP;                       // 6 x LP: conv3's output
  zero_halos(ys, 2 + NR_MID, L);
  const StreamKeep sk = dst.keep();
  for (int i = blockIdx.x; i < nw; i += gridDim.x) {
    const NrKept kp = dst.window(sk, i);
    const long long gw = kp.gw;
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * L; e += blockDim.x) {
      const int c = e / L, l = e - c * L;
      const float v = iy[kp.src + e];
      ys[c * LP + 6 + l] = v;
      if (kp.ly) kp.ly[e] = v;
    }
    dst.keep_stats(kp, stats);
    __syncthreads();
    for (int l0 = NR_PT * threadIdx.x; l0 < L; l0 += NR_PT * blockDim.x) {   // conv3 + LeakyReLU -> a3
      float acc[NR_MID][NR_PT];
      conv13_tile<2, NR_MID>(ys, LP, l0, prm + NR_C3W, prm + NR_C3B, acc);
#pragma unroll
      for (int co = 0; co < NR_MID; ++co)
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) a3[co * LP + 6 + l0 + p] = lrelu001(acc[co][p]);
    }
    __syncthreads();
    // conv4 on the 4-sample tiles that hold kept samples; de-normalise; write the kept ones
    for (int l0 = (kp.ob & ~(NR_PT - 1)) + NR_PT * threadIdx.x; l0 < kp.oe; l0 += NR_PT * blockDim.x) {
      float acc[NR_LEADS][NR_PT];
      conv13_tile<NR_MID, NR_LEADS>(a3, LP, l0, prm + NR_C4W, prm + NR_C4B, acc);
#pragma unroll
      for (int c = 0; c < NR_LEADS; ++c) {
        const float mean = stats[(gw * NR_LEADS + c) * 2], sd = stats[(gw * NR_LEADS + c) * 2 + 1];
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) {
          const int l = l0 + p;
          if (l >= kp.ob && l < kp.oe) dst.out[kp.dst + c * kp.stride + l] = fmaf(acc[c][p], sd, mean);
        }
      }
    }
  }
}

static constexpr int NR_GRID = 2048;   // workgroup cap of the windows of one launch (grid-stride beyond)
static size_t newrale_front_lds(int L) { return (size_t)(NR_LEADS + NR_MID) * (L + 12) * sizeof(float); }
static size_t newrale_back_lds(int L) { return (size_t)(2 + NR_MID) * (L + 12) * sizeof(float); }

static bool newrale_stream_args_ok(long long R, long long T, int L, int hop, long long w0, int nw) {
  if (R < 1 || L < 16 || L % 16 != 0 || L > 1024 || T < L || hop < 1 || hop > L || ((L - hop) & 1) || nw < 1 || w0 < 0) return false;
  const long long n_reg = (T - L) / hop + 1, n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
  return n <= 0x7fffffffLL && w0 + nw <= R * n;
}

// the record calls' rule in words, under the name of the call that refuses
static int newrale_stream_refusal(const char* name, long long R, long long T, int L, int hop, long long w0, int nw) {
  return ral_fail("%s: need R >= 1, T >= L, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, "
                  "a window range inside the records (R=%lld T=%lld L=%d hop=%d w0=%lld nw=%d)", name, R, T, L, hop, w0, nw);
}

extern "C" int ral_newrale_stream_front(const float* rec, int64_t R, int64_t T, int L, int hop, int64_t w0, int nw,
                                        const float* adapter_params, float* inner_x, float* stats, ral_stream s) {
  if (!rec || !adapter_params || !inner_x || !stats) return ral_fail("newrale_stream_front: null pointer");
  if (!newrale_stream_args_ok(R, T, L, hop, w0, nw)) return newrale_stream_refusal("newrale_stream_front", R, T, L, hop, w0, nw);
  const size_t lds = newrale_front_lds(L);
  RAL_SET_LDS(k_newrale_front<NrRecordWindows>, lds);
  const int grid = nw < NR_GRID ? nw : NR_GRID;
  k_newrale_front<<<grid, 256, lds, (hipStream_t)s>>>(NrRecordWindows{rec, T, w0, L, hop}, nw, grid, adapter_params, inner_x, stats);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_newrale_stream_back(const float* inner_y, const float* stats, const float* adapter_params, int64_t R, int64_t T,
                                       int L, int hop, int64_t w0, int nw, float* out, ral_stream s) {
  if (!inner_y || !stats || !adapter_params || !out) return ral_fail("newrale_stream_back: null pointer");
  if (!newrale_stream_args_ok(R, T, L, hop, w0, nw)) return newrale_stream_refusal("newrale_stream_back", R, T, L, hop, w0, nw);
  const size_t lds = newrale_back_lds(L);
  RAL_SET_LDS(k_newrale_back<NrRecordKeep>, lds);
  k_newrale_back<<<nw < NR_GRID ? nw : NR_GRID, 256, lds, (hipStream_t)s>>>(NrRecordKeep{out, T, w0, L, hop}, nw, inner_y, stats,
                                                                            adapter_params);
  HIP_OK(hipGetLastError());
  return 0;
}

// Live 12-lead streams (NewRALELiveDenoiser): the record kernels' bodies on k_live_windows' / k_live_emit's geometry.  L as for
// the record kernels (a multiple of 16 in [16, 1024]).
extern "C" int ral_newrale_live_front(const float* hist, const float* x, float* hist_out, int64_t S, int L, int hop, int C,
                                      int64_t base, int64_t k0, int nw, int64_t T, int64_t w0, int nb, const float* adapter_params,
                                      float* inner_x, float* stats, ral_stream s) {
  if (!hist || !x || !adapter_params || !inner_x || !stats) return ral_fail("newrale_live_front: null pointer");
  if (!live_geom_ok(S, NR_LEADS, L, hop, k0, nw, T, w0, nb, 16, 1024) || C < 0 || (nb == 0 && !hist_out) || hist_out == hist ||
      !live_windows_in_v(L, hop, C, base, k0, nw, T))
    return ral_fail("newrale_live_front: need S >= 1, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, C >= 0, "
                "T < 0 or T >= L, windows k0 .. k0 + nw - 1 of the stream inside samples [base, base + L + C), a window range "
                "inside the S * nw windows, and nb >= 1 or a history to write (another buffer than hist) (S=%lld L=%d hop=%d "
                "C=%d base=%lld k0=%lld nw=%d T=%lld w0=%lld nb=%d)", (long long)S, L, hop, C, (long long)base, (long long)k0,
                nw, (long long)T, (long long)w0, nb);
  const long long rows = S * NR_LEADS;
  const int nwg = nb < NR_GRID ? nb : NR_GRID;
  const int nhg = hist_out ? (int)(rows < NR_GRID ? rows : NR_GRID) : 0;    // history workgroups, rows in turn
  const size_t lds = newrale_front_lds(L);
  RAL_SET_LDS(k_newrale_front<NrLiveWindows>, lds);
  k_newrale_front<<<nwg + nhg, 256, lds, (hipStream_t)s>>>(NrLiveWindows{hist, x, hist_out, S, base, T, w0, L, hop, C, (int)k0, nw},
                                                           nb, nwg, adapter_params, inner_x, stats);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_newrale_live_back(const float* inner_y, const float* stats, const float* adapter_params, int64_t S, int L, int hop,
                                     int64_t k0, int nw, int64_t T, int64_t w0, int nb, int64_t lo, int m, float* out,
                                     float* last_y, float* last_stats, ral_stream s) {
  if (!inner_y || !stats || !adapter_params || !out) return ral_fail("newrale_live_back: null pointer");
  if (!live_geom_ok(S, NR_LEADS, L, hop, k0, nw, T, w0, nb, 16, 1024) || nb < 1 || lo < 0 || m < 0 || (!last_y != !last_stats))
    return ral_fail("newrale_live_back: need S >= 1, L a multiple of 16 in [16, 1024], 1 <= hop <= L with L - hop even, "
                "T < 0 or T >= L with windows k0 .. k0 + nw - 1 in the stream, a window range of nb >= 1 windows inside the "
                "S * nw, lo >= 0, m >= 0, and last_y and last_stats both given or both null (S=%lld L=%d hop=%d k0=%lld nw=%d "
                "T=%lld w0=%lld nb=%d lo=%lld m=%d)", (long long)S, L, hop, (long long)k0, nw, (long long)T, (long long)w0, nb,
                (long long)lo, m);
  const size_t lds = newrale_back_lds(L);
  RAL_SET_LDS(k_newrale_back<NrLiveKeep>, lds);
  k_newrale_back<<<nb < NR_GRID ? nb : NR_GRID, 256, lds, (hipStream_t)s>>>(
      NrLiveKeep{out, last_y, last_stats, T, w0, lo, L, hop, (int)k0, nw, m}, nb, inner_y, stats, adapter_params);
  HIP_OK(hipGetLastError());
  return 0;
}

// =================================================================================
// Stream pool (LivePool / NewRALELivePool, infer.py): the live kernels with every per-call scalar replaced by a row of a table,
// ral_pool_row (include/ralenet.h), one row per stream the call names.  The slots, their two history planes of L samples and
// the rows' shared fields follow the slot protocol (ral_slots.hpp); the history workgroups of the call's first gather launch
// write the next history.  V of a row is its history ++ its chunk, samples [n0 - L, n0 + c) of the stream.  Window gw of the
// call is window k0 + (gw - w_off) of the row found by pool_find_row (the rows' w_off are the prefix sums of their nw).  The
// window arithmetic is that of the live kernels: zscore_wave, stream_keep / stream_keep_open, stream_start, stream_kept.
// =================================================================================
typedef ral_pool_row PoolRow;

// the row that holds window gw of the call: the last one with w_off <= gw (rows without windows share the w_off of the next
// row with some, or the total behind the last one, so they are never the answer for gw below the total)
RAL_DEV int pool_find_row(const PoolRow* __restrict__ tab, int rows, long long gw) {
  int a = 0, b = rows - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (tab[mid].w_off <= gw) a = mid; else b = mid - 1;
  }
  return a;
}

// What a workgroup derives from its row is the same in every lane.  Passing it through readfirstlane keeps it in scalar
// registers: observed with -Rpass-analysis=kernel-resource-usage for gfx950, k_newrale_back<NrPoolKeep> needs 135 VGPRs
// without these calls and 110 with them.
RAL_DEV int pool_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
RAL_DEV long long pool_uniform(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

RAL_DEV StreamKeep pool_keep(const PoolRow& t, int L, int hop) { return t.T < 0 ? stream_keep_open(L, hop) : stream_keep(t.T, L, hop); }

// the samples [b, e) of the stream that window k of row t (starting at `start`) gives to this call: what the window keeps
// (stream_kept), inside [lo, lo + m) and inside the window, as k_live_emit clips them
RAL_DEV void pool_kept(const StreamKeep& sk, const PoolRow& t, int k, long long start, int L, int hop, long long& b, long long& e) {
  stream_kept(sk, k, t.T, hop, b, e);
  b = b > t.lo ? b : t.lo;
  b = b > start ? b : start;
  e = e < t.lo + t.m ? e : t.lo + t.m;
  e = e < start + L ? e : start + L;
}

// the next history of (row, lead): V[c, c + L), the last L samples the stream has received after this call
RAL_DEV void pool_write_history(const PoolRow& t, int c, int leads, int L, long long cap, float* hist,
                                const float* __restrict__ x) {
  slot_write_history(hist + slot_plane(t.turn, t.slot, cap, leads, L, c), x + t.x_off * leads + (long long)c * t.c,
                     hist + slot_plane(1 - t.turn, t.slot, cap, leads, L, c), t.n0, t.c, L);
}

__global__ __launch_bounds__(64) void k_pool_windows(float* hist, const float* __restrict__ x, const PoolRow* __restrict__ tab,
                                                     int rows, long long cap, int leads, int L, int hop, long long w0, int nb,
                                                     float* __restrict__ win, float* __restrict__ stats) {
  const int nwl = nb * leads;
  if ((int)blockIdx.x >= nwl) {   // the history of one (row, lead)
    const int rc = blockIdx.x - nwl, r = rc / leads;
    const PoolRow t = tab[r];
    if (t.flags & RAL_POOL_KEEP) pool_write_history(t, rc - r * leads, leads, L, cap, hist, x);
    return;
  }
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;   // window of this launch, lead
  const long long gw = w0 + i;
  const PoolRow t = tab[pool_find_row(tab, rows, gw)];
  const StreamKeep sk = pool_keep(t, L, hop);
  const int j = (int)(gw - t.w_off);
  const int o = (int)(stream_start(sk, (int)t.k0 + j, t.T, L, hop) - (t.n0 - L));   // the window is V[o, o + L)
  const float* hr = hist + slot_plane(t.turn, t.slot, cap, leads, L, c);
  const float* xr = x + t.x_off * leads + (long long)c * t.c - L;
  float mean, sd;
  zscore_wave([=](int l) { const int v = o + l; return v < L ? hr[v] : xr[v]; }, win + ((size_t)i * leads + c) * L, L, mean, sd);
  if (threadIdx.x == 0) { stats[(gw * leads + c) * 2] = mean; stats[(gw * leads + c) * 2 + 1] = sd; }
}

// y (nb, leads, L) and stats: the model output and (mean, std) of windows [w0, w0 + nb) of the call.  from_last: window gw is
// the one window of row gw, and y / stats are the kept windows of the slots, (capacity, leads, L) and (capacity, leads, 2).
__global__ __launch_bounds__(64) void k_pool_emit(const float* __restrict__ y, const float* __restrict__ stats,
                                                  const PoolRow* __restrict__ tab, int rows, int leads, int L, int hop,
                                                  long long w0, int from_last, float* __restrict__ out,
                                                  float* __restrict__ last_y, float* __restrict__ last_stats) {
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;
  const long long gw = w0 + i;
  const PoolRow t = tab[from_last ? (int)gw : pool_find_row(tab, rows, gw)];
  const StreamKeep sk = pool_keep(t, L, hop);
  const int j = from_last ? 0 : (int)(gw - t.w_off), k = (int)t.k0 + j;
  const long long start = stream_start(sk, k, t.T, L, hop);
  long long b, e;
  pool_kept(sk, t, k, start, L, hop, b, e);
  const long long sw = from_last ? (long long)t.slot : gw;            // the window's place in stats
  const float mean = stats[(sw * leads + c) * 2], sd = stats[(sw * leads + c) * 2 + 1];
  const float* yr = y + ((size_t)(from_last ? t.slot : i) * leads + c) * L;
  float* dst = out + t.out_off * leads + (long long)c * t.m - t.lo;
  for (long long p = b + threadIdx.x; p < e; p += 64) dst[p] = fmaf(yr[p - start], sd, mean);
  if (last_y && (t.flags & RAL_POOL_KEEP) && j == t.nw - 1) {
    float* ly = last_y + ((size_t)t.slot * leads + c) * L;
    for (int l = threadIdx.x; l < L; l += 64) ly[l] = yr[l];
    if (threadIdx.x == 0) { last_stats[((size_t)t.slot * leads + c) * 2] = mean; last_stats[((size_t)t.slot * leads + c) * 2 + 1] = sd; }
  }
}

// The table is checked here, on the host, before anything reaches the device (slots_walk, ral_slots.hpp, with the window pools'
// own rules).  -> null if the table is sound, else the rule that is broken, with *bad the row that breaks it (-1: the geometry).
// x_total / out_total: samples per lead in the packed chunk / output buffer (ignored when negative: the emit / gather does not
// touch that buffer).  from_last: the table of an emit of kept windows (one window per row, the last regular one before n0).
// walk = false (a launch that reuses the device copy of a table checked at its upload): the geometry only.
static const char* pool_table_fault(const PoolRow* tab, int rows, long long cap, int leads, int L, int hop, int lmul, int lmax,
                                    long long x_total, long long out_total, bool from_last, bool walk, int* bad) {
  *bad = -1;
  if (rows < 1) return "rows >= 1";
  if (cap < 1) return "capacity >= 1";
  if (leads < 1) return "leads >= 1";
  if (L < lmul || L % lmul != 0 || L > lmax) return lmul == 64 ? "L a multiple of 64 and <= 2048" : "L a multiple of 16 in [16, 1024]";
  if (hop < 1 || hop > L || ((L - hop) & 1)) return "1 <= hop <= L with L - hop even";
  if (!walk) return nullptr;
  const SlotRules rules{L, true, "n0, c, nw, m, k0, lo >= 0 and c < 2^30",
                        "T = n0 + c >= L without RAL_POOL_KEEP, or T = -1 with RAL_POOL_KEEP and c >= 1"};
  long long w_sum = 0;
  auto in_range = [](const PoolRow& t) {
    return !(t.n0 < 0 || t.c < 0 || t.c > 0x3fffffff || t.nw < 0 || t.m < 0 || t.k0 < 0 || t.lo < 0);
  };
  auto early = [&](const PoolRow& t) -> const char* {
    if (t.w_off != w_sum) return "w_off the prefix sum of nw";
    w_sum += t.nw;
    return nullptr;
  };
  auto own = [&](const PoolRow& t) -> const char* {
    if (out_total >= 0 && (t.out_off < 0 || t.out_off + t.m > out_total)) return "the emitted samples inside the packed output";
    if (t.lo + t.m > t.n0 + t.c) return "lo + m <= n0 + c (nothing emitted that was not received)";
    if (from_last) {   // the last regular window complete at n0: it ends at or before n0, the next one would not
      long long st;
      if (t.T < 0 || t.nw != 1 || t.n0 < L || !live_window_start(t.T, L, hop, t.k0, st) || t.k0 * hop + L > t.n0 ||
          (t.k0 + 1) * hop + L <= t.n0)
        return "from_last rows with T known, nw = 1, n0 >= L and k0 the last regular window complete at n0";
    } else if (t.nw > 0) {
      long long first, last;
      if (!live_window_start(t.T, L, hop, t.k0, first) || !live_window_start(t.T, L, hop, t.k0 + t.nw - 1, last))
        return "windows k0 .. k0 + nw - 1 in the stream";
      if (first < t.n0 - L || first < 0) return "the first window at or after the history, max(n0 - L, 0)";
      if (last + L > t.n0 + t.c) return "the last window inside the received samples, n0 + c";
      if (t.lo < first || t.lo + t.m > last + L) return "[lo, lo + m) inside the windows";
    }
    return nullptr;
  };
  if (const char* why = slots_walk(tab, rows, cap, x_total, rules, in_range, early, own, bad)) return why;
  return w_sum <= 0x7fffffffLL ? nullptr : "at most 2^31 - 1 windows";
}

static long long pool_windows_total(const PoolRow* tab, int rows) { return tab[rows - 1].w_off + tab[rows - 1].nw; }

// the checks of a gather / an emit launch: the table (walked when it is uploaded), then the launch's own arguments
static const char* pool_gather_fault(const PoolRow* tab, int rows, long long cap, int leads, int L, int hop, int lmul, int lmax,
                                     long long x_total, int upload, int write_hist, long long w0, int nb, int* bad) {
  *bad = -1;
  if (x_total < 0) return "x_total >= 0";
  if (const char* why = pool_table_fault(tab, rows, cap, leads, L, hop, lmul, lmax, x_total, -1, false, upload != 0, bad)) return why;
  if (w0 < 0 || nb < 0 || w0 + nb > pool_windows_total(tab, rows)) return "a window range inside the call's windows";
  if (nb == 0 && !write_hist) return "nb >= 1 or write_hist";
  if ((long long)nb * leads + (write_hist ? (long long)rows * leads : 0) > 0x7fffffffLL) return "at most 2^31 - 1 workgroups";
  return nullptr;
}

static const char* pool_emit_fault(const PoolRow* tab, int rows, long long cap, int leads, int L, int hop, int lmul, int lmax,
                                   long long out_total, int upload, long long w0, int nb, int from_last, const float* last_y,
                                   const float* last_stats, int* bad) {
  *bad = -1;
  if (out_total < 0) return "out_total >= 0";
  if (const char* why = pool_table_fault(tab, rows, cap, leads, L, hop, lmul, lmax, -1, out_total, from_last != 0, upload != 0, bad))
    return why;
  if (w0 < 0 || nb < 1 || w0 + nb > pool_windows_total(tab, rows)) return "a window range of nb >= 1 windows inside the call's";
  if (!last_y != !last_stats) return "last_y and last_stats both given or both null";
  if (from_last && last_y) return "last_y and last_stats null with from_last";
  if ((long long)nb * leads > 0x7fffffffLL) return "at most 2^31 - 1 workgroups";
  return nullptr;
}

// The four pool entry points: the table is checked (why, bad), then copied to table_dev on s (upload != 0), then the kernel is
// launched; table_done (ral_model.hpp) words the outcome.  `packed`: the x_total of a gather, the out_total of an emit.
static const char POOL_ARGS[] = "rows=%d capacity=%lld L=%d hop=%d packed=%lld w0=%lld nb=%d";

extern "C" int ral_pool_windows(float* hist, const float* x, int64_t x_total, const ral_pool_row* table, int rows,
                                ral_pool_row* table_dev, int upload, int64_t capacity, int leads, int L, int hop, int write_hist,
                                int64_t w0, int nb, float* win, float* stats, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !win || !stats) return ral_fail("pool_windows: null pointer");
  int bad = -1;
  const char* why = pool_gather_fault(table, rows, capacity, leads, L, hop, 64, 2048, x_total, upload, write_hist, w0, nb, &bad);
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc) {
    const long long grid = (long long)nb * leads + (write_hist ? (long long)rows * leads : 0);
    k_pool_windows<<<(int)grid, 64, 0, (hipStream_t)s>>>(hist, x, table_dev, rows, capacity, leads, L, hop, w0, nb, win, stats);
  }
  return table_done("pool_windows", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)x_total, (long long)w0,
                    nb);
}

extern "C" int ral_pool_emit(const float* y, const float* stats, const ral_pool_row* table, int rows, ral_pool_row* table_dev,
                             int upload, int64_t capacity, int leads, int L, int hop, int64_t w0, int nb, int from_last, float* out,
                             int64_t out_total, float* last_y, float* last_stats, ral_stream s) {
  if (!y || !stats || !table || !table_dev || !out) return ral_fail("pool_emit: null pointer");
  int bad = -1;
  const char* why = pool_emit_fault(table, rows, capacity, leads, L, hop, 64, 2048, out_total, upload, w0, nb, from_last, last_y,
                                    last_stats, &bad);
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc)
    k_pool_emit<<<nb * leads, 64, 0, (hipStream_t)s>>>(y, stats, table_dev, rows, leads, L, hop, w0, from_last, out, last_y,
                                                       last_stats);
  return table_done("pool_emit", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)out_total, (long long)w0,
                    nb);
}

// 12-lead pool streams (NewRALELivePool): the bodies of k_newrale_front / k_newrale_back on the pool's table.  The stream
// geometry differs from row to row, so keep() is a placeholder and window() works out the row's own.
struct NrPoolWindows {
  float* hist;             // (2, capacity, 12, L)
  const float* x;          // the packed chunks
  const PoolRow* tab;
  long long cap, w0;
  int rows, L, hop;
  typedef NrLiveWindows::Reader Reader;
  RAL_DEV StreamKeep keep() const { return stream_keep_open(L, hop); }
  RAL_DEV long long window(const StreamKeep&, int i, Reader& src) const {
    const long long gw = w0 + i;
    const PoolRow t = tab[pool_find_row(tab, rows, gw)];
    const StreamKeep sk = pool_keep(t, L, hop);
    const int j = (int)(gw - t.w_off);
    src.o = pool_uniform((int)(stream_start(sk, (int)t.k0 + j, t.T, L, hop) - (t.n0 - L)));
    src.hr = hist + pool_uniform((long long)slot_plane(t.turn, t.slot, cap, NR_LEADS, L));
    src.xr = x + pool_uniform((long long)(t.x_off * NR_LEADS - L));
    src.L = L;
    src.C = pool_uniform(t.c);
    return gw;
  }
  // workgroup g of ng writes the next history of the (row, lead) pairs g, g + ng, ... of the rows that stay open
  RAL_DEV void write_history(int g, int ng) const {
    for (int rc = g; rc < rows * NR_LEADS; rc += ng) {
      const int r = rc / NR_LEADS;
      const PoolRow t = tab[r];
      if (t.flags & RAL_POOL_KEEP) pool_write_history(t, rc - r * NR_LEADS, NR_LEADS, L, cap, hist, x);
    }
  }
};

struct NrPoolKeep {        // into the packed output of a pool call: row t's samples [lo, lo + m) as (12, m) at out_off * 12
  float* out;
  float* last_y;           // (capacity, 2, L) or null
  float* last_stats;       // (capacity, 12, 2) or null (with last_y)
  const PoolRow* tab;
  long long w0;
  int rows, L, hop, from_last;
  RAL_DEV StreamKeep keep() const { return stream_keep_open(L, hop); }
  RAL_DEV NrKept window(const StreamKeep&, int i) const {
    NrKept kp;
    const long long g = w0 + i;
    const PoolRow t = tab[from_last ? (int)g : pool_find_row(tab, rows, g)];
    const StreamKeep sk = pool_keep(t, L, hop);
    const int j = from_last ? 0 : (int)(g - t.w_off), k = (int)t.k0 + j;
    const long long start = stream_start(sk, k, t.T, L, hop);
    long long b, e;
    pool_kept(sk, t, k, start, L, hop, b, e);
    kp.gw = pool_uniform(from_last ? (long long)t.slot : g);    // (from_last: stats are the slots' kept ones)
    kp.ob = pool_uniform((int)(b - start));
    kp.oe = e > b ? pool_uniform((int)(e - start)) : kp.ob;
    kp.dst = pool_uniform((long long)(t.out_off * NR_LEADS + start - t.lo));
    kp.stride = pool_uniform(t.m);
    kp.src = pool_uniform((from_last ? (long long)t.slot : (long long)i) * 2 * L);
    const long long keep_at = last_y && (t.flags & RAL_POOL_KEEP) && j == t.nw - 1 ? (long long)t.slot * 2 * L : -1;
    kp.ly = pool_uniform(keep_at) >= 0 ? last_y + pool_uniform(keep_at) : nullptr;
    return kp;
  }
  RAL_DEV void keep_stats(const NrKept& kp, const float* stats) const {
    if (kp.ly && threadIdx.x < 2 * NR_LEADS)
      last_stats[((kp.ly - last_y) / (2 * L)) * 2 * NR_LEADS + threadIdx.x] = stats[kp.gw * 2 * NR_LEADS + threadIdx.x];
  }
};

extern "C" int ral_newrale_pool_front(float* hist, const float* x, int64_t x_total, const ral_pool_row* table, int rows,
                                      ral_pool_row* table_dev, int upload, int64_t capacity, int L, int hop, int write_hist,
                                      int64_t w0, int nb, const float* adapter_params, float* inner_x, float* stats, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !adapter_params || !inner_x || !stats) return ral_fail("newrale_pool_front: null pointer");
  int bad = -1;
  const char* why = pool_gather_fault(table, rows, capacity, NR_LEADS, L, hop, 16, 1024, x_total, upload, write_hist, w0, nb, &bad);
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc) {
    const long long hrows = (long long)rows * NR_LEADS;
    const int nwg = nb < NR_GRID ? nb : NR_GRID;
    const int nhg = write_hist ? (int)(hrows < NR_GRID ? hrows : NR_GRID) : 0;
    const size_t lds = newrale_front_lds(L);
    RAL_SET_LDS(k_newrale_front<NrPoolWindows>, lds);
    k_newrale_front<<<nwg + nhg, 256, lds, (hipStream_t)s>>>(NrPoolWindows{hist, x, table_dev, capacity, w0, rows, L, hop}, nb, nwg,
                                                             adapter_params, inner_x, stats);
  }
  return table_done("newrale_pool_front", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)x_total,
                    (long long)w0, nb);
}

extern "C" int ral_newrale_pool_back(const float* inner_y, const float* stats, const float* adapter_params, const ral_pool_row* table,
                                     int rows, ral_pool_row* table_dev, int upload, int64_t capacity, int L, int hop, int64_t w0,
                                     int nb, int from_last, float* out, int64_t out_total, float* last_y, float* last_stats,
                                     ral_stream s) {
  if (!inner_y || !stats || !adapter_params || !table || !table_dev || !out) return ral_fail("newrale_pool_back: null pointer");
  int bad = -1;
  const char* why = pool_emit_fault(table, rows, capacity, NR_LEADS, L, hop, 16, 1024, out_total, upload, w0, nb, from_last, last_y,
                                    last_stats, &bad);
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc) {
    const size_t lds = newrale_back_lds(L);
    RAL_SET_LDS(k_newrale_back<NrPoolKeep>, lds);
    k_newrale_back<<<nb < NR_GRID ? nb : NR_GRID, 256, lds, (hipStream_t)s>>>(
        NrPoolKeep{out, last_y, last_stats, table_dev, w0, rows, L, hop, from_last}, nb, inner_y, stats, adapter_params);
  }
  return table_done("newrale_pool_back", rc, why, bad, POOL_ARGS, rows, (long long)capacity, L, hop, (long long)out_total,
                    (long long)w0, nb);
}
