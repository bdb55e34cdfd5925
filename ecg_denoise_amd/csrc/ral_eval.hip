// Noise-stress evaluation of streamed denoising: the two device stages around StreamingDenoiser.denoise --
//   ral_mix_records    the rule of ral_prep_windows (k_prep_stats / k_prep_mix; reference local_utils/local_utils.py:86-130,
//                      261-266) applied to every record of a group (R, leads, T) over its whole length:
//                      clean = per-lead z-score, noisy = clean + sqrt(P_clean / 10^(snr/10) / P_noise) * noise segment
//   ral_score_records  SNR = 10 log10(sum c^2 / sum (c - x)^2) and RMSE = sqrt(mean (c - x)^2) (local_utils/evaluate.py:10-51) of
//                      the denoised (and the noisy) records against the clean ones: per lead, per record, per window tile of
//                      W samples x all leads, and the means over the tiles (denoise_train.py:82-89)
// Both are HBM-bound streaming passes in plain HIP C++.  Every sum is a double; nothing is accumulated with atomics: a pass
// writes one double partial per (record, lead, tile) to caller-owned scratch and its consumer adds a record's partials in a
// fixed order (thread i takes partials i, i + 256, ..., then a shuffle / LDS tree of fixed shape), so the results are the same
// bits run to run.  The scratch is fully written before it is read: no memset.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"

#define EVAL_MAXL 16          // leads per record, as RAL_PREP_MAXL
#define EVAL_THREADS 256
#define EVAL_WAVES (EVAL_THREADS / 64)
#define MIX_TILE 16384        // samples of one (record, lead) per workgroup: 40 tiles for a 650 000-sample record
#define SCORE_PIECE 2048      // samples per lead that one wave scores: whole windows while W <= SCORE_PIECE, else a piece of one
#define SCORE_LG 4            // leads a wave sums side by side (a record with more leads is swept once per group of 4)

// sum of v over the workgroup in a fixed order, returned to every thread (red: EVAL_WAVES doubles; reusable after the call)
static __device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
static __device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = red[0];
#pragma unroll
  for (int w = 1; w < EVAL_WAVES; ++w) t += red[w];
  __syncthreads();
  return t;
}
// the partials p[0, n) added by the workgroup
static __device__ __forceinline__ double block_sum_array(const double* __restrict__ p, long long n, double* red) {
  double v = 0.0;
  for (long long i = threadIdx.x; i < n; i += EVAL_THREADS) v += p[i];
  return block_sum(v, red);
}

// ---------------------------------------------------------------------------------------------------------------------------
// mix.  scratch: offsets[R] (int64), snr_db[R] (double), then three planes of R * leads * ntile doubles: sum x, sum x^2 of the
// record's lead and sum n^2 of the noise segment's lead over one tile
// ---------------------------------------------------------------------------------------------------------------------------
static long long mix_tiles(long long T) { return (T + MIX_TILE - 1) / MIX_TILE; }

__global__ __launch_bounds__(EVAL_THREADS) void k_mix_stats(const float* __restrict__ rec, const float* __restrict__ noise,
                                                            long long T, long long Tn, int leads, long long ntile,
                                                            const long long* __restrict__ offs, double* __restrict__ part,
                                                            long long plane) {
  __shared__ double red[EVAL_WAVES];
  const long long b = blockIdx.x;
  const long long rc = b / ntile, tile = b - rc * ntile;     // rc = record * leads + lead
  const long long r = rc / leads;
  const int c = (int)(rc - r * leads);
  const float* x = rec + (size_t)rc * T;
  const float* n = noise + (size_t)c * Tn + offs[r];
  const long long t1 = min(T, (tile + 1) * MIX_TILE);
  double sx = 0.0, sxx = 0.0, snn = 0.0;
  for (long long t = tile * MIX_TILE + threadIdx.x; t < t1; t += EVAL_THREADS) {
    const double xv = x[t], nv = n[t];
    sx += xv; sxx += xv * xv; snn += nv * nv;
  }
  sx = block_sum(sx, red); sxx = block_sum(sxx, red); snn = block_sum(snn, red);
  if (threadIdx.x == 0) { part[b] = sx; part[plane + b] = sxx; part[2 * plane + b] = snn; }
}

__global__ __launch_bounds__(EVAL_THREADS) void k_mix_apply(const float* __restrict__ rec, const float* __restrict__ noise,
                                                            long long T, long long Tn, int leads, long long ntile,
                                                            const long long* __restrict__ offs, const double* __restrict__ snr_db,
                                                            const double* __restrict__ part, long long plane,
                                                            float* __restrict__ noisy, float* __restrict__ clean) {
  __shared__ double red[EVAL_WAVES];
  const long long b = blockIdx.x;
  const long long rc = b / ntile, tile = b - rc * ntile;
  const long long r = rc / leads;
  const int c = (int)(rc - r * leads);
  // the record's statistics from its partials, every workgroup of the record in the same order
  const double mean = block_sum_array(part + rc * ntile, ntile, red) / (double)T;
  const double var = block_sum_array(part + plane + rc * ntile, ntile, red) / (double)T - mean * mean;
  const double pn = block_sum_array(part + 2 * plane + r * leads * ntile, leads * ntile, red) / (double)T;
  // P_clean = sum(clean^2) / T = leads (every lead has unit population variance), as in k_prep_mix
  const double scale = sqrt((double)leads / pow(10.0, snr_db[r] / 10.0) / pn);
  const double sd = sqrt(var);
  const float* x = rec + (size_t)rc * T;
  const float* n = noise + (size_t)c * Tn + offs[r];
  float* yc = clean + (size_t)rc * T;
  float* yn = noisy + (size_t)rc * T;
  const long long t1 = min(T, (tile + 1) * MIX_TILE);
  for (long long t = tile * MIX_TILE + threadIdx.x; t < t1; t += EVAL_THREADS) {
    const double xn = ((double)x[t] - mean) / sd;
    yc[t] = (float)xn;
    yn[t] = (float)(xn + scale * (double)n[t]);
  }
}

extern "C" int64_t ral_mix_records_scratch_bytes(int64_t R, int leads, int64_t T) {
  if (R < 1 || leads < 1 || leads > EVAL_MAXL || T < 1)
    return ral_fail("mix_records_scratch_bytes: need R >= 1, 1 <= leads <= 16, T >= 1 (R=%lld leads=%d T=%lld)", (long long)R, leads, (long long)T);
  return 8 * (2 * R + 3 * R * leads * mix_tiles(T));
}

// the rule a mix call breaks (*bad: the record that breaks it, or -1), or null
static const char* mix_records_fault(long long R, int leads, long long T, long long Tn, const int64_t* offsets, const double* snr_db,
                                     long long* bad) {
  *bad = -1;
  if (R < 1) return "R >= 1";
  if (leads < 1 || leads > EVAL_MAXL) return "1 <= leads <= 16";
  if (T < 1) return "T >= 1";
  if (Tn < T) return "Tn >= T";
  if (R > 0x7fffffffLL / (leads * mix_tiles(T))) return "at most 2^31 - 1 workgroups";
  for (long long r = 0; r < R; ++r) {
    *bad = r;
    if (offsets[r] < 0 || offsets[r] > Tn - T) return "0 <= offset <= Tn - T";
    if (!isfinite(snr_db[r])) return "a finite snr_db";
  }
  *bad = -1;
  return nullptr;
}

extern "C" int ral_mix_records(const float* rec, const float* noise, int64_t R, int leads, int64_t T, int64_t Tn,
                               const int64_t* offsets, const double* snr_db, void* scratch, float* noisy, float* clean, ral_stream s) {
  if (!rec || !noise || !offsets || !snr_db || !scratch || !noisy || !clean) return ral_fail("mix_records: need no null pointer");
  long long bad = -1;
  if (const char* why = mix_records_fault(R, leads, T, Tn, offsets, snr_db, &bad)) {
    char at[96] = "";
    if (bad >= 0) snprintf(at, sizeof(at), " in record %lld (offset=%lld snr_db=%g)", bad, (long long)offsets[bad], snr_db[bad]);
    return ral_fail("mix_records: need %s%s (R=%lld leads=%d T=%lld Tn=%lld)", why, at, (long long)R, leads, (long long)T, (long long)Tn);
  }
  hipStream_t st = (hipStream_t)s;
  const long long ntile = mix_tiles(T);
  long long* offs = reinterpret_cast<long long*>(scratch);
  double* snr = reinterpret_cast<double*>(scratch) + R;
  double* part = snr + R;
  if (hipMemcpyAsync(offs, offsets, (size_t)R * 8, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync(snr, snr_db, (size_t)R * 8, hipMemcpyHostToDevice, st) != hipSuccess)
    return ral_fail("mix_records: copying offsets / snr_db to the device failed");
  const long long plane = R * leads * ntile;
  k_mix_stats<<<(int)plane, EVAL_THREADS, 0, st>>>(rec, noise, T, Tn, leads, ntile, offs, part, plane);
  k_mix_apply<<<(int)plane, EVAL_THREADS, 0, st>>>(rec, noise, T, Tn, leads, ntile, offs, snr, part, plane, noisy, clean);
  HIP_OK(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// score.  The samples of a record are cut into chunks, one wave each.  While W <= SCORE_PIECE a chunk is floor(SCORE_PIECE / W)
// whole window tiles, 64 at the most (the trailing partial tile belongs to the chunk its first sample falls into) and the wave
// writes the finished per_window rows itself; a longer tile is cut into ceil(W / SCORE_PIECE) equal pieces, one chunk each, and the finish
// kernel adds the pieces of a tile.  Every wave writes the three sums (c^2, (c - out)^2, (c - noisy)^2) of each lead over its
// chunk to scratch: part[((record * leads + lead) * nchunk + chunk) * 3 ..], followed by R rows of 4 doubles (the column sums
// of a record's per_window rows, for the all-tiles mean).
// ---------------------------------------------------------------------------------------------------------------------------
struct ScoreGeom {
  long long nwin, nchunk;
  long long chunk;   // W <= SCORE_PIECE: samples per chunk (a multiple of W); else the piece length
  int mw;            // W <= SCORE_PIECE: tiles per chunk; else 0
  int spw;           // W > SCORE_PIECE: pieces per tile; else 0
};

static __host__ __device__ ScoreGeom score_geom(long long T, long long W) {
  ScoreGeom g;
  g.nwin = T / W;
  if (W <= SCORE_PIECE) {
    g.mw = (int)(SCORE_PIECE / W < 64 ? SCORE_PIECE / W : 64); g.spw = 0;
    g.chunk = g.mw * W;
    g.nchunk = (T + g.chunk - 1) / g.chunk;
  } else {
    g.mw = 0; g.spw = (int)((W + SCORE_PIECE - 1) / SCORE_PIECE);
    g.chunk = (W + g.spw - 1) / g.spw;
    const long long rem = T - g.nwin * W;
    g.nchunk = g.nwin * g.spw + (rem + g.chunk - 1) / g.chunk;
  }
  return g;
}

// (snr_in_db, snr_out_db, rmse_in, rmse_out) from the three sums over n samples.  Plain IEEE: zero error gives +inf dB, a
// zero-power clean signal -inf or NaN, as the reference's torch expressions do
static __device__ __forceinline__ void score_row(double sc, double so, double si, double n, int has_noisy, double* __restrict__ o) {
  const double nan = __longlong_as_double(0x7ff8000000000000LL);
  o[0] = has_noisy ? 10.0 * log10(sc / si) : nan;
  o[1] = 10.0 * log10(sc / so);
  o[2] = has_noisy ? sqrt(si / n) : nan;
  o[3] = sqrt(so / n);
}

// the lanes of a wave over samples [a, b) of leads [c0, c0 + SCORE_LG) of one record: the sums are added to acc (per lead) and
// to win
template <bool NOISY>
static __device__ __forceinline__ void score_span(const float* __restrict__ cl, const float* __restrict__ ou,
                                                  const float* __restrict__ no, long long T, int leads, int c0, long long a,
                                                  long long b, int lane, double (&acc)[SCORE_LG][3], double (&win)[3]) {
#pragma unroll
  for (int i = 0; i < SCORE_LG; ++i) {
    if (c0 + i < leads) {
      const float* cp = cl + (size_t)(c0 + i) * T;
      const float* op = ou + (size_t)(c0 + i) * T;
      const float* np = NOISY ? no + (size_t)(c0 + i) * T : nullptr;
      double s0 = 0.0, s1 = 0.0, s2 = 0.0;
      for (long long t = a + lane; t < b; t += 64) {
        const double cv = cp[t], d = cv - (double)op[t];
        s0 += cv * cv; s1 += d * d;
        if (NOISY) { const double e = cv - (double)np[t]; s2 += e * e; }
      }
      acc[i][0] += s0; acc[i][1] += s1; acc[i][2] += s2;
      win[0] += s0; win[1] += s1; win[2] += s2;
    }
  }
}

template <bool NOISY>
__global__ __launch_bounds__(EVAL_THREADS) void k_score_chunks(const float* __restrict__ clean, const float* __restrict__ out,
                                                               const float* __restrict__ noisy, long long T, int leads,
                                                               long long W, long long bpr /* workgroups per record */,
                                                               double* __restrict__ part, double* __restrict__ per_window) {
  const ScoreGeom g = score_geom(T, W);
  const long long r = blockIdx.x / bpr;
  const long long ch = (blockIdx.x - r * bpr) * EVAL_WAVES + (threadIdx.x >> 6);
  if (ch >= g.nchunk) return;
  const int lane = threadIdx.x & 63;
  const float* cl = clean + (size_t)r * leads * T;
  const float* ou = out + (size_t)r * leads * T;
  const float* no = NOISY ? noisy + (size_t)r * leads * T : nullptr;
  // the spans of this chunk: nw whole tiles from w0 on (W <= SCORE_PIECE; tile i is summed over the leads in lane i), then
  // samples [ra, rb) that count for the leads only (the trailing partial tile, or a piece of a long tile)
  long long w0 = 0, ra, rb;
  int nw = 0;
  if (g.mw) {
    w0 = ch * g.mw;
    nw = (int)(min(g.nwin, w0 + g.mw) - w0);
    if (nw < 0) nw = 0;
    ra = max(ch * g.chunk, g.nwin * W); rb = min(T, (ch + 1) * g.chunk);
  } else if (ch < g.nwin * g.spw) {
    const long long w = ch / g.spw, p = ch - w * g.spw;
    ra = w * W + p * g.chunk; rb = min(w * W + (p + 1) * g.chunk, (w + 1) * W);
  } else {
    ra = g.nwin * W + (ch - g.nwin * g.spw) * g.chunk; rb = min(T, ra + g.chunk);
  }
  double wt0 = 0.0, wt1 = 0.0, wt2 = 0.0;      // lane i: the sums of tile w0 + i over the lead groups so far
  for (int c0 = 0; c0 < leads; c0 += SCORE_LG) {
    double acc[SCORE_LG][3];
#pragma unroll
    for (int i = 0; i < SCORE_LG; ++i) { acc[i][0] = 0.0; acc[i][1] = 0.0; acc[i][2] = 0.0; }
    for (int i = 0; i < nw; ++i) {
      double win[3] = {0.0, 0.0, 0.0};
      score_span<NOISY>(cl, ou, no, T, leads, c0, (w0 + i) * W, (w0 + i + 1) * W, lane, acc, win);
      const double sc = wave_sum(win[0]), so = wave_sum(win[1]), si = NOISY ? wave_sum(win[2]) : 0.0;
      if (lane == i) { wt0 += sc; wt1 += so; wt2 += si; }
    }
    double skip[3] = {0.0, 0.0, 0.0};
    if (ra < rb) score_span<NOISY>(cl, ou, no, T, leads, c0, ra, rb, lane, acc, skip);
#pragma unroll
    for (int i = 0; i < SCORE_LG; ++i) {
      if (c0 + i < leads) {
        const double s0 = wave_sum(acc[i][0]), s1 = wave_sum(acc[i][1]), s2 = NOISY ? wave_sum(acc[i][2]) : 0.0;
        if (lane == 0) {
          double* p = part + (((size_t)r * leads + c0 + i) * g.nchunk + ch) * 3;
          p[0] = s0; p[1] = s1; p[2] = s2;
        }
      }
    }
  }
  if (lane < nw) score_row(wt0, wt1, wt2, (double)W * leads, NOISY, per_window + (r * g.nwin + w0 + lane) * 4);
}

// one workgroup per record: per_lead, per_record, the per_window rows of tiles longer than a piece, window_mean[record] and
// the record's column sums
__global__ __launch_bounds__(EVAL_THREADS) void k_score_finish(long long T, int leads, long long W, int has_noisy,
                                                               const double* __restrict__ part, double* __restrict__ rsum,
                                                               double* __restrict__ per_lead, double* __restrict__ per_record,
                                                               double* __restrict__ per_window, double* __restrict__ window_mean) {
  __shared__ double red[EVAL_WAVES];
  const ScoreGeom g = score_geom(T, W);
  const long long r = blockIdx.x;
  double rec[3] = {0.0, 0.0, 0.0};
  for (int c = 0; c < leads; ++c) {
    const double* p = part + ((size_t)r * leads + c) * g.nchunk * 3;
    double s[3];
    for (int k = 0; k < 3; ++k) {
      double v = 0.0;
      for (long long i = threadIdx.x; i < g.nchunk; i += EVAL_THREADS) v += p[i * 3 + k];
      s[k] = block_sum(v, red);
      rec[k] += s[k];
    }
    if (threadIdx.x == 0) score_row(s[0], s[1], s[2], (double)T, has_noisy, per_lead + (r * leads + c) * 4);
  }
  if (threadIdx.x == 0) score_row(rec[0], rec[1], rec[2], (double)T * leads, has_noisy, per_record + r * 4);
  if (g.spw) {
    for (long long w = threadIdx.x; w < g.nwin; w += EVAL_THREADS) {
      double s[3] = {0.0, 0.0, 0.0};
      for (int c = 0; c < leads; ++c) {
        const double* p = part + (((size_t)r * leads + c) * g.nchunk + w * g.spw) * 3;
        for (int q = 0; q < g.spw; ++q) { s[0] += p[q * 3]; s[1] += p[q * 3 + 1]; s[2] += p[q * 3 + 2]; }
      }
      score_row(s[0], s[1], s[2], (double)W * leads, has_noisy, per_window + (r * g.nwin + w) * 4);
    }
    __syncthreads();      // the rows above are read back below, each by the thread that wrote it
  }
  for (int k = 0; k < 4; ++k) {
    double v = 0.0;
    for (long long w = threadIdx.x; w < g.nwin; w += EVAL_THREADS) v += per_window[(r * g.nwin + w) * 4 + k];
    v = block_sum(v, red);
    if (threadIdx.x == 0) { rsum[r * 4 + k] = v; window_mean[r * 4 + k] = v / (double)g.nwin; }
  }
}

// the all-tiles row: the records' column sums in record order
__global__ void k_score_total(long long R, long long nwin, const double* __restrict__ rsum, double* __restrict__ window_mean) {
  const int k = threadIdx.x;
  if (k >= 4) return;
  double v = 0.0;
  for (long long r = 0; r < R; ++r) v += rsum[r * 4 + k];
  window_mean[R * 4 + k] = v / ((double)R * (double)nwin);
}

extern "C" int64_t ral_score_records_scratch_bytes(int64_t R, int leads, int64_t T, int64_t W) {
  if (R < 1 || leads < 1 || leads > EVAL_MAXL || T < 1 || W < 1 || W > T)
    return ral_fail("score_records_scratch_bytes: need R >= 1, 1 <= leads <= 16, T >= 1, 1 <= W <= T (R=%lld leads=%d T=%lld W=%lld)",
                (long long)R, leads, (long long)T, (long long)W);
  return 8 * (3 * R * leads * score_geom(T, W).nchunk + 4 * R);
}

// the rule a score call breaks, or null (bpr: workgroups per record)
static const char* score_records_fault(long long R, int leads, long long T, long long W, long long* bpr) {
  if (R < 1) return "R >= 1";
  if (leads < 1 || leads > EVAL_MAXL) return "1 <= leads <= 16";
  if (T < 1) return "T >= 1";
  if (W < 1 || W > T) return "1 <= W <= T";
  *bpr = (score_geom(T, W).nchunk + EVAL_WAVES - 1) / EVAL_WAVES;
  return R > 0x7fffffffLL / *bpr ? "at most 2^31 - 1 workgroups" : nullptr;
}

extern "C" int ral_score_records(const float* clean, const float* out, const float* noisy, int64_t R, int leads, int64_t T, int64_t W,
                                 void* scratch, double* per_lead, double* per_record, double* per_window, double* window_mean,
                                 ral_stream s) {
  if (!clean || !out || !scratch || !per_lead || !per_record || !per_window || !window_mean)
    return ral_fail("score_records: need no null pointer (only noisy may be null)");
  long long bpr = 0;
  if (const char* why = score_records_fault(R, leads, T, W, &bpr))
    return ral_fail("score_records: need %s (R=%lld leads=%d T=%lld W=%lld)", why, (long long)R, leads, (long long)T, (long long)W);
  hipStream_t st = (hipStream_t)s;
  const ScoreGeom g = score_geom(T, W);
  double* part = reinterpret_cast<double*>(scratch);
  double* rsum = part + 3 * R * leads * g.nchunk;
  if (noisy) k_score_chunks<true><<<(int)(R * bpr), EVAL_THREADS, 0, st>>>(clean, out, noisy, T, leads, W, bpr, part, per_window);
  else k_score_chunks<false><<<(int)(R * bpr), EVAL_THREADS, 0, st>>>(clean, out, noisy, T, leads, W, bpr, part, per_window);
  k_score_finish<<<(int)R, EVAL_THREADS, 0, st>>>(T, leads, W, noisy != nullptr, part, rsum, per_lead, per_record, per_window,
                                                  window_mean);
  k_score_total<<<1, 64, 0, st>>>(R, g.nwin, rsum, window_mean);
  HIP_OK(hipGetLastError());
  return 0;
}
