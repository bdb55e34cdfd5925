// R-peak detection in records and live streams (ral_beat_records / ral_beat_pool / ral_beat_match; host side: beats.py).
//
// The detector (include/ralenet.h has the definition): a band-pass bank h of 2 half + 1 taps on every lead, the squared outputs
// summed over the leads (f), a moving mean of 2 Wi + 1 terms (m), a threshold alpha * (max of m within +-Wt), a refractory rule
// within +-Rf and a refinement to the top of f within +-Rw.  Every value is formed on its own, in a fixed order, so a value does
// not depend on which workgroup, tile or call forms it: a stream analysed push by push gives the integers of the whole record.
//
// A row is a record of N samples of which the decisions [d0, d1) are wanted.  For a whole record N = T, d0 = 0, d1 = T; for a
// pool row N = n0 + c (what the stream has received), the decisions are those the push finalises, and samples older than the
// history are never needed for them.  Per row
//   m is needed on [mlo, mhi) = [d0 - Wt, d1 + Wt) and f on [flo, fhi) = [mlo - Wi, mhi + Wi), both clipped to [0, N);
//   f and m live in the caller's scratch at index i - flo.
// Three launches:
//   feature  a workgroup forms fn = tile + 2 Wi values of f (4 consecutive ones per thread) from the staged span of all leads,
//            keeps them in LDS, and writes f and m of its tile.  The taps are padded with zeros to a multiple of 4 (nt4), so
//            that per 4 taps a thread reads one float4 of samples and one of taps for its 16 fmaf; word w of a lead's span
//            holds sample fa + half - nt4 + w (clamped), fa = the tile's first index - Wi.
//   pick     a workgroup stages m of its 1024 decisions with a Wt halo, forms the sliding maximum by doubling (max over
//            [w, w + 2^k) in k steps; a window of 2 Wt + 1 is two overlapping spans of the largest power of two below it),
//            applies the rules, refines in f, and writes its peaks in order (a scan over the threads' counts) and their number.
//   gather   one workgroup per row scans the tile counts and copies the tiles' peaks in order; no atomic anywhere.
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_slots.hpp"
#include <math.h>
#include <stdint.h>
#include <stdio.h>

namespace {

constexpr int BEAT_THREADS = 256;
constexpr int BEAT_FN_MAX = 1024;         // values of f per feature workgroup, halved while the spans of all leads do not fit
constexpr int BEAT_FN_MIN = 128;
constexpr int BEAT_PICK = 1024;           // decisions per pick workgroup: 4 consecutive ones per thread
constexpr int BEAT_LDS_FLOATS = 16384;    // the budget: 64 KB, what a kernel gets without opting into more

struct BeatGeom {
  int leads, half, wi, wt, rf, rw, ntaps;
  float alpha, floor;
  int nt4, fn, tile, xs, tc;      // padded taps; f values and outputs per feature workgroup; words of a lead's span; peaks a pick tile can hold
};

struct BeatRow {
  const float* chunk;      // lead l: samples n0 .. N - 1 at chunk + l * chunk_stride
  const float* hist;       // lead l: samples n0 - hist_len .. n0 - 1 at hist + l * hist_len (null for a record: n0 = 0)
  long long chunk_stride, n0, N, d0, d1, flo, fhi, mlo, mhi;
  float *f, *m;            // index i - flo
  int hist_len;
};

RAL_DEV void beat_spans(BeatRow& rw, const BeatGeom& g) {
  const long long a = rw.d0 - g.wt, b = rw.d1 + g.wt;
  rw.mlo = a < 0 ? 0 : a;
  rw.mhi = b > rw.N ? rw.N : b;
  const long long c = rw.mlo - g.wi, d = rw.mhi + g.wi;
  rw.flo = c < 0 ? 0 : c;
  rw.fhi = d > rw.N ? rw.N : d;
}

// f and m on [a, a + cnt), cnt <= g.tile.  hl: nt4 floats, xs: leads * g.xs, fl: g.fn; each 16-byte aligned
RAL_DEV void beat_feature_tile(const BeatRow& rw, long long a, int cnt, const BeatGeom& g, const float* __restrict__ bank, float* hl,
                               float* xs, float* fl) {
  const int tid = threadIdx.x;
  for (int e = tid; e < g.nt4; e += BEAT_THREADS) hl[e] = e < g.ntaps ? bank[e] : 0.f;
  const long long fa = a - g.wi;
  const long long xb = fa + g.half - g.nt4;
  for (int lead = 0; lead < g.leads; ++lead)      // (older than the history only for values that are discarded: halo and padded taps)
    for (int w = tid; w < g.xs; w += BEAT_THREADS)
      xs[lead * g.xs + w] = slot_sample(rw.chunk, rw.chunk_stride, rw.hist, rw.hist_len, rw.n0, rw.N, lead, xb + w);
  __syncthreads();

  const int q4 = g.nt4 >> 2;
  const float4* hq = reinterpret_cast<const float4*>(hl);
  for (int u = tid; u < (g.fn >> 2); u += BEAT_THREADS) {
    float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f;
    for (int lead = 0; lead < g.leads; ++lead) {
      // output o of this thread, tap i = 4 gq + e: word 4 (u + q4 - gq) + o - e, in `hi` (o >= e) or in the quad below it
      const float4* xq = reinterpret_cast<const float4*>(xs + lead * g.xs) + u + q4;
      float4 hi = xq[0];
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 2
      for (int gq = 0; gq < q4; ++gq) {
        const float4 lo = xq[-gq - 1];
        const float4 hv = hq[gq];
        a0 = fmaf(hv.x, hi.x, a0); a1 = fmaf(hv.x, hi.y, a1); a2 = fmaf(hv.x, hi.z, a2); a3 = fmaf(hv.x, hi.w, a3);
        a0 = fmaf(hv.y, lo.w, a0); a1 = fmaf(hv.y, hi.x, a1); a2 = fmaf(hv.y, hi.y, a2); a3 = fmaf(hv.y, hi.z, a3);
        a0 = fmaf(hv.z, lo.z, a0); a1 = fmaf(hv.z, lo.w, a1); a2 = fmaf(hv.z, hi.x, a2); a3 = fmaf(hv.z, hi.y, a3);
        a0 = fmaf(hv.w, lo.y, a0); a1 = fmaf(hv.w, lo.z, a1); a2 = fmaf(hv.w, lo.w, a2); a3 = fmaf(hv.w, hi.x, a3);
        hi = lo;
      }
      f0 = fmaf(a0, a0, f0); f1 = fmaf(a1, a1, f1); f2 = fmaf(a2, a2, f2); f3 = fmaf(a3, a3, f3);
    }
    const long long i0 = fa + 4 * u;        // f is 0 outside the record; outside the row's span it is not needed
    float4 v;
    v.x = i0 >= rw.flo && i0 < rw.fhi ? f0 : 0.f;
    v.y = i0 + 1 >= rw.flo && i0 + 1 < rw.fhi ? f1 : 0.f;
    v.z = i0 + 2 >= rw.flo && i0 + 2 < rw.fhi ? f2 : 0.f;
    v.w = i0 + 3 >= rw.flo && i0 + 3 < rw.fhi ? f3 : 0.f;
    reinterpret_cast<float4*>(fl)[u] = v;
  }
  __syncthreads();

  const int nw = 2 * g.wi + 1;
  const float div = (float)nw;
  for (int j = tid; j < cnt; j += BEAT_THREADS) {
    float s = 0.f;
    for (int jj = 0; jj < nw; ++jj) s += fl[j + jj];
    const long long i = a + j;
    rw.f[i - rw.flo] = fl[j + g.wi];
    if (i >= rw.mlo && i < rw.mhi) rw.m[i - rw.flo] = s / div;
  }
}

// decisions [t0, t0 + cnt), cnt <= BEAT_PICK.  M, A, B: BEAT_PICK + 2 Wt floats each; scan: BEAT_THREADS ints.
// The tile's peaks go to tpk[0 .. *tcnt) in ascending order.
RAL_DEV void beat_pick_tile(const BeatRow& rw, long long t0, int cnt, const BeatGeom& g, float* M, float* A, float* B, int* scan,
                            long long* tpk, int* tcnt) {
  const int tid = threadIdx.x;
  const int n = cnt + 2 * g.wt;
  const long long base = t0 - g.wt;
  for (int w = tid; w < n; w += BEAT_THREADS) {       // (-1: below every m; what lies outside [mlo, mhi) here lies outside the record)
    const long long i = base + w;
    const float v = i >= rw.mlo && i < rw.mhi ? rw.m[i - rw.flo] : -1.f;
    M[w] = v;
    A[w] = v;
  }
  __syncthreads();
  const int win = 2 * g.wt + 1;
  float *src = A, *dst = B;
  int span = 1;
  while (2 * span <= win) {
    for (int w = tid; w < n; w += BEAT_THREADS) dst[w] = fmaxf(src[w], w + span < n ? src[w + span] : -1.f);
    __syncthreads();
    float* t = src; src = dst; dst = t;
    span *= 2;
  }

  long long pk[4];
  int c = 0;
  for (int o = 0; o < 4; ++o) {
    const int j = 4 * tid + o;
    if (j >= cnt) break;
    const float mv = M[j + g.wt];
    if (!(mv > 0.f)) continue;
    const float thr = fmaxf(g.alpha * fmaxf(src[j], src[j + win - span]), g.floor);
    if (!(mv >= thr)) continue;
    bool ok = true;
    for (int r = 1; r <= g.rf && ok; ++r) ok = mv > M[j + g.wt - r] && mv >= M[j + g.wt + r];
    if (!ok) continue;
    const long long nn = t0 + j;
    const long long lo = nn - g.rw < 0 ? 0 : nn - g.rw, hi = nn + g.rw > rw.N - 1 ? rw.N - 1 : nn + g.rw;
    long long best = lo;
    float bv = rw.f[lo - rw.flo];
    for (long long i = lo + 1; i <= hi; ++i) {
      const float v = rw.f[i - rw.flo];
      if (v > bv) bv = v, best = i;
    }
    pk[c++] = best;
  }
  scan[tid] = c;
  __syncthreads();
  for (int off = 1; off < BEAT_THREADS; off <<= 1) {
    const int v = tid >= off ? scan[tid - off] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  const int first = scan[tid] - c;
  for (int i = 0; i < c; ++i)
    if (first + i < g.tc) tpk[first + i] = pk[i];     // (candidates lie more than Rf apart: a tile never has more than tc)
  if (tid == BEAT_THREADS - 1) *tcnt = scan[tid] < g.tc ? scan[tid] : g.tc;
}

// the peaks of a row's tiles, in tile order -> out[0 .. cap), padded with -1; *count = their number
template <typename OutT>
RAL_DEV void beat_gather_row(const int* tcnt, const long long* tpk, long long ntile, int tc, OutT* out, long long cap, int* count,
                             int* scan) {
  const int tid = threadIdx.x;
  long long total = 0;
  for (long long b0 = 0; b0 < ntile; b0 += BEAT_THREADS) {
    const long long t = b0 + tid;
    const int c = t < ntile ? tcnt[t] : 0;
    scan[tid] = c;
    __syncthreads();
    for (int off = 1; off < BEAT_THREADS; off <<= 1) {
      const int v = tid >= off ? scan[tid - off] : 0;
      __syncthreads();
      scan[tid] += v;
      __syncthreads();
    }
    const long long first = total + scan[tid] - c;
    for (int i = 0; i < c; ++i)
      if (first + i < cap) out[first + i] = (OutT)tpk[t * tc + i];
    total += scan[BEAT_THREADS - 1];
    __syncthreads();
  }
  if (total > cap) total = cap;
  for (long long i = total + tid; i < cap; i += BEAT_THREADS) out[i] = (OutT)-1;
  if (tid == 0) *count = (int)total;
}

RAL_DEV void beat_feature_lds(const BeatGeom& g, float* base, float*& hl, float*& xs, float*& fl) {
  hl = base;
  xs = hl + g.nt4;
  fl = xs + g.leads * g.xs;
}

RAL_DEV void beat_pick_lds(const BeatGeom& g, float* base, float*& M, float*& A, float*& B, int*& scan) {
  const int n = BEAT_PICK + 2 * g.wt;
  M = base;
  A = M + n;
  B = A + n;
  scan = reinterpret_cast<int*>(B + n);
}

// where a row's values lie in the scratch: S floats of f and of m per row, NT tile counts and NT * tc tile peaks
struct BeatScratch {
  float *f, *m;
  int* tcnt;
  long long* tpk;
  long long S, NT;
};

RAL_DEV BeatRow beat_record_row(const float* x, long long row, long long T, const BeatGeom& g, const BeatScratch& sc) {
  BeatRow rw;
  rw.chunk = x + row * g.leads * T;
  rw.hist = nullptr;
  rw.chunk_stride = T, rw.n0 = 0, rw.N = T, rw.d0 = 0, rw.d1 = T, rw.hist_len = 0;
  rw.f = sc.f + row * sc.S, rw.m = sc.m + row * sc.S;
  beat_spans(rw, g);
  return rw;
}

typedef ral_beat_row BeatPoolRow;

RAL_DEV BeatRow beat_pool_row(const float* hist, const float* x, const BeatPoolRow& t, long long row, long long cap, int hist_len,
                              const BeatGeom& g, const BeatScratch& sc) {
  BeatRow rw;
  rw.chunk = x + t.x_off * g.leads;
  rw.hist = hist + slot_plane(t.turn, t.slot, cap, g.leads, hist_len);
  rw.chunk_stride = t.c, rw.n0 = t.n0, rw.N = t.n0 + t.c, rw.d0 = t.d0, rw.d1 = t.d0 + t.d, rw.hist_len = hist_len;
  rw.f = sc.f + row * sc.S, rw.m = sc.m + row * sc.S;
  beat_spans(rw, g);
  return rw;
}

// grid (feature tiles of a record, R)
__global__ __launch_bounds__(BEAT_THREADS) void k_beat_feature_records(const float* __restrict__ x, long long T, BeatGeom g,
                                                                       const float* __restrict__ bank, BeatScratch sc) {
  extern __shared__ __attribute__((aligned(16))) float beat_smem[];
  float *hl, *xs, *fl;
  beat_feature_lds(g, beat_smem, hl, xs, fl);
  const BeatRow rw = beat_record_row(x, blockIdx.y, T, g, sc);
  const long long a = (long long)blockIdx.x * g.tile, left = T - a;
  beat_feature_tile(rw, a, (int)(left < g.tile ? left : g.tile), g, bank, hl, xs, fl);
}

// grid (pick tiles of a record, R)
__global__ __launch_bounds__(BEAT_THREADS) void k_beat_pick_records(const float* __restrict__ x, long long T, BeatGeom g,
                                                                    BeatScratch sc) {
  extern __shared__ __attribute__((aligned(16))) float beat_smem[];
  float *M, *A, *B;
  int* scan;
  beat_pick_lds(g, beat_smem, M, A, B, scan);
  const BeatRow rw = beat_record_row(x, blockIdx.y, T, g, sc);
  const long long t0 = (long long)blockIdx.x * BEAT_PICK, left = T - t0, tl = blockIdx.y * sc.NT + blockIdx.x;
  beat_pick_tile(rw, t0, (int)(left < BEAT_PICK ? left : BEAT_PICK), g, M, A, B, scan, sc.tpk + tl * g.tc, sc.tcnt + tl);
}

// grid (R)
__global__ __launch_bounds__(BEAT_THREADS) void k_beat_gather_records(long long T, BeatGeom g, BeatScratch sc, int* __restrict__ peaks,
                                                                      long long cap, int* __restrict__ count) {
  __shared__ int scan[BEAT_THREADS];
  const long long row = blockIdx.x, ntile = (T + BEAT_PICK - 1) / BEAT_PICK;
  beat_gather_row<int>(sc.tcnt + row * sc.NT, sc.tpk + row * sc.NT * g.tc, ntile, g.tc, peaks + row * cap, cap, count + row, scan);
}

// grid (feature tiles of the longest row + 1, rows): the last x index writes the next history of its row
__global__ __launch_bounds__(BEAT_THREADS) void k_beat_feature_pool(float* hist, const float* __restrict__ x,
                                                                    const BeatPoolRow* __restrict__ tab, long long cap, int hist_len,
                                                                    BeatGeom g, const float* __restrict__ bank, BeatScratch sc) {
  extern __shared__ __attribute__((aligned(16))) float beat_smem[];
  const BeatPoolRow t = tab[blockIdx.y];
  const BeatRow rw = beat_pool_row(hist, x, t, blockIdx.y, cap, hist_len, g, sc);
  if (blockIdx.x == gridDim.x - 1) {
    if (!(t.flags & RAL_POOL_KEEP)) return;
    for (int lead = 0; lead < g.leads; ++lead)
      slot_write_history(rw.hist + (size_t)lead * hist_len, rw.chunk + lead * rw.chunk_stride,
                         hist + slot_plane(1 - t.turn, t.slot, cap, g.leads, hist_len, lead), t.n0, t.c, hist_len);
    return;
  }
  const long long a = rw.flo + (long long)blockIdx.x * g.tile;
  if (t.d == 0 || a >= rw.fhi) return;
  float *hl, *xs, *fl;
  beat_feature_lds(g, beat_smem, hl, xs, fl);
  const long long left = rw.fhi - a;
  beat_feature_tile(rw, a, (int)(left < g.tile ? left : g.tile), g, bank, hl, xs, fl);
}

// grid (pick tiles of the row with the most decisions, rows)
__global__ __launch_bounds__(BEAT_THREADS) void k_beat_pick_pool(const float* hist, const float* __restrict__ x,
                                                                 const BeatPoolRow* __restrict__ tab, long long cap, int hist_len,
                                                                 BeatGeom g, BeatScratch sc) {
  extern __shared__ __attribute__((aligned(16))) float beat_smem[];
  const BeatPoolRow t = tab[blockIdx.y];
  const long long j0 = (long long)blockIdx.x * BEAT_PICK;
  if (j0 >= t.d) return;
  float *M, *A, *B;
  int* scan;
  beat_pick_lds(g, beat_smem, M, A, B, scan);
  const BeatRow rw = beat_pool_row(hist, x, t, blockIdx.y, cap, hist_len, g, sc);
  const long long left = t.d - j0, tl = blockIdx.y * sc.NT + blockIdx.x;
  beat_pick_tile(rw, t.d0 + j0, (int)(left < BEAT_PICK ? left : BEAT_PICK), g, M, A, B, scan, sc.tpk + tl * g.tc, sc.tcnt + tl);
}

// grid (rows)
__global__ __launch_bounds__(BEAT_THREADS) void k_beat_gather_pool(const BeatPoolRow* __restrict__ tab, BeatGeom g, BeatScratch sc,
                                                                   long long* __restrict__ peaks, int* __restrict__ count) {
  __shared__ int scan[BEAT_THREADS];
  const long long row = blockIdx.x;
  const BeatPoolRow t = tab[row];
  const long long ntile = ((long long)t.d + BEAT_PICK - 1) / BEAT_PICK;
  beat_gather_row<long long>(sc.tcnt + row * sc.NT, sc.tpk + row * sc.NT * g.tc, ntile, g.tc, peaks + t.out_off, t.cap, count + row,
                             scan);
}

// one lane per record walks its two sorted lists
__global__ __launch_bounds__(64) void k_beat_match(const int* __restrict__ ref, const int* __restrict__ nref, long long ref_cap,
                                                   const int* __restrict__ det, const int* __restrict__ ndet, long long det_cap,
                                                   long long R, long long tol, long long* __restrict__ out) {
  const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
  if (r >= R) return;
  const int* a = ref + r * ref_cap;
  const int* b = det + r * det_cap;
  long long na = nref[r], nb = ndet[r];
  na = na < 0 ? 0 : (na > ref_cap ? ref_cap : na);
  nb = nb < 0 ? 0 : (nb > det_cap ? det_cap : nb);
  long long i = 0, j = 0, tp = 0, fp = 0, fn = 0;
  while (i < na && j < nb) {
    const long long d = (long long)b[j] - a[i];
    if ((d < 0 ? -d : d) <= tol) ++tp, ++i, ++j;
    else if (d < 0) ++fp, ++j;
    else ++fn, ++i;
  }
  out[3 * r] = tp, out[3 * r + 1] = fp + (nb - j), out[3 * r + 2] = fn + (na - i);
}

// ------------------------------------------------------------------------------------------------ host
const char* beat_geom(int leads, const ral_beat_geom* p, int ntaps, BeatGeom& g) {
  if (!p) return "a geometry";
  if (leads < 1) return "leads >= 1";
  if (p->half < 1 || p->half > 8192) return "1 <= half <= 8192";
  if (ntaps != 2 * p->half + 1) return "ntaps = 2 half + 1";
  if (p->wi < 0 || p->wt < 1 || p->rf < 1 || p->rw < 0) return "Wi >= 0, Wt >= 1, Rf >= 1, Rw >= 0";
  if (p->rf > p->wt || p->rw > p->wt + p->wi || 2 * p->rw > p->rf) return "Rf <= Wt, Rw <= Wt + Wi and 2 Rw <= Rf";
  if (!(p->alpha > 0.f) || !isfinite(p->alpha) || !(p->floor >= 0.f) || !isfinite(p->floor)) return "alpha > 0 and floor >= 0, finite";
  g.leads = leads, g.half = p->half, g.wi = p->wi, g.wt = p->wt, g.rf = p->rf, g.rw = p->rw, g.ntaps = ntaps;
  g.alpha = p->alpha, g.floor = p->floor;
  g.nt4 = (ntaps + 3) & ~3;
  g.tc = (BEAT_PICK - 1) / (g.rf + 1) + 1;
  if (3LL * (BEAT_PICK + 2LL * g.wt) + BEAT_THREADS > BEAT_LDS_FLOATS) return "a threshold window (2 Wt + 1) that fits 64 KB of LDS three times";
  for (g.fn = BEAT_FN_MAX; g.fn >= BEAT_FN_MIN; g.fn >>= 1) {
    g.xs = g.fn + g.nt4, g.tile = g.fn - 2 * g.wi;
    if ((long long)leads * g.xs + g.nt4 + g.fn <= BEAT_LDS_FLOATS && 2 * g.tile >= g.fn) return nullptr;
  }
  return "a bank and a tile's input span of all leads that fit 64 KB of LDS";
}

size_t beat_feature_lds_bytes(const BeatGeom& g) { return ((size_t)g.leads * g.xs + g.nt4 + g.fn) * sizeof(float); }
size_t beat_pick_lds_bytes(const BeatGeom& g) { return (3 * (size_t)(BEAT_PICK + 2 * g.wt) + BEAT_THREADS) * sizeof(float); }

// the scratch of `rows` rows of at most S values of f each -> bytes; sc (if given) is laid out over `base`
long long beat_scratch(long long rows, long long S, const BeatGeom& g, void* base, BeatScratch* sc) {
  const long long NT = (S + BEAT_PICK - 1) / BEAT_PICK;
  const long long fl = (rows * S * 4 + 7) & ~7LL, cn = (rows * NT * 4 + 7) & ~7LL;
  if (sc) {
    char* b = (char*)base;
    sc->f = (float*)b, sc->m = (float*)(b + fl), sc->tcnt = (int*)(b + 2 * fl), sc->tpk = (long long*)(b + 2 * fl + cn);
    sc->S = S, sc->NT = NT;
  }
  return 2 * fl + cn + rows * NT * g.tc * 8;
}

const char* beat_pool_fault(const BeatPoolRow* tab, int rows, long long cap, const BeatGeom& g, int hist_len, long long x_total,
                            long long peaks_total, bool walk, int* bad) {
  *bad = -1;
  if (rows < 1 || rows > 65535) return "1 <= rows <= 65535";
  if (cap < 1) return "capacity >= 1";
  const long long lat = (long long)g.wt + g.wi + g.half;
  if (hist_len < 2 * lat) return "hist_len >= 2 (Wt + Wi + half)";
  if (x_total < 0 || peaks_total < 0) return "x_total, peaks_total >= 0";
  if (!walk) return nullptr;
  const long long big = 1LL << 40;
  const SlotRules rules{1, false, "0 <= n0, d0 <= 2^40, 0 <= c < 2^30, d >= 0 and cap >= 0",
                        "T = n0 + c >= 1 without RAL_POOL_KEEP, or T = -1 with RAL_POOL_KEEP"};
  auto in_range = [&](const BeatPoolRow& t) {
    return !(t.n0 < 0 || t.n0 > big || t.d0 < 0 || t.d0 > big || t.c < 0 || t.c > 0x3fffffff || t.d < 0 || t.cap < 0);
  };
  auto own = [&](const BeatPoolRow& t) -> const char* {
    if (t.out_off < 0 || t.out_off + t.cap > peaks_total) return "the row's peaks inside the packed peaks";
    if (t.d == 0) return nullptr;
    const long long n1 = t.n0 + t.c;
    if (t.T < 0 ? t.d0 + t.d + lat > n1 : t.d0 + t.d > n1)
      return "decisions that are final: d0 + d + Wt + Wi + half <= n0 + c, or d0 + d <= T at the end";
    if (t.cap < ((long long)t.d - 1) / (g.rf + 1) + 1) return "cap >= ceil(d / (Rf + 1))";
    long long oldest = t.d0 - lat;
    if (oldest < 0) oldest = 0;
    if (oldest < t.n0 - hist_len) return "the oldest sample of decision d0 inside the history";
    return nullptr;
  };
  return slots_walk(tab, rows, cap, x_total, rules, in_range, SlotNoRule{}, own, bad);
}

// S of a pool call: the longest span of f over its rows (at least 1)
long long beat_pool_span(const BeatPoolRow* tab, int rows, const BeatGeom& g) {
  long long S = 1;
  for (int r = 0; r < rows; ++r) {
    const BeatPoolRow& t = tab[r];
    if (t.d == 0) continue;
    const long long N = t.n0 + t.c;
    long long lo = t.d0 - g.wt - g.wi, hi = t.d0 + t.d + g.wt + g.wi;
    lo = lo < 0 ? 0 : lo, hi = hi > N ? N : hi;
    S = hi - lo > S ? hi - lo : S;
  }
  return S;
}

}  // namespace

// the caller's geometry as the refusals print it
static void beat_geom_text(const ral_beat_geom* g, char* buf, size_t n) {
  if (g) snprintf(buf, n, "half=%d Wi=%d Wt=%d Rf=%d Rw=%d alpha=%g floor=%g", g->half, g->wi, g->wt, g->rf, g->rw, g->alpha, g->floor);
  else snprintf(buf, n, "no geometry");
}

extern "C" int64_t ral_beat_records_scratch_bytes(int64_t R, int leads, int64_t T, const ral_beat_geom* geom) {
  BeatGeom g;
  const char* why = beat_geom(leads, geom, geom ? 2 * geom->half + 1 : 0, g);
  if (!why && (R < 1 || R > 65535 || T < 1 || T > 0x7fffffffLL)) why = "1 <= R <= 65535 and 1 <= T < 2^31";
  if (why) {
    char gt[160];
    beat_geom_text(geom, gt, sizeof(gt));
    return ral_fail("beat_records_scratch_bytes: need %s (R=%lld leads=%d T=%lld %s)", why, (long long)R, leads, (long long)T, gt);
  }
  return beat_scratch(R, T, g, nullptr, nullptr);
}

extern "C" int ral_beat_records(const float* x, int64_t R, int leads, int64_t T, const ral_beat_geom* geom, const float* bank,
                                int ntaps, void* scratch, int64_t scratch_bytes, int32_t* peaks, int64_t cap, int32_t* count,
                                ral_stream s) {
  if (!x || !geom || !bank || !scratch || !peaks || !count) return ral_fail("beat_records: null pointer");
  BeatGeom g;
  const char* why = beat_geom(leads, geom, ntaps, g);
  if (!why && (R < 1 || R > 65535 || T < 1 || T > 0x7fffffffLL)) why = "1 <= R <= 65535 and 1 <= T < 2^31";
  if (!why && cap < T / (g.rf + 1) + 1) why = "cap >= T / (Rf + 1) + 1";
  if (!why && (((uintptr_t)scratch & 7) || scratch_bytes < beat_scratch(R, T, g, nullptr, nullptr)))
    why = "an 8-byte aligned scratch of ral_beat_records_scratch_bytes bytes";
  if (!why && (T + g.tile - 1) / g.tile > 0x7fffffffLL) why = "fewer than 2^31 tiles per record";
  if (why) {
    char gt[160];
    beat_geom_text(geom, gt, sizeof(gt));
    return ral_fail("beat_records: need %s (R=%lld leads=%d T=%lld ntaps=%d cap=%lld scratch_bytes=%lld %s)", why, (long long)R, leads,
                (long long)T, ntaps, (long long)cap, (long long)scratch_bytes, gt);
  }
  hipStream_t st = (hipStream_t)s;
  BeatScratch sc;
  beat_scratch(R, T, g, scratch, &sc);
  const long long ft = (T + g.tile - 1) / g.tile;
  k_beat_feature_records<<<dim3((unsigned)ft, (unsigned)R), BEAT_THREADS, beat_feature_lds_bytes(g), st>>>(x, T, g, bank, sc);
  k_beat_pick_records<<<dim3((unsigned)sc.NT, (unsigned)R), BEAT_THREADS, beat_pick_lds_bytes(g), st>>>(x, T, g, sc);
  k_beat_gather_records<<<dim3((unsigned)R), BEAT_THREADS, 0, st>>>(T, g, sc, peaks, cap, count);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_beat_pool(float* hist, const float* x, int64_t x_total, const ral_beat_row* table, int rows,
                             ral_beat_row* table_dev, int upload, int64_t capacity, int leads, const ral_beat_geom* geom,
                             const float* bank, int ntaps, int hist_len, void* scratch, int64_t scratch_bytes, int64_t* peaks,
                             int64_t peaks_total, int32_t* count, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !geom || !bank || !scratch || !peaks || !count) return ral_fail("beat_pool: null pointer");
  hipStream_t st = (hipStream_t)s;
  BeatGeom g;
  int bad = -1;
  long long S = 1;
  const char* why = beat_geom(leads, geom, ntaps, g);
  if (!why) why = beat_pool_fault(table, rows, capacity, g, hist_len, x_total, peaks_total, upload != 0, &bad);
  if (!why) {
    S = beat_pool_span(table, rows, g);
    if (((uintptr_t)scratch & 7) || scratch_bytes < beat_scratch(rows, S, g, nullptr, nullptr))
      why = "an 8-byte aligned scratch of ral_beat_records_scratch_bytes(rows, leads, the longest span of f, ...) bytes";
  }
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, st) : 0;
  if (!rc) {
    BeatScratch sc;
    beat_scratch(rows, S, g, scratch, &sc);
    long long d_max = 0;
    for (int r = 0; r < rows; ++r) d_max = table[r].d > d_max ? table[r].d : d_max;
    const long long ft = (S + g.tile - 1) / g.tile, pt = (d_max + BEAT_PICK - 1) / BEAT_PICK;
    k_beat_feature_pool<<<dim3((unsigned)ft + 1, (unsigned)rows), BEAT_THREADS, beat_feature_lds_bytes(g), st>>>(
        hist, x, table_dev, capacity, hist_len, g, bank, sc);
    if (pt > 0)
      k_beat_pick_pool<<<dim3((unsigned)pt, (unsigned)rows), BEAT_THREADS, beat_pick_lds_bytes(g), st>>>(hist, x, table_dev, capacity,
                                                                                                       hist_len, g, sc);
    k_beat_gather_pool<<<dim3((unsigned)rows), BEAT_THREADS, 0, st>>>(table_dev, g, sc, (long long*)peaks, count);
  }
  char gt[160] = "";
  if (rc) beat_geom_text(geom, gt, sizeof(gt));
  return table_done("beat_pool", rc, why, bad, "rows=%d capacity=%lld leads=%d ntaps=%d hist_len=%d x_total=%lld "
                    "peaks_total=%lld scratch_bytes=%lld %s", rows, (long long)capacity, leads, ntaps, hist_len, (long long)x_total,
                    (long long)peaks_total, (long long)scratch_bytes, gt);
}

extern "C" int ral_beat_match(const int32_t* ref, const int32_t* ref_count, int64_t ref_cap, const int32_t* det,
                              const int32_t* det_count, int64_t det_cap, int64_t R, int64_t tol, int64_t* out, ral_stream s) {
  if (!ref || !ref_count || !det || !det_count || !out) return ral_fail("beat_match: null pointer");
  if (R < 1 || R > (1LL << 30) || ref_cap < 1 || det_cap < 1 || tol < 0)
    return ral_fail("beat_match: need 1 <= R <= 2^30, ref_cap, det_cap >= 1 and tol >= 0 (R=%lld ref_cap=%lld det_cap=%lld tol=%lld)",
                (long long)R, (long long)ref_cap, (long long)det_cap, (long long)tol);
  k_beat_match<<<dim3((unsigned)((R + 63) / 64)), 64, 0, (hipStream_t)s>>>(ref, ref_count, ref_cap, det, det_count, det_cap, R, tol,
                                                                         (long long*)out);
  HIP_OK(hipGetLastError());
  return 0;
}
