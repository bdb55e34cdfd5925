// Heart-rate variability of classified beats, window by window (ral_hrv_windows; host side: hrv.py).
//
// include/ralenet.h has the definition.  One device function, hrv_window, serves records and streams: it is handed one ascending
// beat list (with labels or without) and one window [w0, w1) of it, and everything it computes depends on the intervals of that
// window relative to w0 alone - so the windows of a stream, analysed push by push on the beats the stream has kept, carry the bits
// of the windows of the complete record.
//
// One workgroup of 256 threads per table row:
//   locate     two binary searches in the ascending list: the beats [lo, hi) of the window
//   gather     the NN intervals are compacted in beat order into LDS (q, d) with wave ballots and prefix counts - no atomics, so
//              the order is the beat order; the integer sums S1, S2, D2 and the counts k, n50 are formed on the way (exact, so
//              their reduction order cannot matter)
//   time       thread 0 forms the five time-domain values in fp64 from the exact integers and rounds each once
//   spectrum   y = fp32(d - S1 / m) into LDS; thread t takes the bins k = t, t + 256, ... and loops j ascending over LDS (every
//              lane reads the same address: a broadcast); the phase (k + 1) q mod W is exact integer arithmetic (a reciprocal
//              multiply with one correction step); psd_k goes to LDS, over d, which is no longer needed
//   bands      lanes 0 .. 3 of wave 0 add the bins of VLF, LF, HF and of all bands, each sequentially in ascending k
// No floating-point atomics, no scratch memory: the order of every floating-point sum depends on the geometry and on m alone.
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_slots.hpp"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int HV_THREADS = 256;
constexpr int HV_WAVE = 64;
constexpr int HV_WAVES = HV_THREADS / HV_WAVE;
constexpr int HV_MAX_M = 4096;       // NN intervals of a window at most: 12 bytes each, 48 KB of LDS
constexpr int HV_MAX_F = 4096;       // frequency bins at most (they reuse the intervals' LDS)

struct HrvGeom {
  int W, lo_n, hi_n, t50, F, min_nn, max_m, nd;      // nd = max(max_m, F): entries of the LDS array that d and psd share
  unsigned inv;                                     // floor(2^32 / W)
  double fs;
};

typedef ral_hrv_row HrvRow;

// the first index in [0, n) whose position is >= v (n if none)
RAL_DEV int hrv_lower(const int* __restrict__ p, int n, long long v) {
  int a = 0, b = n;
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if ((long long)p[mid] < v) a = mid + 1; else b = mid;
  }
  return a;
}

RAL_DEV long long hrv_wave_sum(long long v) {
#pragma unroll
  for (int o = HV_WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o, HV_WAVE);
  return v;
}

// x mod W for x < 2^31: q = umulhi(x, floor(2^32 / W)) is floor(x / W) or one less
RAL_DEV unsigned hrv_mod(unsigned x, unsigned W, unsigned inv) {
  unsigned r = x - __umulhi(x, inv) * W;
  return r >= W ? r - W : r;
}

// exact m S2 - S1^2 (>= 0) as fp64: 128-bit integer arithmetic, then one conversion (exact below 2^53)
RAL_DEV double hrv_var_num(long long m, unsigned long long S2, unsigned long long S1) {
  const unsigned __int128 a = (unsigned __int128)(unsigned long long)m * S2, b = (unsigned __int128)S1 * S1;
  const unsigned __int128 n = a >= b ? a - b : 0;
  const unsigned long long hi = (unsigned long long)(n >> 64), lo = (unsigned long long)n;
  return hi ? (double)hi * 18446744073709551616.0 + (double)lo : (double)lo;
}

// One window.  pos / lab: the record's list (lab may be null: every beat is N), n its length.  Results: counts[4], stats[10],
// psd[F] (or null).  smem: g.max_m ints (q), g.nd ints (d, later psd as floats), g.max_m floats (y).
RAL_DEV void hrv_window(const HrvGeom& g, const int* __restrict__ pos, const int* __restrict__ lab, int n, long long w0,
                        long long w1, const int* __restrict__ band, int* __restrict__ counts, float* __restrict__ stats,
                        float* __restrict__ psd, int* smem) {
  __shared__ int s_cnt[HV_WAVES];
  __shared__ long long s_red[5][HV_WAVES];
  __shared__ float s_band[4];
  int* q = smem;
  int* d = smem + g.max_m;
  float* y = reinterpret_cast<float*>(smem + g.max_m + g.nd);
  float* pk = reinterpret_cast<float*>(d);
  const int tid = threadIdx.x, lane = tid & (HV_WAVE - 1), wave = tid / HV_WAVE;

  const int lo = hrv_lower(pos, n, w0), hi = hrv_lower(pos, n, w1);
  long long s1 = 0, s2 = 0, d2 = 0, kn = 0;      // kn = k + (n50 << 32)
  int m = 0;
  for (int base = lo + 1; base < hi; base += HV_THREADS) {
    const int i = base + tid;
    bool nn = false;
    int di = 0, pi = 0;
    if (i < hi) {
      pi = pos[i];
      const int pp = pos[i - 1];
      di = pi - pp;
      const bool ok1 = !lab || (lab[i] == 0 && lab[i - 1] == 0);
      nn = ok1 && di >= g.lo_n && di <= g.hi_n;
      if (nn) {
        s1 += di;
        s2 += (long long)di * di;
        if (i - 2 >= lo) {
          const int dp = pp - pos[i - 2];
          if ((!lab || lab[i - 2] == 0) && dp >= g.lo_n && dp <= g.hi_n) {
            const long long dl = (long long)di - dp, ad = dl < 0 ? -dl : dl;
            d2 += dl * dl;
            kn += 1 + (ad > g.t50 ? (1LL << 32) : 0);
          }
        }
      }
    }
    const unsigned long long bal = __ballot(nn);
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int at = m + __popcll(bal & ((1ULL << lane) - 1)), all = 0;
#pragma unroll
    for (int w = 0; w < HV_WAVES; ++w) {
      at += w < wave ? s_cnt[w] : 0;
      all += s_cnt[w];
    }
    if (nn && at < g.max_m) q[at] = (int)(pi - w0), d[at] = di;      // (at < max_m always: the intervals add up to less than W)
    m += all;
    __syncthreads();
  }
  m = m < g.max_m ? m : g.max_m;
  {
    const long long v[5] = {s1, s2, d2, kn, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const long long t = hrv_wave_sum(v[e]);
      if (lane == 0) s_red[e][wave] = t;
    }
    __syncthreads();
    s1 = s2 = d2 = kn = 0;
#pragma unroll
    for (int w = 0; w < HV_WAVES; ++w) s1 += s_red[0][w], s2 += s_red[1][w], d2 += s_red[2][w], kn += s_red[3][w];
  }
  const int k = (int)(kn & 0xffffffffLL), n50 = (int)(kn >> 32);
  const float fnan = nanf("");
  if (tid == 0) {
    counts[0] = hi - lo, counts[1] = m, counts[2] = k, counts[3] = n50;
    const double dm = (double)m, dS1 = (double)s1;
    stats[0] = m >= 1 ? (float)(dS1 / (dm * g.fs)) : fnan;
    stats[1] = m >= 1 ? (float)(60.0 * dm * g.fs / dS1) : fnan;
    stats[2] = m >= 2 ? (float)(sqrt(hrv_var_num(m, (unsigned long long)s2, (unsigned long long)s1) / (dm * (dm - 1.0))) / g.fs) : fnan;
    stats[3] = k >= 1 ? (float)(sqrt((double)d2 / (double)k) / g.fs) : fnan;
    stats[4] = k >= 1 ? (float)((double)n50 / (double)k) : fnan;
  }
  if (m < g.min_nn) {
    if (tid < 5) stats[5 + tid] = fnan;
    if (psd)
      for (int e = tid; e < g.F; e += HV_THREADS) psd[e] = fnan;
    return;
  }
  const double mean = (double)s1 / (double)m;
  for (int j = tid; j < m; j += HV_THREADS) y[j] = (float)((double)d[j] - mean);
  __syncthreads();                                   // (d has been read: psd may overwrite it)
  const float scale = (float)(2.0 / ((double)m * g.fs * g.fs)), fW = (float)g.W;
  for (int kk = tid; kk < g.F; kk += HV_THREADS) {
    const unsigned k1 = (unsigned)kk + 1u;
    float YC = 0.f, YS = 0.f, CC = 0.f, SS = 0.f, CS = 0.f;
    for (int j = 0; j < m; ++j) {
      const unsigned r = hrv_mod(k1 * (unsigned)q[j], (unsigned)g.W, g.inv);
      float s, c;
      sincospif((float)(2u * r) / fW, &s, &c);      // 2 r < 2^32; the angle 2 pi r / W lies in [0, 2 pi)
      const float v = y[j];
      YC = fmaf(v, c, YC);
      YS = fmaf(v, s, YS);
      CC = fmaf(c, c, CC);
      SS = fmaf(s, s, SS);
      CS = fmaf(c, s, CS);
    }
    float st, ct;
    sincosf(0.5f * atan2f(2.f * CS, CC - SS), &st, &ct);
    const float yc = ct * YC + st * YS, ys = ct * YS - st * YC;
    const float x2 = 2.f * ct * st * CS;
    const float cc = ct * ct * CC + x2 + st * st * SS, ss = ct * ct * SS - x2 + st * st * CC;
    const float P = 0.5f * ((cc != 0.f ? yc * yc / cc : 0.f) + (ss != 0.f ? ys * ys / ss : 0.f));
    pk[kk] = P * scale;
  }
  __syncthreads();
  if (psd)
    for (int e = tid; e < g.F; e += HV_THREADS) psd[e] = pk[e];
  if (tid < 4) {
    float acc = 0.f;
    for (int e = 0; e < g.F; ++e)
      if (tid == 3 || band[e] == tid) acc += pk[e];
    s_band[tid] = acc;
    stats[5 + tid] = acc;
  }
  __syncthreads();
  if (tid == 0) stats[9] = s_band[1] / s_band[2];
}

// grid (rows): table row blockIdx.x
__global__ __launch_bounds__(HV_THREADS) void k_hrv_windows(const int* __restrict__ pos, const int* __restrict__ label,
                                                            const int* __restrict__ count, long long cap,
                                                            const HrvRow* __restrict__ tab, HrvGeom g, const int* __restrict__ band,
                                                            int* __restrict__ counts, float* __restrict__ stats,
                                                            float* __restrict__ psd) {
  extern __shared__ __attribute__((aligned(16))) int hrv_smem[];
  const HrvRow t = tab[blockIdx.x];
  long long n = count[t.rec];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const size_t o = (size_t)t.rec * (size_t)cap, row = blockIdx.x;
  hrv_window(g, pos + o, label ? label + o : nullptr, (int)n, t.w0, t.w1, band, counts + row * 4, stats + row * 10,
             psd ? psd + row * (size_t)g.F : nullptr, hrv_smem);
}

const char* hrv_geom(const ral_hrv_geom* p, HrvGeom& g) {
  if (!p) return "a geometry";
  if (p->W < 2) return "2 <= W < 2^31";
  if (p->lo_n < 1 || p->hi_n < p->lo_n) return "1 <= lo_n <= hi_n";
  if (p->F < 1 || p->F > HV_MAX_F) return "1 <= F <= 4096";
  if ((long long)p->F * p->W >= (1LL << 31)) return "F * W < 2^31";
  if ((p->W - 1) / p->lo_n > HV_MAX_M) return "max_m = (W - 1) // lo_n <= 4096";
  if (p->min_nn < 2) return "2 <= min_nn";
  if (p->t50 < 0) return "t50 >= 0";
  if (!(p->fs > 0.0) || !isfinite(p->fs)) return "a finite fs > 0";
  g.W = p->W, g.lo_n = p->lo_n, g.hi_n = p->hi_n, g.t50 = p->t50, g.F = p->F, g.min_nn = p->min_nn, g.fs = p->fs;
  g.max_m = (p->W - 1) / p->lo_n;
  g.max_m = g.max_m < 1 ? 1 : g.max_m;
  g.nd = g.max_m > g.F ? g.max_m : g.F;
  g.inv = (unsigned)((1ULL << 32) / (unsigned)p->W);
  return nullptr;
}

}  // namespace

// the rule a call breaks (*bad: the table row that breaks it, or -1), or null; the table is read only when it is uploaded
static const char* hrv_fault(long long R, long long cap, const ral_hrv_row* tab, long long rows, int upload, const ral_hrv_geom* geom,
                             HrvGeom& g, long long* bad) {
  *bad = -1;
  if (const char* why = hrv_geom(geom, g)) return why;
  if (R < 1 || R > 0x7fffffffLL || cap < 1 || cap > 0x7fffffffLL) return "1 <= R < 2^31 and 1 <= cap < 2^31";
  if (rows < 0 || rows > 0x7fffffffLL) return "0 <= rows < 2^31";
  for (long long r = 0; upload && r < rows; ++r) {
    const ral_hrv_row& t = tab[r];
    *bad = r;
    if (t.rec < 0 || t.rec >= R) return "0 <= rec < R";
    if (t.w0 < 0 || t.w1 <= t.w0 || t.w1 > t.w0 + g.W) return "0 <= w0 < w1 <= w0 + W";
  }
  *bad = -1;
  return nullptr;
}

extern "C" int ral_hrv_windows(const int32_t* pos, const int32_t* label_or_null, const int32_t* count, int64_t R, int64_t cap,
                               const ral_hrv_row* table, int64_t rows, ral_hrv_row* table_dev, int upload, const ral_hrv_geom* geom,
                               const int32_t* band, int32_t* counts, float* stats, float* psd_or_null, ral_stream s) {
  if (!pos || !count || !table_dev || (upload && !table) || !geom || !band || !counts || !stats)
    return ral_fail("hrv_windows: null pointer");
  HrvGeom g;
  long long bad = -1;
  const char* why = hrv_fault(R, cap, table, rows, upload, geom, g, &bad);
  const int rc = why ? -1 : (upload && rows > 0) ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc && rows > 0) {
    const size_t lds = ((size_t)2 * g.max_m + g.nd) * 4;
    k_hrv_windows<<<dim3((unsigned)rows), HV_THREADS, lds, (hipStream_t)s>>>(pos, label_or_null, count, cap, table_dev, g, band, counts,
                                                                           stats, psd_or_null);
  }
  return table_done("hrv_windows", rc, why, bad, "R=%lld cap=%lld rows=%lld W=%d lo_n=%d hi_n=%d t50=%d F=%d min_nn=%d fs=%g",
                    (long long)R, (long long)cap, (long long)rows, geom->W, geom->lo_n, geom->hi_n, geom->t50, geom->F,
                    geom->min_nn, geom->fs);
}
