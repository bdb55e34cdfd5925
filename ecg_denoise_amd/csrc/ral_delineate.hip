// Beat delineation in records (ral_delineate_records; host side: delineate.py).
//
// The delineator (include/ralenet.h has the definition): for a beat at p, the QRS onset and offset are the ends of the runs of
// g quiet samples of the smoothed slope activity a that lie nearest to p inside [p - Wq, p + Wq] (quiet: a <= q0 times the
// largest a of that window); the T peak is the first largest deviation s of the smoothed leads from their level at the onset
// over [off + gt, lim], and the T end the first largest trapezium area behind that peak.  Every beat is measured on its own, by
// one wave, from the record, its own position and the next beat's.
//
// A lane owns samples e = lane, lane + 64, ... of a window and forms each of their sums alone, one term at a time in the order of
// the definition; no product is followed by an addition, so nothing contracts and the four integers are those of the numpy
// restatement.  The wave keeps d over [lo - g - m, hi + g + m], a over [lo - g, hi + g] and s over [t0, lim] in LDS (each cut to
// the record).  Max and argmax are butterflies over (value, index) pairs that prefer the smaller index on equal values; a quiet
// run is a per-lane flag, followed by a butterfly over the indices that passed.
//
// Launch: one, grid (cap, R), a wave per beat (a beat at or beyond count writes the padding).
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_wave_pick.hpp"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int DL_LDS_BYTES = 65536;            // the budget: what a kernel gets without opting into more

struct DelinGeom {
  int leads, h, m, wq, g, m2, gt, wt;
  int nd, na, ns;      // floats of d, a and s in LDS: 2 (Wq + g + m) + 1, 2 (Wq + g) + 1, Wt + 1
  float q0;
};

size_t delin_lds_bytes(const DelinGeom& g) { return ((size_t)g.nd + g.na + g.ns) * sizeof(float); }

// grid (cap, R): beat blockIdx.x of record blockIdx.y
__global__ __launch_bounds__(DL_WAVE) void k_delineate_records(const float* __restrict__ x, long long T, DelinGeom g,
                                                               const int* __restrict__ peaks, const int* __restrict__ count,
                                                               long long cap, int* __restrict__ on_out, int* __restrict__ off_out,
                                                               int* __restrict__ tpeak_out, int* __restrict__ tend_out) {
  extern __shared__ __attribute__((aligned(16))) char delin_smem[];
  float* const d = reinterpret_cast<float*>(delin_smem);
  float* const a = d + g.nd;
  float* const sv = a + g.na;
  const int lane = threadIdx.x;
  const long long r = blockIdx.y, i = blockIdx.x, o = r * cap + i, top = T - 1;
  long long n = count[r];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  int on = -1, off = -1, tpeak = -1, tend = -1;
  if (i < n) {
    const float* xr = x + (size_t)r * g.leads * T;
    const long long p = delin_clamp(peaks[o], top);      // (the positions live on the device: every read stays in the record)
    const long long lo = p - g.wq > 0 ? p - g.wq : 0, hi = p + g.wq < top ? p + g.wq : top;
    const long long alo = lo - g.g > 0 ? lo - g.g : 0, ahi = hi + g.g < top ? hi + g.g : top;
    const long long dlo = alo - g.m > 0 ? alo - g.m : 0, dhi = ahi + g.m < top ? ahi + g.m : top;
    for (long long u = dlo + lane; u <= dhi; u += DL_WAVE) {
      const long long up = delin_clamp(u + g.h, top), dn = delin_clamp(u - g.h, top);
      float acc = 0.f;
      for (int l = 0; l < g.leads; ++l) acc += fabsf(xr[(size_t)l * T + up] - xr[(size_t)l * T + dn]);
      d[u - dlo] = acc;
    }
    __syncthreads();
    float best = 0.f;
    for (long long t = alo + lane; t <= ahi; t += DL_WAVE) {
      float acc = 0.f;
      for (int k = -g.m; k <= g.m; ++k) acc += d[delin_clamp(t + k, top) - dlo];
      a[t - alo] = acc;
      if (t >= lo && t <= hi) best = fmaxf(best, acc);
    }
    __syncthreads();
    const float A = delin_max(best);
    if (A != 0.f) {                                       // (A is the same in every lane: the branches below are the wave's)
      const float theta = g.q0 * A;
      long long won = -1, woff = T;
      for (long long t = lo + lane; t <= p; t += DL_WAVE) {
        bool quiet = t - g.g >= 0;
        for (int j = 1; quiet && j <= g.g; ++j) quiet = a[t - j - alo] <= theta;
        if (quiet) won = t;                               // (ascending: the lane's largest stays)
      }
      for (long long t = p + lane; t <= hi; t += DL_WAVE) {
        bool quiet = t + g.g <= top;
        for (int j = 1; quiet && j <= g.g; ++j) quiet = a[t + j - alo] <= theta;
        if (quiet && t < woff) woff = t;
      }
      won = delin_imax(won);
      woff = delin_imin(woff);
      on = (int)won;
      off = woff == T ? -1 : (int)woff;
      if (on >= 0 && off >= 0) {
        long long lim = p + g.wt < top ? p + g.wt : top;
        if (i + 1 < n) {
          const long long cut = p + (2 * ((long long)peaks[o + 1] - p)) / 3;
          lim = cut < lim ? cut : lim;
        }
        const long long t0 = (long long)off + g.gt;
        if (t0 <= lim) {
          for (long long t = t0 + lane; t <= lim; t += DL_WAVE) sv[t - t0] = 0.f;
          for (int l = 0; l < g.leads; ++l) {
            const float* xl = xr + (size_t)l * T;
            float b = 0.f;
            for (int k = -g.m2; k <= g.m2; ++k) b += xl[delin_clamp(on + k, top)];
            for (long long t = t0 + lane; t <= lim; t += DL_WAVE) {
              float z = 0.f;
              for (int k = -g.m2; k <= g.m2; ++k) z += xl[delin_clamp(t + k, top)];
              sv[t - t0] += fabsf(z - b);                 // (a lane adds to the values it owns, in lead order)
            }
          }
          __syncthreads();
          float v = -1.f;
          long long at = T;
          for (long long t = t0 + lane; t <= lim; t += DL_WAVE)
            if (sv[t - t0] > v) v = sv[t - t0], at = t;
          delin_argmax(v, at);
          if (v != 0.f && at != lim) {
            const long long tp = at;
            const float sp = v;
            v = -1.f, at = T;
            for (long long t = tp + lane; t <= lim; t += DL_WAVE) {
              const float area = (sp - sv[t - t0]) * (float)(2 * lim - tp - t);
              if (area > v) v = area, at = t;
            }
            delin_argmax(v, at);
            tpeak = (int)tp, tend = (int)at;
          }
        }
      }
    }
  }
  if (lane == 0) on_out[o] = on, off_out[o] = off, tpeak_out[o] = tpeak, tend_out[o] = tend;
}

// ------------------------------------------------------------------------------------------------ host
const char* delin_geom(int leads, const ral_delin_geom* p, DelinGeom& g) {
  if (!p) return "a geometry";
  if (leads < 1 || leads > 65535) return "1 <= leads <= 65535";
  const int big = 1 << 20;
  if (p->h < 1 || p->h > big || p->m < 0 || p->m > big || p->wq < 1 || p->wq > big || p->g < 1 || p->g > big || p->m2 < 0 ||
      p->m2 > big || p->gt < 0 || p->gt > big || p->wt < 1 || p->wt > big)
    return "1 <= h, Wq, g, Wt <= 2^20 and 0 <= m, m2, gt <= 2^20";
  if (!isfinite(p->q0) || p->q0 < 0.f) return "a finite q0 >= 0";
  g.leads = leads, g.h = p->h, g.m = p->m, g.wq = p->wq, g.g = p->g, g.m2 = p->m2, g.gt = p->gt, g.wt = p->wt, g.q0 = p->q0;
  g.nd = 2 * (g.wq + g.g + g.m) + 1, g.na = 2 * (g.wq + g.g) + 1, g.ns = g.wt + 1;
  if (delin_lds_bytes(g) > (size_t)DL_LDS_BYTES)
    return "the windows of one beat (2 (Wq + g + m) + 1, 2 (Wq + g) + 1 and Wt + 1 floats) within 64 KB of LDS";
  return nullptr;
}

}  // namespace

extern "C" int ral_delineate_records(const float* x, int64_t R, int leads, int64_t T, const ral_delin_geom* geom, const int32_t* peaks,
                                     const int32_t* count, int64_t cap, int32_t* on, int32_t* off, int32_t* tpeak, int32_t* tend,
                                     ral_stream s) {
  if (!x || !geom || !peaks || !count || !on || !off || !tpeak || !tend) return ral_fail("delineate_records: null pointer");
  DelinGeom g;
  const char* why = delin_geom(leads, geom, g);
  if (!why && (R < 1 || R > 65535 || T < 1 || T > 0x7fffffffLL)) why = "1 <= R <= 65535 and 1 <= T < 2^31";
  if (!why && (cap < 1 || cap > 0x7fffffffLL)) why = "1 <= cap < 2^31";
  if (why)
    return ral_fail("delineate_records: need %s (R=%lld leads=%d T=%lld cap=%lld h=%d m=%d Wq=%d g=%d m2=%d gt=%d Wt=%d q0=%g)", why,
                    (long long)R, leads, (long long)T, (long long)cap, geom->h, geom->m, geom->wq, geom->g, geom->m2, geom->gt,
                    geom->wt, geom->q0);
  k_delineate_records<<<dim3((unsigned)cap, (unsigned)R), DL_WAVE, delin_lds_bytes(g), (hipStream_t)s>>>(x, T, g, peaks, count, cap, on,
                                                                                                       off, tpeak, tend);
  HIP_OK(hipGetLastError());
  return 0;
}
