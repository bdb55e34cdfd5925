// P wave and ST level of delineated beats in records (ral_pst_records; host side: pst.py).
//
// The measurement (include/ralenet.h has the definition): for a beat at p with the delineator's QRS onset on and offset off,
// the isoelectric level of a lead is its smoothed value z at e = max(on - g, 0), inside the quiet run in front of the QRS; the
// ST level of a lead is the mean of its samples around off + j over that level; the P peak is the first largest deviation s of
// the smoothed leads from that level over [plo, e], accepted if it lies strictly inside and reaches p0 times the largest s of
// the QRS, and the P onset and end are the first largest trapezium areas in front of and behind that peak.  Every beat is
// measured on its own, by one wave, from the record, its own position, on and off, and the two neighbouring positions.
//
// A lane owns samples t = plo + lane, plo + lane + 64, ... of the P window and forms each of their sums alone, one term at a
// time in the order of the definition; no product is followed by an addition, so nothing contracts and the three integers and
// the ST levels are those of the numpy restatement, bit for bit.  The wave keeps s over [plo, e] in LDS (at most Wp + 1
// floats) and, one lead at a time, that lead's samples over [plo - m2, e + m2] (at most Wp + 2 m2 + 1 floats), from which
// the 2 m2 + 1 terms of every smoothed value of the window are read: staged, the window's loads from the record fall from
// 2 m2 + 1 per value to one (measured, tools/pst_bench.py: 1.33 times the beats/s at 2 leads and 360 Hz, 1.78 times at 12
// leads and 500 Hz).  The QRS, whose length the caller's on and off decide, is not kept: it is walked in stretches of
// PST_QK * 64 samples whose s a lane accumulates in registers, lead by lead, from the record through L1 / L2 as the
// delineator reads it, and only the running maximum stays.  The ST levels are formed one lead per lane.  Whether on and off
// count is decided here (0 <= on <= p <= off <= T - 1), every index is clamped into the record and the neighbouring
// positions only move plo and lim: no read leaves the record or the lists whatever the tensors hold.
//
// Launch: one, grid (cap, R), a wave per beat (a beat at or beyond count writes the padding).
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_wave_pick.hpp"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int PST_LDS_BYTES = 65536;           // the budget: what a kernel gets without opting into more
constexpr int PST_QK = 2;                      // stretches of 128 samples: one holds a QRS up to 350 ms at 360 Hz

struct PstGeom {
  int leads, m2, g, wp, j;
  float w, p0;
};

// s over the P window, and the samples of one lead under it
size_t pst_lds_bytes(const PstGeom& g) { return (2 * (size_t)g.wp + 2 * (size_t)g.m2 + 2) * sizeof(float); }

// z_l[t]: k ascending, one term at a time
RAL_DEV float pst_z(const float* __restrict__ xl, long long t, int m2, long long top) {
  float z = 0.f;
  for (int k = -m2; k <= m2; ++k) z += xl[delin_clamp(t + k, top)];
  return z;
}

// the same sum over staged samples: w[0] is x_l[c(t - m2)]
RAL_DEV float pst_zs(const float* w, int m2) {
  float z = 0.f;
  for (int k = 0; k <= 2 * m2; ++k) z += w[k];
  return z;
}

// grid (cap, R): beat blockIdx.x of record blockIdx.y
__global__ __launch_bounds__(DL_WAVE) void k_pst_records(const float* __restrict__ x, long long T, PstGeom g,
                                                         const int* __restrict__ peaks, const int* __restrict__ count,
                                                         long long cap, const int* __restrict__ on_in,
                                                         const int* __restrict__ off_in, int* __restrict__ pon_out,
                                                         int* __restrict__ ppeak_out, int* __restrict__ poff_out,
                                                         float* __restrict__ st_out) {
  extern __shared__ __attribute__((aligned(16))) char pst_smem[];
  float* const sv = reinterpret_cast<float*>(pst_smem);
  const int lane = threadIdx.x;
  const long long r = blockIdx.y, i = blockIdx.x, o = r * cap + i, top = T - 1;
  const float* xr = x + (size_t)r * g.leads * T;
  long long n = count[r];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  int pon = -1, ppeak = -1, poff = -1;
  long long e = -1, ts = -1;                               // e >= 0: the beat has an onset; ts >= 0: and a sample to read ST at
  if (i < n) {
    const long long p = delin_clamp(peaks[o], top);        // (the positions live on the device: every read stays in the record)
    const long long on = on_in[o], off = off_in[o];
    const bool has_off = off >= p && off <= top;
    if (on >= 0 && on <= p) {                              // (the same in every lane: the branches below are the wave's)
      e = on - g.g > 0 ? on - g.g : 0;
      if (has_off) {
        long long lim = top;
        if (i + 1 < n) {
          const long long cut = p + (2 * ((long long)peaks[o + 1] - p)) / 3;
          lim = cut < lim ? cut : lim;
        }
        if (off + g.j <= lim) ts = off + g.j;
      }
      long long plo = on - g.wp > 0 ? on - g.wp : 0;
      if (i > 0) {
        const long long prev = peaks[o - 1], cut = prev + (2 * (p - prev)) / 3;
        plo = cut > plo ? cut : plo;
      }
      if (plo <= e) {                                      // (e - plo <= Wp: s fits its Wp + 1 floats)
        for (long long t = plo + lane; t <= e; t += DL_WAVE) sv[t - plo] = 0.f;
        float* const raw = sv + g.wp + 1;                  // raw[u] = x_l[c(plo - m2 + u)] of the lead at hand
        const long long nr = e - plo + 2 * g.m2 + 1;
        for (int l = 0; l < g.leads; ++l) {
          const float* xl = xr + (size_t)l * T;
          __syncthreads();                                 // (the lead before has been read)
          for (long long u = lane; u < nr; u += DL_WAVE) raw[u] = xl[delin_clamp(plo - g.m2 + u, top)];
          __syncthreads();
          const float b = pst_zs(raw + (e - plo), g.m2);
          for (long long t = plo + lane; t <= e; t += DL_WAVE)
            sv[t - plo] += fabsf(pst_zs(raw + (t - plo), g.m2) - b);   // (a lane adds to the values it owns, in lead order)
        }
        __syncthreads();
        float v = -1.f;
        long long at = T;
        for (long long t = plo + lane; t <= e; t += DL_WAVE)
          if (sv[t - plo] > v) v = sv[t - plo], at = t;
        delin_argmax(v, at);
        if (at != plo && at != e && v != 0.f) {
          const long long pk = at, qhi = has_off && off > p ? off : p;
          const float sp = v;
          float best = 0.f;                                // (s >= 0, and a slot past qhi stays 0)
          for (long long c0 = on; c0 <= qhi; c0 += PST_QK * DL_WAVE) {
            float acc[PST_QK];
#pragma unroll
            for (int k = 0; k < PST_QK; ++k) acc[k] = 0.f;
            for (int l = 0; l < g.leads; ++l) {
              const float* xl = xr + (size_t)l * T;
              const float b = pst_z(xl, e, g.m2, top);
#pragma unroll
              for (int k = 0; k < PST_QK; ++k) {
                const long long t = c0 + k * DL_WAVE + lane;
                if (t <= qhi) acc[k] += fabsf(pst_z(xl, t, g.m2, top) - b);
              }
            }
#pragma unroll
            for (int k = 0; k < PST_QK; ++k) best = fmaxf(best, acc[k]);
          }
          const float S = delin_max(best);
          if (!(sp < g.p0 * S)) {
            v = -1.f, at = T;
            for (long long t = plo + lane; t <= pk; t += DL_WAVE) {
              const float area = (sp - sv[t - plo]) * (float)(t + pk - 2 * plo);
              if (area > v) v = area, at = t;
            }
            delin_argmax(v, at);
            pon = (int)at, ppeak = (int)pk;
            v = -1.f, at = T;
            for (long long t = pk + lane; t <= e; t += DL_WAVE) {
              const float area = (sp - sv[t - plo]) * (float)(2 * e - pk - t);
              if (area > v) v = area, at = t;
            }
            delin_argmax(v, at);
            poff = (int)at;
          }
        }
      }
    }
  }
  if (lane == 0) pon_out[o] = pon, ppeak_out[o] = ppeak, poff_out[o] = poff;
  for (int l = lane; l < g.leads; l += DL_WAVE) {          // one lead per lane: a subtraction and a product
    float st = __builtin_nanf("");
    if (ts >= 0) {
      const float* xl = xr + (size_t)l * T;
      st = (pst_z(xl, ts, g.m2, top) - pst_z(xl, e, g.m2, top)) * g.w;
    }
    st_out[(size_t)o * g.leads + l] = st;
  }
}

// ------------------------------------------------------------------------------------------------ host
const char* pst_geom(int leads, const ral_pst_geom* p, PstGeom& g) {
  if (!p) return "a geometry";
  if (leads < 1 || leads > 65535) return "1 <= leads <= 65535";
  const int big = 1 << 20;
  if (p->m2 < 0 || p->m2 > big || p->g < 1 || p->g > big || p->wp < 1 || p->wp > big || p->j < 0 || p->j > big)
    return "1 <= g, Wp <= 2^20 and 0 <= m2, j <= 2^20";
  if (!isfinite(p->w)) return "a finite w";
  if (!isfinite(p->p0) || p->p0 < 0.f) return "a finite p0 >= 0";
  g.leads = leads, g.m2 = p->m2, g.g = p->g, g.wp = p->wp, g.j = p->j, g.w = p->w, g.p0 = p->p0;
  if (pst_lds_bytes(g) > (size_t)PST_LDS_BYTES) return "the P window of one beat (Wp + 1 and Wp + 2 m2 + 1 floats) within 64 KB of LDS";
  return nullptr;
}

}  // namespace

extern "C" int ral_pst_records(const float* x, int64_t R, int leads, int64_t T, const ral_pst_geom* geom, const int32_t* peaks,
                               const int32_t* count, int64_t cap, const int32_t* on, const int32_t* off, int32_t* pon, int32_t* ppeak,
                               int32_t* poff, float* st, ral_stream s) {
  if (!x || !geom || !peaks || !count || !on || !off || !pon || !ppeak || !poff || !st) return ral_fail("pst_records: null pointer");
  PstGeom g;
  const char* why = pst_geom(leads, geom, g);
  if (!why && (R < 1 || R > 65535 || T < 1 || T > 0x7fffffffLL)) why = "1 <= R <= 65535 and 1 <= T < 2^31";
  if (!why && (cap < 1 || cap > 0x7fffffffLL)) why = "1 <= cap < 2^31";
  if (why)
    return ral_fail("pst_records: need %s (R=%lld leads=%d T=%lld cap=%lld m2=%d g=%d Wp=%d j=%d w=%g p0=%g)", why, (long long)R,
                    leads, (long long)T, (long long)cap, geom->m2, geom->g, geom->wp, geom->j, geom->w, geom->p0);
  k_pst_records<<<dim3((unsigned)cap, (unsigned)R), DL_WAVE, pst_lds_bytes(g), (hipStream_t)s>>>(x, T, g, peaks, count, cap, on, off, pon,
                                                                                               ppeak, poff, st);
  HIP_OK(hipGetLastError());
  return 0;
}
