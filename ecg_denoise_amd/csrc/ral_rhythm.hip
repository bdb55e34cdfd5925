// Beat classes in records and live streams (ral_rhythm_records / ral_rhythm_pool; host side: rhythm.py).
//
// The classifier (include/ralenet.h has the definition): beat i is compared with the median template of its up to K = 8
// neighbours - the correlation of its window of 2 Wb + 1 samples per lead with that template, the best over shifts of +-Sa -
// and its RR interval with the median interval of the same neighbourhood.  Every beat is classified on its own, by one wave:
// the order of its sums depends on nothing but the geometry, so a stream classified push by push gives the bits of the record.
//
// One device function, rhythm_beat, serves both forms.  It is handed the beats of the neighbourhood [a, hi) - beat i among
// them - as sources: where the extended window (2 (Wb + Sa) + 1 samples per lead, starting at p - Wb - Sa) of each can be read,
// with the clamp the definition asks for.  For a record a source is the record itself; for a pool it is a window gathered by
// the call (a beat the call's detector has just given) or kept in the slot's ring (one of the K beats before them).
// Per lead the wave stages the neighbours' windows and the beat's own extended window in LDS, forms their means (a wave
// reduction each), the template (per sample a sorting network over the neighbours, padded with +inf), and the three sums per
// shift (a wave reduction each); lane 0 adds them to the running sums in lead order and decides at the end.
//
// Launches:  records  one: grid (cap, R), a wave per beat (a beat at or beyond count writes the padding).
//            pool     gather (the extended windows of the call's new beats, from the history plane and the chunk, into scratch),
//                     classify (a wave per beat that became final), keep (the last K beats' windows and positions into the ring).
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_slots.hpp"
#include <math.h>
#include <stdint.h>
#include <stdio.h>

namespace {

constexpr int RH_K = RAL_RHYTHM_K;             // neighbours at most; the sorting network below has this many inputs
constexpr int RH_SET = RH_K + 1;               // beats of a neighbourhood, beat i among them
constexpr int RH_MIN_REF = RAL_RHYTHM_MIN_REF;
constexpr int RH_WAVE = 64;
constexpr int RH_NS_MAX = 56;                  // shifts (2 Sa + 1) at most
constexpr int RH_LDS_BYTES = 65536;            // the budget: what a kernel gets without opting into more
static_assert(RH_K == 8, "rhythm_sort8 sorts 8 values");

struct RhythmGeom {
  int leads, wb, sa, W, We, NS;     // W = 2 Wb + 1, We = 2 (Wb + Sa) + 1, NS = 2 Sa + 1
  float c0, r0;
};

// sample e of lead l of a beat's extended window: base[l * stride + clamp(off + e, 0, hi)]
struct RhythmSrc {
  const float* base;
  long long stride, off, hi;
};

struct RhythmLds {
  RhythmSrc* src;      // RH_SET
  long long* pos;      // RH_SET
  long long* dif;      // RH_K
  float *nbw, *own, *tpl, *mu, *acc;      // RH_K * W, We, W, RH_K + NS, 2 NS + 1
};

size_t rhythm_lds_bytes(const RhythmGeom& g) {
  return RH_SET * sizeof(RhythmSrc) + (RH_SET + RH_K) * sizeof(long long) +
         ((size_t)(RH_K + 1) * g.W + g.We + RH_K + 3 * g.NS + 1) * sizeof(float);
}

RAL_DEV RhythmLds rhythm_lds(const RhythmGeom& g, char* base) {
  RhythmLds s;
  s.src = reinterpret_cast<RhythmSrc*>(base);
  s.pos = reinterpret_cast<long long*>(s.src + RH_SET);
  s.dif = s.pos + RH_SET;
  s.nbw = reinterpret_cast<float*>(s.dif + RH_K);
  s.own = s.nbw + RH_K * g.W;
  s.tpl = s.own + g.We;
  s.mu = s.tpl + g.W;
  s.acc = s.mu + RH_K + g.NS;
  return s;
}

// the sum over the wave, the same bits in every lane
RAL_DEV float rhythm_sum(float v) {
#pragma unroll
  for (int o = RH_WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o, RH_WAVE);
  return v;
}

#define RH_CE(a, b) { const float lo_ = fminf(v[a], v[b]), hi_ = fmaxf(v[a], v[b]); v[a] = lo_; v[b] = hi_; }
RAL_DEV void rhythm_sort8(float (&v)[8]) {      // 19 exchanges
  RH_CE(0, 1) RH_CE(2, 3) RH_CE(4, 5) RH_CE(6, 7)
  RH_CE(0, 2) RH_CE(1, 3) RH_CE(4, 6) RH_CE(5, 7)
  RH_CE(1, 2) RH_CE(5, 6) RH_CE(0, 4) RH_CE(3, 7)
  RH_CE(1, 5) RH_CE(2, 6)
  RH_CE(1, 4) RH_CE(3, 6)
  RH_CE(2, 4) RH_CE(3, 5)
  RH_CE(3, 4)
}
#undef RH_CE

// the neighbourhood of beat i of n: [a, hi)
RAL_DEV void rhythm_hood(long long i, long long n, long long& a, long long& hi) {
  const long long lo = i - RH_K > 0 ? i - RH_K : 0, top = n - RH_K - 1 > 0 ? n - RH_K - 1 : 0;
  a = lo < top ? lo : top;
  hi = a + RH_K + 1 < n ? a + RH_K + 1 : n;
}

// Beat `self` of the nset beats whose sources and positions the caller has put into L.src / L.pos (and synchronised);
// first: it is beat 0 of its record.  One wave; lane 0 writes the three results.
RAL_DEV void rhythm_beat(const RhythmGeom& g, const RhythmLds& L, int nset, int self, bool first, int* label, float* corr,
                         float* rr) {
  const int lane = threadIdx.x;
  const int nn = nset - 1;
  if (nn < RH_MIN_REF) {
    if (lane == 0) *label = -1, *corr = nanf(""), *rr = nanf("");
    return;
  }
  const float div = (float)g.W;
  if (lane == 0)
    for (int e = 0; e < 2 * g.NS + 1; ++e) L.acc[e] = 0.f;
  for (int lead = 0; lead < g.leads; ++lead) {
    __syncthreads();                                 // (the lead before has been read)
    for (int j = 0, q = 0; j < nset; ++j) {
      const RhythmSrc s = L.src[j];
      const float* p = s.base + (size_t)lead * s.stride;
      if (j == self) {
        for (int e = lane; e < g.We; e += RH_WAVE) {
          const long long at = s.off + e;
          L.own[e] = p[at < 0 ? 0 : (at > s.hi ? s.hi : at)];
        }
      } else {
        for (int e = lane; e < g.W; e += RH_WAVE) {
          const long long at = s.off + g.sa + e;
          L.nbw[q * g.W + e] = p[at < 0 ? 0 : (at > s.hi ? s.hi : at)];
        }
        ++q;
      }
    }
    __syncthreads();
    for (int q = 0; q < nn + g.NS; ++q) {            // the means of the neighbours' windows, then of the beat's shifted ones
      const float* w = q < nn ? L.nbw + q * g.W : L.own + (q - nn);
      float part = 0.f;
      for (int e = lane; e < g.W; e += RH_WAVE) part += w[e];
      const float tot = rhythm_sum(part);
      if (lane == 0) L.mu[q < nn ? q : RH_K + (q - nn)] = tot / div;
    }
    __syncthreads();
    float tt = 0.f;
    for (int k = lane; k < g.W; k += RH_WAVE) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = j < nn ? L.nbw[j * g.W + k] - L.mu[j] : INFINITY;
      rhythm_sort8(v);
      const int ia = (nn - 1) >> 1, ib = nn >> 1;
      float lo = v[0], hi = v[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) lo = j == ia ? v[j] : lo, hi = j == ib ? v[j] : hi;
      const float t = 0.5f * (lo + hi);
      L.tpl[k] = t;
      tt = fmaf(t, t, tt);
    }
    tt = rhythm_sum(tt);
    if (lane == 0) L.acc[0] += tt;
    for (int s = 0; s < g.NS; ++s) {                 // (a lane reads the template values it wrote)
      const float m = L.mu[RH_K + s];
      float tv = 0.f, vv = 0.f;
      for (int k = lane; k < g.W; k += RH_WAVE) {
        const float v = L.own[s + k] - m;
        tv = fmaf(L.tpl[k], v, tv);
        vv = fmaf(v, v, vv);
      }
      tv = rhythm_sum(tv);
      vv = rhythm_sum(vv);
      if (lane == 0) L.acc[1 + 2 * s] += tv, L.acc[2 + 2 * s] += vv;
    }
  }
  if (lane != 0) return;
  float best = 0.f;
  for (int s = 0; s < g.NS; ++s) {
    const float den = L.acc[0] * L.acc[2 + 2 * s];
    const float c = den > 0.f ? L.acc[1 + 2 * s] / sqrtf(den) : 0.f;
    best = s == 0 || c > best ? c : best;
  }
  const int nd = nset - 1;
  for (int j = 0; j < nd; ++j) {                     // the intervals of the neighbourhood, sorted by insertion
    const long long d = L.pos[j + 1] - L.pos[j];
    int e = j;
    for (; e > 0 && L.dif[e - 1] > d; --e) L.dif[e] = L.dif[e - 1];
    L.dif[e] = d;
  }
  const float med = 0.5f * (float)(L.dif[(nd - 1) >> 1] + L.dif[nd >> 1]);
  const float ratio = first ? nanf("") : (float)(L.pos[self] - L.pos[self - 1]) / med;
  *corr = best;
  *rr = ratio;
  *label = best < g.c0 ? 1 : (!first && ratio < g.r0 ? 2 : 0);
}

// grid (cap, R): beat blockIdx.x of record blockIdx.y
__global__ __launch_bounds__(RH_WAVE) void k_rhythm_records(const float* __restrict__ x, long long T, RhythmGeom g,
                                                            const int* __restrict__ peaks, const int* __restrict__ count,
                                                            long long cap, int* __restrict__ label, float* __restrict__ corr,
                                                            float* __restrict__ rr) {
  extern __shared__ __attribute__((aligned(16))) char rhythm_smem[];
  const RhythmLds L = rhythm_lds(g, rhythm_smem);
  const long long r = blockIdx.y, i = blockIdx.x;
  long long n = count[r];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  const long long o = r * cap + i;
  if (i >= n) {
    if (threadIdx.x == 0) label[o] = -1, corr[o] = nanf(""), rr[o] = nanf("");
    return;
  }
  long long a, hi;
  rhythm_hood(i, n, a, hi);
  const int nset = (int)(hi - a);
  if ((int)threadIdx.x < nset) {
    const long long p = peaks[r * cap + a + threadIdx.x];
    RhythmSrc s;
    s.base = x + (size_t)r * g.leads * T, s.stride = T, s.off = p - g.wb - g.sa, s.hi = T - 1;
    L.src[threadIdx.x] = s;
    L.pos[threadIdx.x] = p;
  }
  __syncthreads();
  rhythm_beat(g, L, nset, (int)(i - a), i == 0, label + o, corr + o, rr + o);
}

typedef ral_rhythm_row RhythmRow;

// grid (new beats of the row with the most, rows): the extended window of a new beat, from the row's history plane and chunk
__global__ __launch_bounds__(RH_WAVE) void k_rhythm_gather_pool(const float* __restrict__ hist, const float* __restrict__ x,
                                                                const RhythmRow* __restrict__ tab, long long cap, int hist_len,
                                                                RhythmGeom g, const long long* __restrict__ new_pos,
                                                                float* __restrict__ win) {
  const RhythmRow t = tab[blockIdx.y];
  if ((long long)blockIdx.x >= t.m) return;
  const long long b = t.new_off + blockIdx.x, N = t.n0 + t.c;
  const long long first = new_pos[b] - g.wb - g.sa;
  const float* chunk = x + (size_t)t.x_off * g.leads;
  const float* h = hist + slot_plane(t.turn, t.slot, cap, g.leads, hist_len);
  float* dst = win + (size_t)b * g.leads * g.We;
  for (int lead = 0; lead < g.leads; ++lead)      // (a beat the detector has just given lies inside the history)
    for (int e = threadIdx.x; e < g.We; e += RH_WAVE)
      dst[(size_t)lead * g.We + e] = slot_sample(chunk, t.c, h, hist_len, t.n0, N, lead, first + e);
}

// grid (beats that become final of the row with the most, rows)
__global__ __launch_bounds__(RH_WAVE) void k_rhythm_classify_pool(const RhythmRow* __restrict__ tab, long long cap, RhythmGeom g,
                                                                  const float* __restrict__ ring, const long long* __restrict__ ring_pos,
                                                                  const long long* __restrict__ new_pos, const float* __restrict__ win,
                                                                  long long* __restrict__ out_pos, int* __restrict__ label,
                                                                  float* __restrict__ corr, float* __restrict__ rr) {
  extern __shared__ __attribute__((aligned(16))) char rhythm_smem[];
  const RhythmRow t = tab[blockIdx.y];
  if ((long long)blockIdx.x >= t.ne) return;
  const RhythmLds L = rhythm_lds(g, rhythm_smem);
  const long long i = t.e0 + blockIdx.x, n = t.nb + t.m;
  long long a, hi;
  rhythm_hood(i, n, a, hi);
  const int nset = (int)(hi - a);
  const size_t wsz = (size_t)g.leads * g.We;
  if ((int)threadIdx.x < nset) {
    const long long j = a + threadIdx.x;
    RhythmSrc s;
    s.stride = g.We, s.off = 0, s.hi = g.We - 1;
    if (j >= t.nb) {
      s.base = win + (size_t)(t.new_off + (j - t.nb)) * wsz;
      L.pos[threadIdx.x] = new_pos[t.new_off + (j - t.nb)];
    } else {
      const size_t at = (size_t)t.slot * RH_K + (size_t)(j % RH_K);
      s.base = ring + at * wsz;
      L.pos[threadIdx.x] = ring_pos[at];
    }
    L.src[threadIdx.x] = s;
  }
  __syncthreads();
  const long long o = t.out_off + blockIdx.x;
  if (threadIdx.x == 0) out_pos[o] = L.pos[i - a];
  rhythm_beat(g, L, nset, (int)(i - a), i == 0, label + o, corr + o, rr + o);
}

// grid (K, rows): the last K beats of a row that stays open go to its ring (those of this call; the older ones are there)
__global__ __launch_bounds__(RH_WAVE) void k_rhythm_keep_pool(const RhythmRow* __restrict__ tab, RhythmGeom g, float* __restrict__ ring,
                                                              long long* __restrict__ ring_pos, const long long* __restrict__ new_pos,
                                                              const float* __restrict__ win) {
  const RhythmRow t = tab[blockIdx.y];
  if (!(t.flags & RAL_POOL_KEEP)) return;
  const long long j = t.nb + t.m - 1 - blockIdx.x;
  if (j < t.nb) return;
  const size_t wsz = (size_t)g.leads * g.We, at = (size_t)t.slot * RH_K + (size_t)(j % RH_K);
  const size_t b = (size_t)(t.new_off + (j - t.nb));
  for (size_t e = threadIdx.x; e < wsz; e += RH_WAVE) ring[at * wsz + e] = win[b * wsz + e];
  if (threadIdx.x == 0) ring_pos[at] = new_pos[b];
}

// ------------------------------------------------------------------------------------------------ host
const char* rhythm_geom(int leads, const ral_rhythm_geom* p, RhythmGeom& g) {
  if (!p) return "a geometry";
  if (leads < 1 || leads > 65535) return "1 <= leads <= 65535";
  if (p->wb < 1 || p->wb > (1 << 20) || p->sa < 0 || 2 * p->sa + 1 > RH_NS_MAX) return "1 <= Wb <= 2^20 and 0 <= Sa <= 27";
  if (!isfinite(p->c0) || !isfinite(p->r0)) return "finite c0 and r0";
  g.leads = leads, g.wb = p->wb, g.sa = p->sa, g.c0 = p->c0, g.r0 = p->r0;
  g.W = 2 * g.wb + 1, g.We = 2 * (g.wb + g.sa) + 1, g.NS = 2 * g.sa + 1;
  if (rhythm_lds_bytes(g) > (size_t)RH_LDS_BYTES) return "the windows of eight neighbours of one lead (9 (2 Wb + 1) + 2 (Wb + Sa) + 1 floats) within 64 KB of LDS";
  return nullptr;
}

const char* rhythm_pool_fault(const RhythmRow* tab, int rows, long long cap, const RhythmGeom& g, int hist_len, long long x_total,
                              long long new_total, long long out_total, bool walk, int* bad) {
  *bad = -1;
  if (rows < 1 || rows > 65535) return "1 <= rows <= 65535";
  if (cap < 1) return "capacity >= 1";
  if (hist_len < 1) return "hist_len >= 1";
  if (x_total < 0 || new_total < 0 || out_total < 0) return "x_total, new_total, out_total >= 0";
  if (!walk) return nullptr;
  const long long big = 1LL << 40;
  const SlotRules rules{1, false, "0 <= n0, nb <= 2^40, 0 <= c < 2^30, m >= 0 and ne >= 0",
                        "T = n0 + c >= 1 without RAL_POOL_KEEP, or T = -1 with RAL_POOL_KEEP"};
  auto in_range = [&](const RhythmRow& t) {
    return !(t.n0 < 0 || t.n0 > big || t.c < 0 || t.c > 0x3fffffff || t.nb < 0 || t.nb > big || t.m < 0 || t.ne < 0);
  };
  auto own = [&](const RhythmRow& t) -> const char* {
    if (t.new_off < 0 || t.new_off + t.m > new_total) return "the row's new beats inside the packed new beats";
    if (t.out_off < 0 || t.out_off + t.ne > out_total) return "the row's results inside the packed results";
    if (t.m > 0 && t.n0 + t.c < 1) return "no new beat in a stream without a sample";
    const long long n = t.nb + t.m;
    if (t.ne == 0) return nullptr;
    if (t.e0 + t.ne != n) return "results up to the stream's last beat: e0 + ne = nb + m";
    if (t.e0 != t.nb && !(t.e0 == 0 && t.nb <= RH_K)) return "e0 = nb, or e0 = 0 while the first K beats wait (nb <= K)";
    if (t.T < 0 && n < RH_K + 1) return "beats that are final: nb + m >= K + 1, or the stream ends";
    return nullptr;
  };
  return slots_walk(tab, rows, cap, x_total, rules, in_range, SlotNoRule{}, own, bad);
}

}  // namespace

// the caller's geometry as the refusals print it
static void rhythm_geom_text(const ral_rhythm_geom* g, char* buf, size_t n) {
  if (g) snprintf(buf, n, "Wb=%d Sa=%d c0=%g r0=%g", g->wb, g->sa, g->c0, g->r0);
  else snprintf(buf, n, "no geometry");
}

extern "C" int64_t ral_rhythm_pool_scratch_bytes(int64_t beats, int leads, const ral_rhythm_geom* geom) {
  RhythmGeom g;
  const char* why = rhythm_geom(leads, geom, g);
  if (!why && (beats < 0 || beats > (1LL << 31))) why = "0 <= beats <= 2^31";
  if (why) {
    char gt[96];
    rhythm_geom_text(geom, gt, sizeof(gt));
    return ral_fail("rhythm_pool_scratch_bytes: need %s (beats=%lld leads=%d %s)", why, (long long)beats, leads, gt);
  }
  return (beats > 0 ? beats : 1) * g.leads * g.We * 4;
}

extern "C" int ral_rhythm_records(const float* x, int64_t R, int leads, int64_t T, const ral_rhythm_geom* geom, const int32_t* peaks,
                                  const int32_t* count, int64_t cap, int32_t* label, float* corr, float* rr_ratio, ral_stream s) {
  if (!x || !geom || !peaks || !count || !label || !corr || !rr_ratio) return ral_fail("rhythm_records: null pointer");
  RhythmGeom g;
  const char* why = rhythm_geom(leads, geom, g);
  if (!why && (R < 1 || R > 65535 || T < 1 || T > 0x7fffffffLL)) why = "1 <= R <= 65535 and 1 <= T < 2^31";
  if (!why && (cap < 1 || cap > 0x7fffffffLL)) why = "1 <= cap < 2^31";
  if (why) {
    char gt[96];
    rhythm_geom_text(geom, gt, sizeof(gt));
    return ral_fail("rhythm_records: need %s (R=%lld leads=%d T=%lld cap=%lld %s)", why, (long long)R, leads, (long long)T,
                (long long)cap, gt);
  }
  k_rhythm_records<<<dim3((unsigned)cap, (unsigned)R), RH_WAVE, rhythm_lds_bytes(g), (hipStream_t)s>>>(x, T, g, peaks, count, cap, label,
                                                                                                     corr, rr_ratio);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_rhythm_pool(const float* hist, const float* x, int64_t x_total, const ral_rhythm_row* table, int rows,
                               ral_rhythm_row* table_dev, int upload, int64_t capacity, int leads, const ral_rhythm_geom* geom,
                               int hist_len, float* ring, int64_t* ring_pos, const int64_t* new_pos, int64_t new_total, void* scratch,
                               int64_t scratch_bytes, int64_t* out_pos, int32_t* label, float* corr, float* rr_ratio,
                               int64_t out_total, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !geom || !ring || !ring_pos || !new_pos || !scratch || !out_pos || !label || !corr ||
      !rr_ratio)
    return ral_fail("rhythm_pool: null pointer");
  hipStream_t st = (hipStream_t)s;
  RhythmGeom g;
  int bad = -1;
  const char* why = rhythm_geom(leads, geom, g);
  if (!why) why = rhythm_pool_fault(table, rows, capacity, g, hist_len, x_total, new_total, out_total, upload != 0, &bad);
  if (!why && (((uintptr_t)scratch & 3) || scratch_bytes < (new_total > 0 ? new_total : 1) * g.leads * g.We * 4))
    why = "a scratch of ral_rhythm_pool_scratch_bytes(new_total, leads, ...) bytes";
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, st) : 0;
  if (!rc) {
    long long m_max = 0, ne_max = 0;
    for (int r = 0; r < rows; ++r) {
      m_max = table[r].m > m_max ? table[r].m : m_max;
      ne_max = table[r].ne > ne_max ? table[r].ne : ne_max;
    }
    long long* rpos = (long long*)ring_pos;
    const long long* npos = (const long long*)new_pos;
    float* win = (float*)scratch;
    if (m_max > 0)
      k_rhythm_gather_pool<<<dim3((unsigned)m_max, (unsigned)rows), RH_WAVE, 0, st>>>(hist, x, table_dev, capacity, hist_len, g, npos, win);
    if (ne_max > 0)
      k_rhythm_classify_pool<<<dim3((unsigned)ne_max, (unsigned)rows), RH_WAVE, rhythm_lds_bytes(g), st>>>(
          table_dev, capacity, g, ring, rpos, npos, win, (long long*)out_pos, label, corr, rr_ratio);
    if (m_max > 0) k_rhythm_keep_pool<<<dim3(RH_K, (unsigned)rows), RH_WAVE, 0, st>>>(table_dev, g, ring, rpos, npos, win);
  }
  char gt[96] = "";
  if (rc) rhythm_geom_text(geom, gt, sizeof(gt));
  return table_done("rhythm_pool", rc, why, bad, "rows=%d capacity=%lld leads=%d hist_len=%d x_total=%lld new_total=%lld "
                    "out_total=%lld scratch_bytes=%lld %s", rows, (long long)capacity, leads, hist_len, (long long)x_total,
                    (long long)new_total, (long long)out_total, (long long)scratch_bytes, gt);
}
