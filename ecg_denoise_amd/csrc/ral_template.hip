// Median beats of records, window by window (ral_template_records; host side: template.py).
//
// The definition (include/ralenet.h has it): the members of window w = [w H, min(w H + W, T)) of a record are, in list order, its
// beats p with w0 <= p < w1, label 0 where labels are given, and p - Wpre >= 0, p + Wpost <= T - 1; the first used = min(total,
// kmax) of them are measured.  tpl[l][k] is the median over them of x_l[p - Wpre + k] (an even count: (a + b) * 0.5f of the two
// middle values, an addition and then a product, so nothing contracts), and rr the lower median of p_i - p_{i-1} over the used
// beats with i >= 1.
//
// One workgroup per (window, record, span of TP_SPAN tiles of TP_TILE consecutive template samples).  It finds the first beat at
// or behind w0 by a search in which every thread probes the end of one segment of the list (two rounds for 65 536 beats), then
// tests the beats from there on TP_THREADS at a time, until one lies at or behind w1, and compacts those that pass in list
// order with a ballot prefix (no atomic counter); a position that fails the test is no member, so every read below stays inside
// the record whatever the list holds.  Per tile and lead it stages used x tile floats into LDS (a member's run of the tile is
// contiguous in the record: half a wave reads one row) and takes each column's median by rank counting: with lt values of the
// column smaller than a member's and le smaller or equal, that value holds the sorted places [lt, le), so the members whose
// [lt, le) holds the middle place all carry the middle value, and each of them stores it (a zero as +0.0).  The leads are
// staged one at a time - or, where used is small, as many together as fit the same TP_KMAX rows, so that their reads are in
// flight together - so their number is not limited by LDS.  Nothing depends on the grid.
//
// Launch: one, grid (nw, R, ceil(Wn / (TP_SPAN TP_TILE))), TP_THREADS threads; no scratch buffer, no memset, no atomics.
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include <stdint.h>

namespace {

constexpr int TP_WAVE = 64;
constexpr int TP_THREADS = 256;
constexpr int TP_WAVES = TP_THREADS / TP_WAVE;
constexpr int TP_TILE = 32;                     // template samples per tile: TP_KMAX x TP_TILE floats are 32 KB of LDS
constexpr int TP_SPAN = 4;                      // tiles per workgroup, which finds its members once for all of them
constexpr int TP_ROWS = TP_THREADS / TP_TILE;   // rows (a member of a lead each) staged and ranked per pass
constexpr int TP_KMAX = 256;
constexpr int TP_BATCH = 8;                     // rows a thread reads from the record before it stores the first
constexpr int TP_GROUP = 16;                    // the most leads staged together (where the members are few enough)

struct TplGeom {
  int leads, wpre, wpost, wn, kmax;
  long long w, h;
};

// how many threads of the workgroup raise `flag` (the same in every thread), and in `before` how many of them precede this one;
// two barriers, so `wsum` may be used again at once
RAL_DEV int tpl_count(bool flag, int* wsum, int lane, int wave, int& before) {
  const unsigned long long vote = __ballot(flag);
  if (lane == 0) wsum[wave] = __popcll(vote);
  __syncthreads();
  int all = 0;
  before = __popcll(vote & ((1ull << lane) - 1));
  for (int v = 0; v < TP_WAVES; ++v) {
    if (v < wave) before += wsum[v];
    all += wsum[v];
  }
  __syncthreads();
  return all;
}

// grid (nw, R, spans): window blockIdx.x of record blockIdx.y, template samples [blockIdx.z TP_SPAN TP_TILE, + TP_SPAN TP_TILE)
__global__ __launch_bounds__(TP_THREADS) void k_template_records(const float* __restrict__ x, long long T, TplGeom g,
                                                                 const int* __restrict__ peaks, const int* __restrict__ label,
                                                                 const int* __restrict__ count, long long cap, long long nw,
                                                                 float* __restrict__ tpl, int* __restrict__ used_out,
                                                                 int* __restrict__ total_out, int* __restrict__ rr_out) {
  __shared__ float vals[TP_KMAX * TP_TILE];
  __shared__ float mid[2][TP_GROUP][TP_TILE];
  __shared__ int start[TP_KMAX];               // p - Wpre of the used members, in list order
  __shared__ int diff[TP_KMAX];                // p_i - p_{i-1} of the used members
  __shared__ unsigned char has[TP_KMAX];       // i >= 1
  __shared__ int wsum[TP_WAVES];
  __shared__ int s_rr;
  const int tid = threadIdx.x, lane = tid & (TP_WAVE - 1), wave = tid / TP_WAVE;
  const long long w = blockIdx.x, r = blockIdx.y, o = r * cap;
  const long long w0 = w * g.h, w1 = w0 + g.w < T ? w0 + g.w : T;
  const int* const pr = peaks + o;
  long long n = count[r];
  n = n < 0 ? 0 : (n > cap ? cap : n);
  if (tid == 0) s_rr = -1;
  // the first index in [0, n) whose position is >= w0 (n: none).  The list is cut into TP_THREADS segments; on an ascending list
  // those that end below w0 are the first `below` of them, and the index sought lies in the next one.  On any other list the
  // loop still ends, at an index in [0, n]: the range shrinks every round.
  long long lo = 0, hi = n;
  while (lo < hi) {
    const long long step = (hi - lo + TP_THREADS - 1) / TP_THREADS, last = lo + (tid + 1) * step - 1;
    int before;
    const int below = tpl_count(last < hi && (long long)pr[last] < w0, wsum, lane, wave, before);
    lo += below * step;
    lo = lo < hi ? lo : hi;
    hi = lo + step - 1 < hi ? lo + step - 1 : hi;
  }
  // the members, from there on: the scan ends behind the first beats that lie at or behind w1
  int total = 0;
  for (long long base = lo; base < n; base += TP_THREADS) {
    const long long i = base + tid;
    bool ok = false, past = false;
    long long p = 0;
    if (i < n) {
      p = pr[i];
      past = p >= w1;
      ok = p >= w0 && p < w1 && p - g.wpre >= 0 && p + g.wpost <= T - 1 && (!label || label[o + i] == 0);
    }
    int slot, none;
    const int found = tpl_count(ok, wsum, lane, wave, slot);
    slot += total;
    if (ok && slot < g.kmax) {
      start[slot] = (int)(p - g.wpre);
      has[slot] = i >= 1;
      diff[slot] = i >= 1 ? (int)((unsigned)p - (unsigned)pr[i - 1]) : 0;
    }
    total += found;
    if (tpl_count(past, wsum, lane, wave, none)) break;
  }
  __syncthreads();
  const int used = total < g.kmax ? total : g.kmax;
  const long long ow = r * nw + w;
  if (blockIdx.z == 0) {
    if (tid < used && has[tid]) {              // (used <= TP_KMAX = TP_THREADS: a thread per member)
      int m = 0, rank = 0;
      const int d = diff[tid];
      for (int k = 0; k < used; ++k) {
        if (!has[k]) continue;
        ++m;
        rank += diff[k] < d || (diff[k] == d && k < tid);
      }
      if (rank == (m - 1) / 2) s_rr = d;
    }
    __syncthreads();
    if (tid == 0) used_out[ow] = used, total_out[ow] = total, rr_out[ow] = s_rr;
  }
  const int c = tid % TP_TILE, row = tid / TP_TILE;
  const int below = (used - 1) / 2, above = used / 2;      // the ranks of the two middle values (one rank when used is odd)
  int group = TP_KMAX / (used ? used : 1);                 // leads staged together: group x used rows fit the TP_KMAX of vals
  group = group < TP_GROUP ? group : TP_GROUP;
  group = group < g.leads ? group : g.leads;
  for (int ti = 0; ti < TP_SPAN; ++ti) {
    const int k0 = ((int)blockIdx.z * TP_SPAN + ti) * TP_TILE;
    if (k0 >= g.wn) break;
    const bool live = k0 + c < g.wn;
    for (int l0 = 0; l0 < g.leads; l0 += group) {
      const int nl = group < g.leads - l0 ? group : g.leads - l0, rows = nl * used;
      const float* const xl = x + ((size_t)r * g.leads + l0) * T + k0 + c;
      if (live)
        for (int e0 = row; e0 < rows; e0 += TP_BATCH * TP_ROWS) {      // row e: lead l0 + e / used, member e % used
          float v[TP_BATCH];                                           // (a batch of reads is in flight before the first is stored)
#pragma unroll
          for (int u = 0; u < TP_BATCH; ++u) {
            const int e = e0 + u * TP_ROWS, q = e < rows ? e / used : 0;
            v[u] = e < rows ? xl[(size_t)q * T + start[e - q * used]] : 0.f;
          }
#pragma unroll
          for (int u = 0; u < TP_BATCH; ++u) {
            const int e = e0 + u * TP_ROWS;
            if (e < rows) vals[e * TP_TILE + c] = v[u];
          }
        }
      __syncthreads();
      if (live)
        for (int e = row; e < rows; e += TP_ROWS) {
          const int q = e / used;
          const float* const col = vals + q * used * TP_TILE + c;
          const float v = col[(e - q * used) * TP_TILE];
          int lt = 0, le = 0;                              // how many values of the column are smaller, and smaller or equal
#pragma unroll 4
          for (int k = 0; k < used; ++k) {
            const float u = col[k * TP_TILE];
            lt += u < v;
            le += u <= v;
          }
          const float z = v == 0.f ? 0.f : v;              // (-0.0 -> +0.0: whichever of equal values is stored, the bits are the same)
          if (lt <= below && below < le) mid[0][q][c] = z;
          if (lt <= above && above < le) mid[1][q][c] = z;
        }
      __syncthreads();
      for (int e = tid; e < nl * TP_TILE; e += TP_THREADS) {
        const int q = e / TP_TILE, cc = e % TP_TILE;
        if (k0 + cc >= g.wn) continue;
        float m = 0.f;
        if (used) m = (used & 1) ? mid[0][q][cc] : (mid[0][q][cc] + mid[1][q][cc]) * 0.5f;
        tpl[((size_t)ow * g.leads + l0 + q) * g.wn + k0 + cc] = m;
      }
      __syncthreads();
    }
  }
}

}  // namespace

// the argument a call is refused for (geom is not null), or null
static const char* template_fault(long long R, int leads, long long T, const ral_template_geom* geom, long long cap, long long nw) {
  const int big = 1 << 19;      // (Wn <= 2^20 + 1: the spans fit a grid dimension)
  if (R < 1 || R > 65535) return "R must be in [1, 65535]";
  if (leads < 1 || leads > 65535) return "leads must be in [1, 65535]";
  if (T < 1 || T > 0x7fffffffLL) return "T must be in [1, 2^31)";
  if (cap < 1 || cap > 0x7fffffffLL) return "cap must be in [1, 2^31)";
  if (geom->wpre < 1 || geom->wpre > big) return "geom.wpre must be in [1, 2^19]";
  if (geom->wpost < 1 || geom->wpost > big) return "geom.wpost must be in [1, 2^19]";
  if (geom->w < 1) return "geom.w must be >= 1";
  if (geom->h < 1) return "geom.h must be >= 1";
  if (geom->kmax < 1 || geom->kmax > TP_KMAX) return "geom.kmax must be in [1, 256]";
  const long long rule = T < geom->w ? 1 : (T - geom->w) / geom->h + 1;
  if (nw != rule) return "nw must be max(1, (T - w) / h + 1), the number of windows of T samples";
  return nullptr;
}

extern "C" int ral_template_records(const float* x, int64_t R, int leads, int64_t T, const ral_template_geom* geom,
                                    const int32_t* peaks, const int32_t* label_or_null, const int32_t* count, int64_t cap, int64_t nw,
                                    float* tpl, int32_t* used, int32_t* total, int32_t* rr, ral_stream s) {
  const char* why = !x ? "x is NULL" : !geom ? "geom is NULL" : !peaks ? "peaks is NULL" : !count ? "count is NULL" :
                    !tpl ? "tpl is NULL" : !used ? "used is NULL" : !total ? "total is NULL" : !rr ? "rr is NULL" :
                    template_fault(R, leads, T, geom, cap, nw);
  if (why) {
    const ral_template_geom none = {0, 0, 0, 0, 0}, *g = geom ? geom : &none;
    return ral_fail("ral_template_records: %s (R=%lld leads=%d T=%lld cap=%lld nw=%lld wpre=%d wpost=%d w=%d h=%d kmax=%d)", why,
                    (long long)R, leads, (long long)T, (long long)cap, (long long)nw, g->wpre, g->wpost, g->w, g->h, g->kmax);
  }
  TplGeom g;
  g.leads = leads, g.wpre = geom->wpre, g.wpost = geom->wpost, g.wn = geom->wpre + geom->wpost + 1, g.kmax = geom->kmax;
  g.w = geom->w, g.h = geom->h;
  const unsigned spans = (unsigned)((g.wn + TP_SPAN * TP_TILE - 1) / (TP_SPAN * TP_TILE));
  k_template_records<<<dim3((unsigned)nw, (unsigned)R, spans), TP_THREADS, 0, (hipStream_t)s>>>(x, T, g, peaks, label_or_null, count, cap,
                                                                                              nw, tpl, used, total, rr);
  HIP_OK(hipGetLastError());
  return 0;
}
