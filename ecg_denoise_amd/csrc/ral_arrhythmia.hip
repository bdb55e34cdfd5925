// Rhythm findings of classified, delineated beats, window by window (ral_arrhythmia_windows; host side: arrhythmia.py).
//
// include/ralenet.h has the definition.  Everything a window yields is an integer count or an exact 64-bit integer sum, so the
// order of every reduction is free: threads count in registers, waves add with shuffles, and the block adds with LDS integer
// atomics.  The five statistics are formed once, by thread 0, in fp64 from those integers and rounded once; the flags are decided
// from the rounded values.  There is no floating-point sum anywhere.
//
// One workgroup of 256 threads per table row:
//   locate     two binary searches in the ascending list: the members [lo, hi) of the window
//   sweep      thread t takes the members lo + t, lo + t + 256, ...; a member reads its own position and label and those of the
//              three beats in front of it (the list is re-read through L1 / L2: the members of a window are a few hundred bytes),
//              and decides pause, accepted interval, difference and Lorenz point on its own.  A Lorenz point sets one bit of a
//              (2G + 1)^2 bitmap in LDS (atomicOr); a found P wave adds one to bin pr of a histogram over 1 .. prmax in LDS
//              (atomicAdd).  The longest ventricular run comes from an inclusive max-scan of "the last member at or before me
//              that is not V" (wave shuffles, wave totals in LDS, a carry from chunk to chunk): a V member's run ends at it with
//              length i - that index.
//   median     every thread adds a contiguous strip of the histogram, an exclusive block scan of the strips finds the one that
//              holds rank (n - 1) / 2, and its thread walks it; then the bins within lock_n of the median are added
//   cells      the bitmap's words are popcounted
// Nothing depends on the members being sparse: a window holds up to W of them and the sweep takes them 256 at a time.  No
// scratch memory, no global atomics, no memset; LDS: 4 (prmax + 1) + 4 ceil((2G + 1)^2 / 32) bytes, at most 34 KB, plus 80 bytes static.
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_slots.hpp"
#include <math.h>
#include <stdint.h>

namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_WAVE = 64;
constexpr int AR_WAVES = AR_THREADS / AR_WAVE;
constexpr int AR_MAX_M = 4096;       // the bound of ral_hrv_windows on (W - 1) // lo_n, kept so that both take the same windows
constexpr int AR_MAX_G = 64;
constexpr int AR_MAX_PR = 8192;      // bins of the PR histogram at most: 32 KB of LDS

// the block's integer accumulators in LDS
enum { A_NV, A_PAUSES, A_M, A_K, A_K2, A_ORIGIN, A_PMEAS, A_PFOUND, A_PLOCKED, A_NEC, A_VRUN, A_MED, A_N };

struct ArrGeom {
  int W, lo_n, hi_n, bin, G, lock_n, prmax, pause_n, min_m, vrun_min;
  int side, words;                     // 2G + 1, and the 32-bit words of the bitmap
  float n0, c0, pl0, tachy, brady;
  double fs;
};

typedef ral_hrv_row ArrRow;

// the first index in [0, n) whose position is >= v (n if none)
RAL_DEV int arr_lower(const int* __restrict__ p, int n, long long v) {
  int a = 0, b = n;
  while (a < b) {
    const int mid = a + ((b - a) >> 1);
    if ((long long)p[mid] < v) a = mid + 1; else b = mid;
  }
  return a;
}

RAL_DEV int arr_wave_sum(int v) {
#pragma unroll
  for (int o = AR_WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o, AR_WAVE);
  return v;
}

RAL_DEV long long arr_wave_sum(long long v) {
#pragma unroll
  for (int o = AR_WAVE / 2; o; o >>= 1) v += __shfl_xor(v, o, AR_WAVE);
  return v;
}

// cell(D) = clamp(floor((2 D + bin) / (2 bin)), -G, G), floor towards minus infinity
RAL_DEV int arr_cell(int D, int bin, int G) {
  const long long a = 2LL * D + bin, b = 2LL * bin;
  long long q = a / b;
  if (a % b < 0) --q;
  return (int)(q < -G ? -G : (q > G ? G : q));
}

// One block-wide inclusive scan step over the 256 threads: `x` is this thread's value, op is max (IS_MAX) or plus.  -> the
// inclusive result; *total receives the result over all 256.  tmp: AR_WAVES ints of LDS, free again when the call returns.
template <bool IS_MAX>
RAL_DEV int arr_block_scan(int x, int identity, int* tmp, int* total) {
  const int lane = threadIdx.x & (AR_WAVE - 1), wave = threadIdx.x / AR_WAVE;
#pragma unroll
  for (int o = 1; o < AR_WAVE; o <<= 1) {
    const int t = __shfl_up(x, o, AR_WAVE);
    if (lane >= o) x = IS_MAX ? (t > x ? t : x) : x + t;
  }
  if (lane == AR_WAVE - 1) tmp[wave] = x;
  __syncthreads();
  int before = identity, all = identity;
#pragma unroll
  for (int w = 0; w < AR_WAVES; ++w) {
    const int t = tmp[w];
    if (w < wave) before = IS_MAX ? (t > before ? t : before) : before + t;
    all = IS_MAX ? (t > all ? t : all) : all + t;
  }
  __syncthreads();
  *total = all;
  return IS_MAX ? (before > x ? before : x) : before + x;
}

// grid (rows): table row blockIdx.x
__global__ __launch_bounds__(AR_THREADS) void k_arrhythmia_windows(const int* __restrict__ peaks, const int* __restrict__ label,
                                                                   const int* __restrict__ count, const int* __restrict__ on,
                                                                   const int* __restrict__ ppeak, long long cap,
                                                                   const ArrRow* __restrict__ tab, ArrGeom g,
                                                                   int* __restrict__ counts, float* __restrict__ stats,
                                                                   int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) int arr_smem[];
  __shared__ int s_acc[A_N];
  __shared__ unsigned long long s_sum[2];      // S1, D2
  __shared__ int s_tmp[AR_WAVES];
  int* hist = arr_smem;                        // bins 0 .. prmax (bin 0 stays empty)
  unsigned* bits = reinterpret_cast<unsigned*>(arr_smem + g.prmax + 1);
  const int tid = threadIdx.x, lane = tid & (AR_WAVE - 1);

  const ArrRow t = tab[blockIdx.x];
  long long nn = count[t.rec];
  nn = nn < 0 ? 0 : (nn > cap ? cap : nn);
  const int n = (int)nn;
  const size_t o = (size_t)t.rec * (size_t)cap;
  const int* __restrict__ pos = peaks + o;
  const int* __restrict__ lab = label ? label + o : nullptr;
  const int* __restrict__ qon = on ? on + o : nullptr;
  const int* __restrict__ pk = ppeak ? ppeak + o : nullptr;

  for (int e = tid; e <= g.prmax; e += AR_THREADS) hist[e] = 0;
  for (int e = tid; e < g.words; e += AR_THREADS) bits[e] = 0u;
  if (tid < A_N) s_acc[tid] = 0;
  if (tid < 2) s_sum[tid] = 0ULL;
  __syncthreads();

  const int lo = arr_lower(pos, n, t.w0), hi = arr_lower(pos, n, t.w1);
  int nv = 0, pauses = 0, m = 0, k = 0, k2 = 0, origin = 0, pmeas = 0, pfound = 0, vrun = 0;
  long long s1 = 0, d2 = 0;
  int carry = lo - 1;                          // the last member so far that is not V; lo - 1: none
  for (long long base = lo; base < hi; base += AR_THREADS) {      // (64 bits: hi may lie within 256 of 2^31)
    const bool in = base + tid < hi;
    const int i = in ? (int)(base + tid) : lo;
    bool v = false;
    if (in) {
      // the labels and intervals of beats i - 3 .. i, as far as they are members
      const int back = i - lo < 3 ? i - lo : 3;
      int p[4], l[4];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const bool have = b <= back;
        p[b] = have ? pos[i - b] : 0;
        l[b] = have && lab ? lab[i - b] : 0;
      }
      v = l[0] == 1;
      nv += v;
      int d[3];
      bool acc[3];
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        d[b] = p[b] - p[b + 1];
        acc[b] = b < back && l[b] != 1 && l[b + 1] != 1 && d[b] >= g.lo_n && d[b] <= g.hi_n;
      }
      if (back >= 1 && d[0] > g.pause_n) ++pauses;
      if (acc[0]) {
        ++m;
        s1 += d[0];
        if (acc[1]) {
          const int D = d[0] - d[1];
          ++k;
          d2 += (long long)D * D;
          if (acc[2]) {
            const int cx = arr_cell(d[1] - d[2], g.bin, g.G), cy = arr_cell(D, g.bin, g.G);
            const int cell = (cx + g.G) * g.side + (cy + g.G);
            ++k2;
            origin += cx == 0 && cy == 0;
            atomicOr(&bits[cell >> 5], 1u << (cell & 31));
          }
        }
      }
      if (qon && !v) {
        const int q = qon[i];
        if (q >= 0) {
          ++pmeas;
          const int pp = pk[i];
          const long long pr = (long long)q - (long long)pp;
          if (pp >= 0 && pr >= 1 && pr <= g.prmax) {
            ++pfound;
            atomicAdd(&hist[(int)pr], 1);
          }
        }
      }
    }
    int all;
    const int last = arr_block_scan<true>(in && !v ? i : lo - 1, lo - 1, s_tmp, &all);
    const int brk = last > carry ? last : carry;
    if (in && v && i - brk > vrun) vrun = i - brk;
    carry = all > carry ? all : carry;
  }
  {
    const int v[8] = {nv, pauses, m, k, k2, origin, pmeas, pfound};
    const int at[8] = {A_NV, A_PAUSES, A_M, A_K, A_K2, A_ORIGIN, A_PMEAS, A_PFOUND};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int w = arr_wave_sum(v[e]);
      if (lane == 0 && w) atomicAdd(&s_acc[at[e]], w);
    }
    const long long a = arr_wave_sum(s1), b = arr_wave_sum(d2);
    if (lane == 0) {
      if (a) atomicAdd(&s_sum[0], (unsigned long long)a);
      if (b) atomicAdd(&s_sum[1], (unsigned long long)b);
    }
    if (vrun) atomicMax(&s_acc[A_VRUN], vrun);
  }
  __syncthreads();

  // the lower median of the PR histogram: rank (n - 1) / 2, counted from 0
  const int found = s_acc[A_PFOUND];
  {
    const int strip = (g.prmax + AR_THREADS - 1) / AR_THREADS;
    const int b0 = 1 + tid * strip, b1 = b0 + strip - 1 < g.prmax ? b0 + strip - 1 : g.prmax;
    int mine = 0;
    for (int e = b0; e <= b1; ++e) mine += hist[e];
    int all;
    const int incl = arr_block_scan<false>(mine, 0, s_tmp, &all);
    const int rank = (found - 1) / 2;                     // (found == 0: no thread holds it, A_MED is set below)
    if (found > 0 && incl - mine <= rank && rank < incl) {
      int c = incl - mine, e = b0;
      for (; e <= b1; ++e) {
        c += hist[e];
        if (c > rank) break;
      }
      s_acc[A_MED] = e;
    }
    if (found == 0 && tid == 0) s_acc[A_MED] = -1;
  }
  __syncthreads();
  const int med = s_acc[A_MED];
  if (med >= 1) {
    const long long a = (long long)med - g.lock_n, b = (long long)med + g.lock_n;
    const int e0 = (int)(a < 1 ? 1 : a), e1 = (int)(b > g.prmax ? g.prmax : b);
    int c = 0;
    for (int e = e0 + tid; e <= e1; e += AR_THREADS) c += hist[e];
    if (c) atomicAdd(&s_acc[A_PLOCKED], c);
  }
  {
    int c = 0;
    for (int e = tid; e < g.words; e += AR_THREADS) c += __popc(bits[e]);
    if (c) atomicAdd(&s_acc[A_NEC], c);
  }
  __syncthreads();

  if (tid == 0) {
    const size_t row = blockIdx.x;
    int* c = counts + row * 13;
    float* st = stats + row * 5;
    const int M = s_acc[A_M], K = s_acc[A_K], K2 = s_acc[A_K2], nec = s_acc[A_NEC], pm = s_acc[A_PMEAS], pl = s_acc[A_PLOCKED];
    const int np = s_acc[A_PAUSES], vr = s_acc[A_VRUN];
    c[0] = hi - lo, c[1] = M, c[2] = K, c[3] = K2, c[4] = nec, c[5] = s_acc[A_ORIGIN], c[6] = pm, c[7] = found, c[8] = pl;
    c[9] = med, c[10] = np, c[11] = s_acc[A_NV], c[12] = vr;
    const float fnan = nanf("");
    const double dm = (double)M, dS1 = (double)s_sum[0], dD2 = (double)s_sum[1];
    const float mean_rr = M >= 1 ? (float)(dS1 / (dm * g.fs)) : fnan;
    const float hr = M >= 1 ? (float)(60.0 * dm * g.fs / dS1) : fnan;
    const float nrmssd = K >= 1 ? (float)(sqrt(dD2 / (double)K) / (dS1 / dm)) : fnan;
    const float nec_ratio = K2 >= 1 ? (float)((double)nec / (double)K2) : fnan;
    const float p_share = pm >= 1 ? (float)((double)pl / (double)pm) : fnan;
    st[0] = mean_rr, st[1] = hr, st[2] = nrmssd, st[3] = nec_ratio, st[4] = p_share;
    const bool irregular = M >= g.min_m && K2 >= 1 && nrmssd >= g.n0 && nec_ratio >= g.c0;
    int f = 0;
    if (irregular) f |= RAL_ARR_IRREGULAR;
    if (irregular && !(p_share >= g.pl0)) f |= RAL_ARR_AF;
    if (M >= 1 && hr > g.tachy) f |= RAL_ARR_TACHY;
    if (M >= 1 && hr < g.brady) f |= RAL_ARR_BRADY;
    if (np >= 1) f |= RAL_ARR_PAUSE;
    if (vr >= g.vrun_min) f |= RAL_ARR_VRUN;
    flags[row] = f;
  }
}

const char* arr_geom(const ral_arrhythmia_geom* p, ArrGeom& g) {
  if (p->W < 2) return "2 <= W < 2^31";
  if (p->lo_n < 1 || p->hi_n < p->lo_n) return "1 <= lo_n <= hi_n";
  if ((p->W - 1) / p->lo_n > AR_MAX_M) return "max_m = (W - 1) // lo_n <= 4096";
  if (p->bin < 1) return "1 <= bin";
  if (p->G < 1 || p->G > AR_MAX_G) return "1 <= G <= 64";
  if (p->lock_n < 0) return "0 <= lock_n";
  if (p->prmax < 1 || p->prmax > AR_MAX_PR) return "1 <= prmax <= 8192";
  if (p->pause_n < 1) return "1 <= pause_n";
  if (p->min_m < 2) return "2 <= min_m";
  if (p->vrun_min < 1) return "1 <= vrun_min";
  if (!isfinite(p->n0) || !isfinite(p->c0) || !isfinite(p->pl0) || !isfinite(p->tachy) || !isfinite(p->brady))
    return "finite limits n0, c0, pl0, tachy, brady";
  if (!(p->fs > 0.0) || !isfinite(p->fs)) return "a finite fs > 0";
  g.W = p->W, g.lo_n = p->lo_n, g.hi_n = p->hi_n, g.bin = p->bin, g.G = p->G, g.lock_n = p->lock_n, g.prmax = p->prmax;
  g.pause_n = p->pause_n, g.min_m = p->min_m, g.vrun_min = p->vrun_min;
  g.side = 2 * p->G + 1;
  g.words = (g.side * g.side + 31) / 32;
  g.n0 = p->n0, g.c0 = p->c0, g.pl0 = p->pl0, g.tachy = p->tachy, g.brady = p->brady, g.fs = p->fs;
  return nullptr;
}

}  // namespace

// the rule a call breaks (*bad: the table row that breaks it, or -1), or null; the table is read only when it is uploaded
static const char* arr_fault(long long R, long long cap, const ral_hrv_row* tab, long long rows, int upload,
                             const ral_arrhythmia_geom* geom, ArrGeom& g, long long* bad) {
  *bad = -1;
  if (R < 1 || R > 65535) return "1 <= R <= 65535";
  if (cap < 1 || cap > 0x7fffffffLL) return "1 <= cap < 2^31";
  if (const char* why = arr_geom(geom, g)) return why;
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

extern "C" int ral_arrhythmia_windows(const int32_t* peaks, const int32_t* label_or_null, const int32_t* count,
                                      const int32_t* on_or_null, const int32_t* ppeak_or_null, int64_t R, int64_t cap,
                                      const ral_hrv_row* table, int64_t rows, ral_hrv_row* table_dev, int upload,
                                      const ral_arrhythmia_geom* geom, int32_t* counts, float* stats, int32_t* flags, ral_stream s) {
  static const char NAME[] = "ral_arrhythmia_windows";
  // (the host table is read only when it is uploaded: without upload NAME stands in for it as something non-null)
  const struct { const void* p; const char* name; } need[] = {{peaks, "peaks"}, {count, "count"}, {table_dev, "table_dev"},
      {upload ? (const void*)table : (const void*)NAME, "table"}, {geom, "geom"}, {counts, "counts"}, {stats, "stats"}, {flags, "flags"}};
  for (const auto& a : need)
    if (!a.p) return ral_fail("%s: need a non-null %s", NAME, a.name);
  if (!on_or_null != !ppeak_or_null)
    return ral_fail("%s: need on and ppeak together or neither (%s is null)", NAME, on_or_null ? "ppeak" : "on");
  ArrGeom g;
  long long bad = -1;
  const char* why = arr_fault(R, cap, table, rows, upload, geom, g, &bad);
  const int rc = why ? -1 : (upload && rows > 0) ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc && rows > 0) {
    const size_t lds = ((size_t)g.prmax + 1 + (size_t)g.words) * 4;
    k_arrhythmia_windows<<<dim3((unsigned)rows), AR_THREADS, lds, (hipStream_t)s>>>(peaks, label_or_null, count, on_or_null, ppeak_or_null,
                                                                                  cap, table_dev, g, counts, stats, flags);
  }
  return table_done(NAME, rc, why, bad, "R=%lld cap=%lld rows=%lld W=%d lo_n=%d hi_n=%d bin=%d G=%d lock_n=%d prmax=%d pause_n=%d "
                    "min_m=%d vrun_min=%d n0=%g c0=%g pl0=%g tachy=%g brady=%g fs=%g", (long long)R, (long long)cap, (long long)rows,
                    geom->W, geom->lo_n, geom->hi_n, geom->bin, geom->G, geom->lock_n, geom->prmax, geom->pause_n, geom->min_m,
                    geom->vrun_min, geom->n0, geom->c0, geom->pl0, geom->tachy, geom->brady, geom->fs);
}
