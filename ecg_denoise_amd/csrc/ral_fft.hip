// FFT-threshold baseline (local_utils/denoisefunc.py:36-66 fft_denoise, scored as the model "fft" in test_cls.py:240-255):
//   X = fft(item);  mag = |X|;  cutoff = threshold * max(mag);  X[mag < cutoff] = 0;  out = ifft(X).real
// per GROUP: a 2-D input thresholds every row against its own maximum (rows_per_group = 1), a 3-D input (batch, leads, L) all
// leads of an item against one maximum (test_cls.py:246 calls it with (B, 2, 1000); numpy's fft runs along the last axis, the
// maximum over the whole item).  fp32 throughout, |X| = sqrtf(re^2 + im^2), no fused contraction anywhere in this file (the
// pragma below), so the magnitude of a bin is the same number wherever it is formed: the maximal bin compares equal to the
// maximum and survives threshold = 1.  The comparison is `<`: a bin at the cutoff is kept, an all-zero group stays zero.
//
// Two paths, one kernel body (fft_group) over a `path` object that knows three things: forward (a row -> its slot in LDS),
// scan (the bins of a slot: their maximum, or threshold them and count the survivors) and inverse (a slot -> a row).
//
// FFT path: L even, 5-smooth, 16 <= L <= 8192.  The row is packed as N = L / 2 complex numbers z[n] = x[2n] + i x[2n+1] and
//   transformed by a Stockham mixed-radix (4, 2, 3, 5) FFT that ping-pongs between the row's slot and one shared buffer; the
//   slot keeps Z = FFT_N(z), never the split spectrum.  The bins k and N - k of the real row's spectrum come from the pair
//   (Z[k], Z[N-k]) alone:  E = (Z[k] + conj Z[N-k]) / 2, O = -i (Z[k] - conj Z[N-k]) / 2, X[k] = E + w^k O,
//   X[N-k] = conj(E - w^k O), w = exp(-2 pi i / L), so split, threshold and merge are one in-place pass over the pairs.  The
//   merge writes conj(Z'), the same forward butterflies run again and the result is conjugated and scaled by 1 / N on the way
//   out.  Twiddles: exp(-2 pi i t / N) and w^k as two LDS tables built per workgroup with sincospi in fp64 from the integer
//   ratio, rounded once to fp32.
//   LDS bytes: 8 N (table) + 4 N + 8 (w^k) + 8 N (shared buffer) + 8 N per resident row.
//   The butterfly passes read with unit stride; their writes have stride Ns (the product of the radices already done), which is
//   a 4-way bank conflict of the 8-byte stores in the passes with 4 <= Ns < 64 when Ns is a power of two.  Left as it is: the
//   padding that removes it costs a quarter more LDS, which the 2 x 8192 group does not have.
// Direct path: every other L in [2, 1024] (odd lengths, 112, 1008, ...).  An O(L^2) DFT: the row and the table
//   exp(-2 pi i t / L) in LDS, bin k of sample n uses entry (k n) mod L kept as a running integer, sums in blocks of 32 terms.
//   Bins 0 .. L / 2 are kept per row.  It is short and slow (about L / log2 L times the work of the FFT path) and exists so
//   that every window length the models take has the baseline.
//   LDS bytes: 4 L (row) + 8 L (table) + 8 (L / 2 + 1) per resident row.
//
// Groups.  mode 0: one workgroup per group, all its rows resident, when that fits FFT_LDS_BUDGET (2 x 8192 and 12 x 1024 do):
//   a sample is read once and written once.  Otherwise two launches of one workgroup per row: mode 1 transforms and writes the
//   row's maximum to scratch, mode 2 transforms again, takes the group's maximum from scratch, thresholds and inverts
//   (recomputing the transform is cheaper than a round trip of the spectrum through HBM; the same code on the same input gives
//   the same bits).  The kept count of a group is summed with an integer atomicAdd there; there is no floating-point atomic.
// x == y is allowed: a workgroup has read every row it owns before it writes the first.
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include <stdint.h>

#pragma clang fp contract(off)

namespace {

constexpr int FFT_THREADS = 256;
constexpr int FFT_MAX_PASSES = 12;                 // N <= 4096: at most 7 (3^7 = 2187)
constexpr long long FFT_LDS_BUDGET = 152 * 1024;   // of the 160 KB of a CU; the rest covers the static words and alignment
constexpr int FFT_MIN_L = 16, FFT_MAX_L = 8192, DIRECT_MAX_L = 1024;

struct FftPlan {
  int L, N;                       // N = L / 2 on the FFT path, unused on the direct path
  int npass, radix[FFT_MAX_PASSES];
};

struct FftArgs {
  const float* x;
  float* y;
  int32_t* kept;                  // null: not wanted
  float* rowmax;                  // scratch of modes 1 and 2
  int rpg;                        // rows per group
  int mode;
  float thr;
  FftPlan plan;
};

struct ScanOut { float mx; int cnt; };

RAL_DEV float2 cmul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
RAL_DEV float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
RAL_DEV float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
RAL_DEV float2 cmuli_neg(float2 a) { return make_float2(a.y, -a.x); }     // -i a
RAL_DEV float cmag(float2 a) { return sqrtf(a.x * a.x + a.y * a.y); }

// exp(-2 pi i num / den), 0 <= num < den: fp64 sincospi of the exact ratio, rounded once
RAL_DEV float2 unit_root(int num, int den) {
  double s, c;
  sincospi(2.0 * (double)num / (double)den, &s, &c);
  return make_float2((float)c, (float)-s);
}

// ---------------------------------------------------------------- the FFT path
struct FftPath {
  const FftPlan& P;
  float2 *tw, *wl, *T, *slots;

  __device__ FftPath(const FftPlan& plan, float* sm) : P(plan) {
    const int N = P.N;
    tw = reinterpret_cast<float2*>(sm);
    T = tw + N;
    slots = T + N;                       // (the w^k table goes last: its length is odd)
  }
  __device__ void tables(int rows) {
    const int N = P.N;
    wl = slots + (size_t)rows * N;
    for (int t = threadIdx.x; t < N; t += FFT_THREADS) tw[t] = unit_root(t, N);
    for (int k = threadIdx.x; k <= N / 2; k += FFT_THREADS) wl[k] = unit_root(k, P.L);
  }

  // Stockham passes src -> dst -> src ...; the result is in src when npass is even, in dst when it is odd
  __device__ void passes(float2* src, float2* dst) const {
    const int N = P.N;
    int Ns = 1;
    for (int p = 0; p < P.npass; ++p) {
      const int R = P.radix[p], M = N / R, stride = N / (Ns * R);
      for (int j = threadIdx.x; j < M; j += FFT_THREADS) {
        const int q = j / Ns, k = j - q * Ns;
        float2* o = dst + (q * Ns * R + k);
        const int t1 = k * stride;                       // k r stride < N for r < R
        const float2 a = src[j];
        if (R == 4) {
          const float2 b = cmul(src[j + M], tw[t1]), c = cmul(src[j + 2 * M], tw[2 * t1]), d = cmul(src[j + 3 * M], tw[3 * t1]);
          const float2 t0 = cadd(a, c), t1_ = csub(a, c), t2 = cadd(b, d), t3 = cmuli_neg(csub(b, d));
          o[0] = cadd(t0, t2); o[Ns] = cadd(t1_, t3); o[2 * Ns] = csub(t0, t2); o[3 * Ns] = csub(t1_, t3);
        } else if (R == 2) {
          const float2 b = cmul(src[j + M], tw[t1]);
          o[0] = cadd(a, b); o[Ns] = csub(a, b);
        } else if (R == 3) {
          const float2 b = cmul(src[j + M], tw[t1]), c = cmul(src[j + 2 * M], tw[2 * t1]);
          const float s3 = 0.86602540378443864676f;
          const float2 t = cadd(b, c), d = csub(b, c);
          const float2 m = make_float2(a.x - 0.5f * t.x, a.y - 0.5f * t.y);
          const float2 u = make_float2(s3 * d.y, -s3 * d.x);
          o[0] = cadd(a, t); o[Ns] = cadd(m, u); o[2 * Ns] = csub(m, u);
        } else {   // 5
          const float2 b = cmul(src[j + M], tw[t1]), c = cmul(src[j + 2 * M], tw[2 * t1]), d = cmul(src[j + 3 * M], tw[3 * t1]),
                       e = cmul(src[j + 4 * M], tw[4 * t1]);
          const float c1 = 0.30901699437494742410f, c2 = -0.80901699437494742410f, s1 = 0.95105651629515357212f,
                      s2 = 0.58778525229247312917f;
          const float2 t1_ = cadd(b, e), t2 = cadd(c, d), t3 = csub(b, e), t4 = csub(c, d);
          const float2 m1 = make_float2(a.x + (c1 * t1_.x + c2 * t2.x), a.y + (c1 * t1_.y + c2 * t2.y));
          const float2 m2 = make_float2(a.x + (c2 * t1_.x + c1 * t2.x), a.y + (c2 * t1_.y + c1 * t2.y));
          const float2 n1 = cmuli_neg(make_float2(s1 * t3.x + s2 * t4.x, s1 * t3.y + s2 * t4.y));
          const float2 n2 = cmuli_neg(make_float2(s2 * t3.x - s1 * t4.x, s2 * t3.y - s1 * t4.y));
          o[0] = cadd(a, cadd(t1_, t2));
          o[Ns] = cadd(m1, n1); o[4 * Ns] = csub(m1, n1); o[2 * Ns] = cadd(m2, n2); o[3 * Ns] = csub(m2, n2);
        }
      }
      __syncthreads();
      float2* t = src; src = dst; dst = t;
      Ns *= R;
    }
  }

  // row -> Z in slot r
  __device__ void forward(const float* xrow, int r) const {
    const int N = P.N;
    float2* slot = slots + (size_t)r * N;
    float2* first = (P.npass & 1) ? T : slot;          // so that the result lands in the slot
    if ((((uintptr_t)xrow) & 15) == 0 && (N & 1) == 0) {
      const float4* g = reinterpret_cast<const float4*>(xrow);
      float4* d = reinterpret_cast<float4*>(first);
      for (int i = threadIdx.x; i < N / 2; i += FFT_THREADS) d[i] = g[i];
    } else {
      float* d = reinterpret_cast<float*>(first);
      for (int i = threadIdx.x; i < P.L; i += FFT_THREADS) d[i] = xrow[i];
    }
    __syncthreads();
    passes(first, first == slot ? T : slot);
  }

  // the bins of slot r.  apply = false: their maximum.  apply = true: zero those below the cutoff, count the survivors over the
  // full spectrum, and leave conj(Z') in the slot
  __device__ ScanOut scan(int r, float cutoff, bool apply) const {
    const int N = P.N;
    float2* Z = slots + (size_t)r * N;
    ScanOut out{0.f, 0};
    for (int k = threadIdx.x; k <= N / 2; k += FFT_THREADS) {
      const int kk = k ? N - k : 0;
      const float2 zk = Z[k], zn = Z[kk], w = wl[k];
      const float2 zc = make_float2(zn.x, -zn.y);
      const float2 E = make_float2(0.5f * (zk.x + zc.x), 0.5f * (zk.y + zc.y));
      const float2 D = make_float2(0.5f * (zk.x - zc.x), 0.5f * (zk.y - zc.y));
      const float2 WO = cmul(w, cmuli_neg(D));
      float2 xa = cadd(E, WO);                          // bin k
      float2 xb = csub(E, WO); xb.y = -xb.y;            // bin N - k
      const bool self = (k == kk) && k;                 // k = N / 2: one bin
      if (self) xb = xa;
      const float ma = cmag(xa), mb = cmag(xb);
      if (!apply) {
        out.mx = fmaxf(out.mx, fmaxf(ma, mb));
        continue;
      }
      const bool ka = !(ma < cutoff), kb = !(mb < cutoff);
      out.cnt += k == 0 ? (int)ka + (int)kb : (self ? 2 * (int)ka : 2 * ((int)ka + (int)kb));
      if (!ka) xa = make_float2(0.f, 0.f);
      if (!kb) xb = make_float2(0.f, 0.f);
      const float2 xbc = make_float2(xb.x, -xb.y);
      const float2 E2 = make_float2(0.5f * (xa.x + xbc.x), 0.5f * (xa.y + xbc.y));
      const float2 P2 = make_float2(0.5f * (xa.x - xbc.x), 0.5f * (xa.y - xbc.y));
      const float2 O2 = cmul(make_float2(w.x, -w.y), P2);
      // Z'[k] = E2 + i O2, Z'[N-k] = conj(E2) + i conj(O2); stored conjugated for the inverse
      Z[k] = make_float2(E2.x - O2.y, -(E2.y + O2.x));
      if (kk != k) Z[kk] = make_float2(E2.x + O2.y, -(O2.x - E2.y));
    }
    __syncthreads();
    return out;
  }

  // conj(Z') in slot r -> row
  __device__ void inverse(int r, float* yrow) const {
    const int N = P.N;
    float2* slot = slots + (size_t)r * N;
    passes(slot, T);
    const float2* res = (P.npass & 1) ? T : slot;
    const float sc = 1.0f / (float)N;
    if ((((uintptr_t)yrow) & 15) == 0 && (N & 1) == 0) {
      const float4* s4 = reinterpret_cast<const float4*>(res);
      float4* g = reinterpret_cast<float4*>(yrow);
      for (int i = threadIdx.x; i < N / 2; i += FFT_THREADS) {
        const float4 v = s4[i];
        g[i] = make_float4(v.x * sc, -v.y * sc, v.z * sc, -v.w * sc);
      }
    } else {
      const float* s1 = reinterpret_cast<const float*>(res);
      for (int i = threadIdx.x; i < P.L; i += FFT_THREADS) yrow[i] = (i & 1) ? -s1[i] * sc : s1[i] * sc;
    }
    __syncthreads();                                     // T is free again
  }
};

// ---------------------------------------------------------------- the direct path
struct DirectPath {
  const FftPlan& P;
  float* xs;
  float2 *tw, *slots;
  int H;                                                 // bins 0 .. H are kept

  __device__ DirectPath(const FftPlan& plan, float* sm) : P(plan) {
    const int L = P.L;
    H = L / 2;
    tw = reinterpret_cast<float2*>(sm);
    slots = tw + L;
  }
  __device__ void tables(int rows) {
    xs = reinterpret_cast<float*>(slots + (size_t)rows * (H + 1));
    for (int t = threadIdx.x; t < P.L; t += FFT_THREADS) tw[t] = unit_root(t, P.L);
  }
  RAL_DEV int weight(int k) const { return (k == 0 || 2 * k == P.L) ? 1 : 2; }   // bins k and L - k of the full spectrum

  __device__ void forward(const float* xrow, int r) const {
    const int L = P.L;
    float2* X = slots + (size_t)r * (H + 1);
    for (int i = threadIdx.x; i < L; i += FFT_THREADS) xs[i] = xrow[i];
    __syncthreads();
    for (int k = threadIdx.x; k <= H; k += FFT_THREADS) {
      float re = 0.f, im = 0.f;
      int idx = 0;                                       // (k n) mod L
      for (int n0 = 0; n0 < L; n0 += 32) {
        float br = 0.f, bi = 0.f;
        const int n1 = n0 + 32 < L ? n0 + 32 : L;
        for (int n = n0; n < n1; ++n) {
          const float v = xs[n];
          const float2 w = tw[idx];
          br = fmaf(v, w.x, br); bi = fmaf(v, w.y, bi);
          idx += k; idx -= idx >= L ? L : 0;
        }
        re += br; im += bi;
      }
      X[k] = make_float2(re, im);
    }
    __syncthreads();
  }

  __device__ ScanOut scan(int r, float cutoff, bool apply) const {
    float2* X = slots + (size_t)r * (H + 1);
    ScanOut out{0.f, 0};
    for (int k = threadIdx.x; k <= H; k += FFT_THREADS) {
      const float m = cmag(X[k]);
      if (!apply) { out.mx = fmaxf(out.mx, m); continue; }
      if (m < cutoff) X[k] = make_float2(0.f, 0.f);
      else out.cnt += weight(k);
    }
    __syncthreads();
    return out;
  }

  __device__ void inverse(int r, float* yrow) const {
    const int L = P.L;
    const float2* X = slots + (size_t)r * (H + 1);
    const float sc = 1.0f / (float)L;
    for (int n = threadIdx.x; n < L; n += FFT_THREADS) {
      float acc = 0.f;
      int idx = 0;                                       // (k n) mod L
      for (int k0 = 0; k0 <= H; k0 += 32) {
        float b = 0.f;
        const int k1 = k0 + 32 <= H ? k0 + 32 : H + 1;
        for (int k = k0; k < k1; ++k) {
          const float2 v = X[k], w = tw[idx];
          b = fmaf((float)weight(k), fmaf(v.x, w.x, v.y * w.y), b);      // Re(X[k] exp(+2 pi i k n / L)), twice for k and L - k
          idx += n; idx -= idx >= L ? L : 0;
        }
        acc += b;
      }
      yrow[n] = acc * sc;
    }
    __syncthreads();
  }
};

// ---------------------------------------------------------------- one body for both
template <class Path>
RAL_DEV void fft_group(const FftArgs& a, float* sm, float* red_f, int* red_i) {
  const int tid = threadIdx.x, L = a.plan.L;
  const int rows = a.mode == 0 ? a.rpg : 1;
  const long long row0 = (long long)blockIdx.x * rows;
  Path p(a.plan, sm);
  p.tables(rows);
  __syncthreads();
  float mx = 0.f;
  for (int r = 0; r < rows; ++r) {
    p.forward(a.x + (row0 + r) * L, r);
    if (a.mode != 2) mx = fmaxf(mx, p.scan(r, 0.f, false).mx);
  }
  if (a.mode != 2) {
    for (int s = 32; s > 0; s >>= 1) mx = fmaxf(mx, __shfl_xor(mx, s));
    if ((tid & 63) == 0) red_f[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red_f[0], red_f[1]), fmaxf(red_f[2], red_f[3]));
    if (a.mode == 1) {
      if (tid == 0) a.rowmax[row0] = mx;
      return;
    }
  } else {
    const float* gm = a.rowmax + (row0 / a.rpg) * a.rpg;
    for (int i = 0; i < a.rpg; ++i) mx = fmaxf(mx, gm[i]);
  }
  const float cutoff = a.thr * mx;
  int cnt = 0;
  for (int r = 0; r < rows; ++r) {
    cnt += p.scan(r, cutoff, true).cnt;
    p.inverse(r, a.y + (row0 + r) * L);
  }
  if (!a.kept) return;
  for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s);
  if ((tid & 63) == 0) red_i[tid >> 6] = cnt;
  __syncthreads();
  if (tid == 0) {
    const int total = red_i[0] + red_i[1] + red_i[2] + red_i[3];
    if (a.mode == 0) a.kept[blockIdx.x] = total;
    else atomicAdd(a.kept + row0 / a.rpg, total);       // integers: the sum does not depend on the order
  }
}

__global__ __launch_bounds__(FFT_THREADS) void k_fft_denoise(FftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fft_smem[];
  __shared__ float red_f[4];
  __shared__ int red_i[4];
  fft_group<FftPath>(a, fft_smem, red_f, red_i);
}

__global__ __launch_bounds__(FFT_THREADS) void k_dft_denoise(FftArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fft_smem[];
  __shared__ float red_f[4];
  __shared__ int red_i[4];
  fft_group<DirectPath>(a, fft_smem, red_f, red_i);
}

// ---------------------------------------------------------------- host
enum { FFT_REFUSED = 0, FFT_FAST = 1, FFT_DIRECT = 2 };

int fft_classify(int L) {
  if (L < 2 || L > FFT_MAX_L) return FFT_REFUSED;
  int m = L;
  for (int f : {2, 3, 5})
    while (m % f == 0) m /= f;
  if (L % 2 == 0 && m == 1 && L >= FFT_MIN_L) return FFT_FAST;
  return L <= DIRECT_MAX_L ? FFT_DIRECT : FFT_REFUSED;
}

// radix 4 while it divides, then 2, 3, 5
bool fft_plan(int L, int cls, FftPlan& P) {
  P.L = L, P.N = L / 2, P.npass = 0;
  if (cls != FFT_FAST) return true;
  int m = P.N;
  for (int f : {4, 2, 3, 5})
    while (m % f == 0) {
      if (P.npass == FFT_MAX_PASSES) return false;
      P.radix[P.npass++] = f;
      m /= f;
    }
  return m == 1;
}

long long fft_lds_bytes(int L, int cls, long long rows) {
  const long long N = L / 2;
  if (cls == FFT_FAST) return 8 * N + 8 * (N / 2 + 1) + 8 * N + rows * 8 * N;
  return 4LL * ((L + 3) & ~3) + 8LL * L + rows * 8 * (L / 2 + 1);
}

}  // namespace

// bytes of scratch ral_fft_denoise needs (0: one launch, the group is resident), -1: a length or a count that is refused
static long long fft_denoise_scratch_bytes(long long groups, int rows_per_group, int L) {
  const int cls = fft_classify(L);
  if (cls == FFT_REFUSED || groups < 0 || rows_per_group < 1) return -1;
  if (groups > 0x7fffffffLL / rows_per_group) return -1;
  if (fft_lds_bytes(L, cls, rows_per_group) <= FFT_LDS_BUDGET) return 0;
  return groups * rows_per_group * (long long)sizeof(float);
}

// the counts and the length both entry points refuse, in the words of `who`
static int fft_denoise_counts(const char* who, int64_t groups, int rows_per_group, int L) {
  if (groups < 0 || rows_per_group < 1)
    return ral_fail("%s: need groups >= 0 and rows_per_group >= 1 (groups=%lld rows_per_group=%d)", who, (long long)groups, rows_per_group);
  if (groups > 0x7fffffffLL / rows_per_group)
    return ral_fail("%s: need groups * rows_per_group < 2^31 (groups=%lld rows_per_group=%d)", who, (long long)groups, rows_per_group);
  if (fft_denoise_scratch_bytes(0, 1, L) < 0)
    return ral_fail("%s: L=%d is not supported: need an even record length with no prime factor above 5 in [16, 8192] (the FFT path), "
                    "or any other length in [2, 1024] (the direct path)", who, L);
  return 0;
}

extern "C" int64_t ral_fft_denoise_scratch_bytes(int64_t groups, int rows_per_group, int L) {
  if (fft_denoise_counts("fft_denoise_scratch_bytes", groups, rows_per_group, L)) return -1;
  return (int64_t)fft_denoise_scratch_bytes((long long)groups, rows_per_group, L);
}

extern "C" int ral_fft_denoise(const float* x, float* y, int32_t* kept, int64_t groups, int rows_per_group, int L, float threshold,
                               void* scratch, ral_stream s) {
  if (!x || !y) return ral_fail("fft_denoise: null pointer (x=%p y=%p)", (const void*)x, (void*)y);
  if (fft_denoise_counts("fft_denoise", groups, rows_per_group, L)) return -1;
  if (!(threshold >= 0.f)) return ral_fail("fft_denoise: the threshold factor must be non-negative (got %g)", (double)threshold);
  const long long sb = fft_denoise_scratch_bytes((long long)groups, rows_per_group, L);
  if (sb > 0 && !scratch)
    return ral_fail("fft_denoise: null scratch, %lld bytes are needed (groups=%lld rows_per_group=%d L=%d)", sb, (long long)groups,
                rows_per_group, L);
  if (groups == 0) {
    HIP_OK(hipGetLastError());
    return 0;
  }
  hipStream_t stream = (hipStream_t)s;
  const int cls = fft_classify(L);
  FftArgs a;
  if (!fft_plan(L, cls, a.plan))
    return ral_fail("fft_denoise: refused (groups=%lld rows_per_group=%d L=%d)", (long long)groups, rows_per_group, L);
  a.x = x, a.y = y, a.kept = kept, a.rowmax = static_cast<float*>(scratch), a.rpg = rows_per_group, a.thr = threshold;
  const bool resident = sb == 0;
  const size_t lds = (size_t)fft_lds_bytes(L, cls, resident ? rows_per_group : 1);
  const void* fn = cls == FFT_FAST ? reinterpret_cast<const void*>(k_fft_denoise) : reinterpret_cast<const void*>(k_dft_denoise);
  auto run = [&](int mode, unsigned grid) {
    a.mode = mode;
    if (cls == FFT_FAST) k_fft_denoise<<<grid, FFT_THREADS, lds, stream>>>(a);
    else k_dft_denoise<<<grid, FFT_THREADS, lds, stream>>>(a);
  };
  // (a failed HIP call of the set-up is reported in HIP's words)
  if (lds > 48 * 1024 && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return ral_fail("fft_denoise: %s", hipGetErrorString(hipGetLastError()));
  if (resident) run(0, (unsigned)groups);
  else {
    if (kept && hipMemsetAsync(kept, 0, (size_t)groups * sizeof(int32_t), stream) != hipSuccess)
      return ral_fail("fft_denoise: %s", hipGetErrorString(hipGetLastError()));
    run(1, (unsigned)(groups * rows_per_group));
    run(2, (unsigned)(groups * rows_per_group));
  }
  HIP_OK(hipGetLastError());
  return 0;
}
