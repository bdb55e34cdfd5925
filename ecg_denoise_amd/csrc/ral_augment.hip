// On-the-fly noise mixing of training batches (ral_mix_batch): for every window of a batch the clean row and its crop, the noise
// kind, the noise segment and the SNR are drawn on the device, the crop is z-scored per lead and the noise segment added at the
// drawn SNR -- the reference's np_norm + Gnoisegen (local_utils/local_utils.py:176-192, 261-266) per window, in front of the
// training loop instead of once on disk (data_utils.py:88-117).
//
// One launch, one workgroup of four waves per window, plain HIP C++.  The draw is Philox4x32-10 keyed by the seed and counted by
// the sample's ordinal, so a sample depends on (seed, ordinal) and on nothing else: not on B, the grid, `first` or its
// neighbours.  The window's clean and noise rows are read from global memory ONCE, at arbitrary (unaligned) crop offsets, into
// LDS; the three passes over them (sum x and sum n^2; sum (x - mean)^2; the mix) then run from LDS.  A lead's samples are cut
// into `cpl` equal pieces so that all four waves have work when leads < 4; piece u = lead * cpl + p belongs to wave u % 4 in
// every pass, lane l of it adds samples a + l, a + l + 64, ..., a xor-shuffle tree of fixed shape adds the lanes and the pieces
// of a lead are added in piece order: every sum has one fixed order, all in double.  No scratch, no memset, no atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"

// The geometry of a call travels by value, as a kernel argument (thresholds included: no copy).
struct MixBatchGeom {
  long long N, Lsrc, Tn;
  int leads, L, K;
  uint32_t cum[RAL_MIX_MAX_KINDS];
  double snr_lo, snr_hi;
  uint64_t seed, first;
};

#define AUG_THREADS 256
#define AUG_WAVES (AUG_THREADS / 64)
#define AUG_MAXLEADS 16
#define AUG_MAXU 16                 // pieces per window: leads * cpl <= max(AUG_MAXLEADS, AUG_WAVES)
#define AUG_PART (3 * AUG_MAXU + 2) // doubles of LDS in front of the staged rows (a multiple of 2: 16 bytes)
#define AUG_MAX_FOOT 16384          // leads * L: two fp32 rows of it are 128 KB of the CU's 160 KB of LDS
#define AUG_STD_FLOOR 1e-6          // as ral_stream_windows

static __host__ __device__ inline void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}

// (x * n) >> 32: a uniform integer in [0, n)
static __host__ __device__ inline uint32_t mul_hi(uint32_t x, uint32_t n) { return (uint32_t)(((uint64_t)x * n) >> 32); }

static __host__ __device__ inline void mix_draw(const MixBatchGeom& G, uint64_t g, uint32_t (&d)[4], double* snr_db) {
  uint32_t a[4] = {(uint32_t)g, (uint32_t)(g >> 32), 0u, 0u};
  uint32_t b[4] = {(uint32_t)g, (uint32_t)(g >> 32), 1u, 0u};
  philox4x32_10(a, (uint32_t)G.seed, (uint32_t)(G.seed >> 32));
  philox4x32_10(b, (uint32_t)G.seed, (uint32_t)(G.seed >> 32));
  d[0] = mul_hi(a[0], (uint32_t)G.N);
  d[1] = mul_hi(a[1], (uint32_t)(G.Lsrc - G.L + 1));
  uint32_t kind = (uint32_t)G.K - 1;
  for (int k = G.K - 2; k >= 0; --k)
    if (a[2] < G.cum[k]) kind = (uint32_t)k;      // ends at the first k with a[2] < cum[k] (the thresholds do not decrease)
  d[2] = kind;
  d[3] = mul_hi(b[0], (uint32_t)(G.Tn - G.L + 1));
  *snr_db = G.snr_lo + (G.snr_hi - G.snr_lo) * ((double)a[3] * (1.0 / 4294967296.0));
}

static __device__ __forceinline__ double aug_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

__global__ __launch_bounds__(AUG_THREADS) void k_mix_batch(const float* __restrict__ bank, const float* __restrict__ noise,
                                                           const long long* __restrict__ rows, const MixBatchGeom G,
                                                           float* __restrict__ noisy, float* __restrict__ clean,
                                                           int32_t* __restrict__ draws, double* __restrict__ snr_out) {
  extern __shared__ float4 smem4[];
  double* part = reinterpret_cast<double*>(smem4);      // [3][AUG_MAXU]: sum x, sum n^2, sum (x - mean)^2 per piece; 10^(snr/10)
  const int L = G.L, leads = G.leads;
  const int foot = leads * L;
  float* xs = reinterpret_cast<float*>(part + AUG_PART);             // 400 bytes in: the rows stay 16-byte aligned
  float* ns = xs + foot;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t blk = blockIdx.x;

  uint32_t d[4];
  double snr_db;
  mix_draw(G, G.first + blk, d, &snr_db);
  long long row = d[0];
  if (rows) row = rows[blk];
  const bool ok = row >= 0 && row < G.N;
  if (threadIdx.x == 0) {
    draws[blk * 4 + 0] = ok ? (int32_t)row : -1;
    draws[blk * 4 + 1] = (int32_t)d[1]; draws[blk * 4 + 2] = (int32_t)d[2]; draws[blk * 4 + 3] = (int32_t)d[3];
    snr_out[blk] = snr_db;
  }
  float* yc = clean + blk * foot;
  float* yn = noisy + blk * foot;
  if (!ok) {        // a caller's row outside the bank: nothing is read; the window is NaN and its draw says row -1
    const float nanf = __int_as_float(0x7fc00000);
    for (int i = threadIdx.x; i < foot; i += AUG_THREADS) { yc[i] = nanf; yn[i] = nanf; }
    return;
  }
  const float* xg = bank + (size_t)row * leads * (size_t)G.Lsrc + d[1];
  const float* ng = noise + (size_t)d[2] * leads * (size_t)G.Tn + d[3];

  const int cpl = leads >= AUG_WAVES ? 1 : AUG_WAVES / leads;       // pieces per lead
  const int nunit = leads * cpl;
  const int chunk = (L + cpl - 1) / cpl;

  // pass A: global -> LDS, sum x and sum n^2 of every piece
  for (int u = wave; u < nunit; u += AUG_WAVES) {
    const int c = u / cpl, p = u - c * cpl;
    const int a = p * chunk, b = min(L, a + chunk);
    const float* xr = xg + (size_t)c * (size_t)G.Lsrc;
    const float* nr = ng + (size_t)c * (size_t)G.Tn;
    double sx = 0.0, snn = 0.0;
    for (int i = a + lane; i < b; i += 64) {
      const float xv = xr[i], nv = nr[i];
      xs[c * L + i] = xv; ns[c * L + i] = nv;
      sx += (double)xv; snn += (double)nv * (double)nv;
    }
    sx = aug_wave_sum(sx); snn = aug_wave_sum(snn);
    if (lane == 0) { part[u] = sx; part[AUG_MAXU + u] = snn; }
  }
  // 10^(snr_db / 10) depends on the draw alone: one wave evaluates the (long) double pow, under the other waves' loads
  if (threadIdx.x == AUG_THREADS - 1) part[3 * AUG_MAXU] = pow(10.0, snr_db / 10.0);
  __syncthreads();
  // lane c < leads of every wave: the mean of lead c
  double mean_l = 0.0;
  if (lane < leads) {
    for (int p = 0; p < cpl; ++p) mean_l += part[lane * cpl + p];
    mean_l /= (double)L;
  }
  // pass B: sum (x - mean)^2 of every piece, from the samples this wave staged itself
  for (int u = wave; u < nunit; u += AUG_WAVES) {
    const int c = u / cpl, p = u - c * cpl;
    const int a = p * chunk, b = min(L, a + chunk);
    const double mean = __shfl(mean_l, c, 64);
    double sd2 = 0.0;
    for (int i = a + lane; i < b; i += 64) {
      const double dv = (double)xs[c * L + i] - mean;
      sd2 += dv * dv;
    }
    sd2 = aug_wave_sum(sd2);
    if (lane == 0) part[2 * AUG_MAXU + u] = sd2;
  }
  __syncthreads();
  // lane c < leads: std of lead c (population, floored) and the lead's share of P_clean = sum ((x - mean) / std)^2;
  // lane u < nunit: piece u's share of P_noise
  double std_l = 1.0, pc = 0.0, pn = 0.0;
  if (lane < leads) {
    double d2 = 0.0;
    for (int p = 0; p < cpl; ++p) d2 += part[2 * AUG_MAXU + lane * cpl + p];
    std_l = fmax(sqrt(d2 / (double)L), AUG_STD_FLOOR);
    pc = d2 / (std_l * std_l);
  }
  if (lane < nunit) pn = part[AUG_MAXU + lane];
  pc = aug_wave_sum(pc); pn = aug_wave_sum(pn);
  const double scale = pn == 0.0 ? 0.0 : sqrt(pc / part[3 * AUG_MAXU] / pn);

  // pass C: the mix, rounded once to fp32
  for (int u = wave; u < nunit; u += AUG_WAVES) {
    const int c = u / cpl, p = u - c * cpl;
    const int a = p * chunk, b = min(L, a + chunk);
    const double mean = __shfl(mean_l, c, 64), sd = __shfl(std_l, c, 64);
    for (int i = a + lane; i < b; i += 64) {
      const double cv = ((double)xs[c * L + i] - mean) / sd;
      yc[c * L + i] = (float)cv;
      yn[c * L + i] = (float)(cv + scale * (double)ns[c * L + i]);
    }
  }
}

// the rules of the draw and of the window geometry (everything but B and the pointers); nullptr: all hold
static const char* mix_batch_check(const MixBatchGeom& G) {
  if (G.N < 1) return "N >= 1";
  if (G.leads < 1 || G.leads > AUG_MAXLEADS) return "1 <= leads <= 16";
  if (G.L < 1 || G.L > G.Lsrc) return "1 <= L <= Lsrc";
  if (G.K < 1 || G.K > RAL_MIX_MAX_KINDS) return "1 <= K <= 8";
  if (G.Tn < G.L) return "Tn >= L";
  if (!isfinite(G.snr_lo) || !isfinite(G.snr_hi) || G.snr_lo > G.snr_hi) return "finite snr_lo <= snr_hi";
  for (int k = 1; k < G.K; ++k)
    if (G.cum[k] < G.cum[k - 1]) return "non-decreasing thresholds";
  if (G.N > 0x7fffffffLL || G.Lsrc - G.L + 1 > 0xffffffffLL || G.Tn - G.L + 1 > 0xffffffffLL)
    return "N < 2^31, B < 2^31, Lsrc - L + 1 < 2^32 and Tn - L + 1 < 2^32";
  if ((long long)G.leads * G.L > AUG_MAX_FOOT) return "leads * L <= 16384 (the window's two rows are staged in LDS)";
  return nullptr;
}

static MixBatchGeom mix_geom(int64_t N, int leads, int64_t Lsrc, int L, int K, int64_t Tn, const uint32_t* cum, double snr_lo,
                             double snr_hi, uint64_t seed, uint64_t first) {
  MixBatchGeom G;
  G.N = (long long)N; G.Lsrc = (long long)Lsrc; G.Tn = (long long)Tn;
  G.leads = leads; G.L = L; G.K = K;
  for (int k = 0; k < RAL_MIX_MAX_KINDS; ++k) G.cum[k] = (cum && k < K) ? cum[k] : 0xffffffffu;
  G.snr_lo = snr_lo; G.snr_hi = snr_hi;
  G.seed = seed; G.first = first;
  return G;
}
#define MIX_ARGS "(N=%lld leads=%d Lsrc=%lld L=%d K=%d Tn=%lld B=%lld snr_db=[%g, %g])"

extern "C" int ral_mix_batch(const float* bank, const float* noise, const int64_t* rows, int64_t N, int leads, int64_t Lsrc, int L,
                             int K, int64_t Tn, const uint32_t* cum, double snr_lo, double snr_hi, uint64_t seed, uint64_t first,
                             int64_t B, float* noisy, float* clean, int32_t* draws, double* snr_db, ral_stream s) {
  const MixBatchGeom G = mix_geom(N, leads, Lsrc, L, K, Tn, cum, snr_lo, snr_hi, seed, first);
  const char* why = (!bank || !noise || !cum || !noisy || !clean || !draws || !snr_db) ? "no null pointer (only rows may be null)"
                                                                                       : mix_batch_check(G);
  if (!why && B < 1) why = "B >= 1";
  if (!why && B > 0x7fffffffLL) why = "N < 2^31, B < 2^31, Lsrc - L + 1 < 2^32 and Tn - L + 1 < 2^32";
  if (why)
    return ral_fail("mix_batch: need %s " MIX_ARGS, why, (long long)N, leads, (long long)Lsrc, L, K, (long long)Tn, (long long)B,
                    snr_lo, snr_hi);
  const size_t lds = AUG_PART * sizeof(double) + 2 * (size_t)G.leads * G.L * sizeof(float);
  RAL_SET_LDS(k_mix_batch, lds);
  k_mix_batch<<<(unsigned)B, AUG_THREADS, lds, (hipStream_t)s>>>(bank, noise, reinterpret_cast<const long long*>(rows), G, noisy, clean,
                                                                 draws, snr_db);
  HIP_OK(hipGetLastError());
  return 0;
}

// the draw of ordinal g on the host, by the code the kernel runs
extern "C" int ral_mix_draw(int64_t N, int64_t Lsrc, int L, int K, int64_t Tn, const uint32_t* cum, double snr_lo, double snr_hi,
                            uint64_t seed, uint64_t g, int32_t* draw, double* snr_db) {
  const MixBatchGeom G = mix_geom(N, 1, Lsrc, L, K, Tn, cum, snr_lo, snr_hi, seed, 0);
  const char* why = (!cum || !draw || !snr_db) ? "no null pointer" : mix_batch_check(G);
  if (why)
    return ral_fail("mix_draw: need %s " MIX_ARGS, why, (long long)N, 1, (long long)Lsrc, L, K, (long long)Tn, 1LL, snr_lo, snr_hi);
  uint32_t d[4];
  mix_draw(G, g, d, snr_db);
  for (int i = 0; i < 4; ++i) draw[i] = (int32_t)d[i];
  return 0;
}
