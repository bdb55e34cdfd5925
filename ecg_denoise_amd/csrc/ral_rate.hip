// Sample-rate conversion in front of and behind the models (ral_rate_records / ral_rate_pool; host side: rate.py).
//
// The conversion is scipy.signal.resample_poly(x, up, down, window=('kaiser', 5.0), padtype='edge') with up / down in lowest
// terms: half = 10 max(up, down), h the 2 half + 1 taps designed on the host, and
//   y[m] = sum over n = ceil((m down - half) / up) .. floor((m down + half) / up) of h[m down - n up + half] x[clamp(n, 0, T - 1)]
// accumulated in fp32 with fmaf in ascending n.  With q = m down + half, nh = q / up and r = q % up the taps of output m are
// h[r + i up] on x[nh - i], i = 0 .. (2 half - r) / up: the polyphase row r.  Every row is padded with zero taps to
// K = ceil((2 half + 1) / up) entries, so the tap loop has a fixed length; the padded taps come first in ascending n, where they
// add 0 to an accumulator that is 0 (every staged sample is a clamped, i.e. real, sample of the stream).
//
// One workgroup computes a tile of consecutive outputs of one (row, lead).  It stages in LDS
//   the bank, K x up, row t = taps i = K - 1 - t (so t ascends with n), column p = the phase's place in the order in which
//     consecutive outputs visit the phases: r = p (down mod up) mod up.  Consecutive lanes then read consecutive words of a
//     row (wrapping at up), whatever down mod up is;
//   the input span of the tile with the clamp applied, [nh(first) - (K - 1), nh(last)], shifted by 0 .. 3 words so that an
//     LDS word and the global word it comes from sit at the same place of a 16-byte group (float4 loads in the interior);
//   the tile's outputs, shifted the same way for float4 stores.
// rate_tile is the only place that forms an output, for whole records and for pool chunks alike: a record is a stream that
// has received nothing before (n0 = 0) and gets all T samples now, so both read the same staged values through the same code.
#include "../../include/ralenet.h"
#include "ral_device.hpp"
#include "ral_model.hpp"
#include "ral_slots.hpp"
#include <stdint.h>

namespace {

constexpr int RATE_THREADS = 256;
constexpr int RATE_TILE_MAX = 1024;      // outputs per workgroup, halved while the input span is longer than RATE_SPAN_CAP
constexpr int RATE_TILE_MIN = 64;
constexpr int RATE_SPAN_CAP = 4096;      // floats of the staged input span
constexpr int RATE_LDS_FLOATS = 16384;   // the budget: 64 KB, what a kernel gets without opting into more

struct RateGeom {
  int up, down, half, K, ntaps, tile, dinv, bank_floats, span_floats;
};

// one (stream, lead): the stream had n0 samples before this call and has n0 + c now.  chunk[0 .. c) are samples n0 .. n0 + c - 1,
// hist[0 .. hist_len) samples n0 - hist_len .. n0 - 1 (null for a record: n0 = 0, nothing lies before the chunk)
struct RateRow {
  const float* chunk;
  const float* hist;
  float* out;          // output m0 + j at out[j]
  long long n0, c, m0, m;
  int hist_len;
};

RAL_DEV int rate_word(const void* p) { return (int)(((uintptr_t)p >> 2) & 3); }

// outputs [m0 + j0, m0 + j0 + cnt) of one row.  bl, xs, os: the three LDS regions, each 16-byte aligned
RAL_DEV void rate_tile(const RateRow& rw, long long j0, int cnt, const RateGeom& g, const float* __restrict__ bank, float* bl,
                       float* xs, float* os) {
  const int tid = threadIdx.x, up = g.up, K = g.K;
  const long long q0 = (rw.m0 + j0) * g.down + g.half;
  const long long nh0 = q0 / up;
  const int r0 = (int)(q0 - nh0 * up);
  const long long n_first = nh0 - (K - 1);                       // the oldest sample of the span
  const int count = (r0 + (cnt - 1) * g.down) / up + K;          // its length

  // the bank, in visiting order of the phases
  const int d = g.down % up;
  for (int e = tid; e < K * up; e += RATE_THREADS) {
    const int t = e / up, p = e - t * up;
    const int j = (int)(((long long)p * d) % up) + (K - 1 - t) * up;
    bl[e] = j < g.ntaps ? bank[j] : 0.f;
  }

  // the span.  Word w of xs holds sample n_first - ax + w, clamped to what the stream holds (the host has checked that the call
  // needs nothing older than the history); the chunk is the part of the stream that float4 loads may touch
  const long long c_lo = rw.n0, c_hi = rw.n0 + rw.c;
  const int ax = (int)(((long long)rate_word(rw.chunk) + ((n_first - c_lo) & 3)) & 3);
  for (int gi = tid; gi < (ax + count + 3) >> 2; gi += RATE_THREADS) {
    const long long pos = n_first - ax + 4 * (long long)gi;
    if (pos >= c_lo && pos + 4 <= c_hi) {
      *reinterpret_cast<float4*>(xs + 4 * gi) = *reinterpret_cast<const float4*>(rw.chunk + (pos - c_lo));
    } else {
      for (int e = 0; e < 4; ++e) {
        const int w = 4 * gi + e;
        if (w >= ax && w < ax + count) xs[w] = slot_sample(rw.chunk, 0, rw.hist, rw.hist_len, rw.n0, c_hi, 0, pos + e);
      }
    }
  }
  __syncthreads();

  const int p0 = (int)(((long long)r0 * g.dinv) % up);
  float* dst = rw.out + j0;
  const int ao = rate_word(dst);
  for (int j = tid; j < cnt; j += RATE_THREADS) {
    const int b = (r0 + j * g.down) / up;          // nh(m) - nh0
    const int p = (p0 + j) % up;
    const float* xr = xs + ax + b;
    const float* br = bl + p;
    float acc = 0.f;
#pragma unroll 4
    for (int t = 0; t < K; ++t) acc = fmaf(br[t * up], xr[t], acc);
    os[ao + j] = acc;
  }
  __syncthreads();

  for (int gi = tid; gi < (ao + cnt + 3) >> 2; gi += RATE_THREADS) {
    const int j = 4 * gi - ao;
    if (j >= 0 && j + 4 <= cnt) {
      *reinterpret_cast<float4*>(dst + j) = *reinterpret_cast<const float4*>(os + 4 * gi);
    } else {
      for (int e = 0; e < 4; ++e)
        if (j + e >= 0 && j + e < cnt) dst[j + e] = os[4 * gi + e];
    }
  }
}

RAL_DEV void rate_lds(const RateGeom& g, float* base, float*& bl, float*& xs, float*& os) {
  bl = base;
  xs = bl + g.bank_floats;
  os = xs + g.span_floats;
}

// grid (tiles of a record, R * leads)
__global__ __launch_bounds__(RATE_THREADS) void k_rate_records(const float* __restrict__ x, long long T, long long T_out, RateGeom g,
                                                               const float* __restrict__ bank, float* __restrict__ y) {
  extern __shared__ __attribute__((aligned(16))) float rate_smem[];
  float *bl, *xs, *os;
  rate_lds(g, rate_smem, bl, xs, os);
  const long long row = blockIdx.y, j0 = (long long)blockIdx.x * g.tile;
  const RateRow rw{x + row * T, nullptr, y + row * T_out, 0, T, 0, T_out, 0};
  const long long left = T_out - j0;
  rate_tile(rw, j0, (int)(left < g.tile ? left : g.tile), g, bank, bl, xs, os);
}

typedef ral_rate_row RatePoolRow;

// grid (tiles of the longest row + 1, rows * leads): the last x index writes the next history of its (row, lead)
__global__ __launch_bounds__(RATE_THREADS) void k_rate_pool(float* hist, const float* __restrict__ x,
                                                            const RatePoolRow* __restrict__ tab, long long cap, int leads,
                                                            int hist_len, RateGeom g, const float* __restrict__ bank,
                                                            float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float rate_smem[];
  const int r = blockIdx.y / leads, lead = blockIdx.y - r * leads;
  const RatePoolRow t = tab[r];
  const float* hr = hist + slot_plane(t.turn, t.slot, cap, leads, hist_len, lead);
  const float* chunk = x + (t.x_off * leads + (long long)lead * t.c);
  if (blockIdx.x == gridDim.x - 1) {
    if (t.flags & RAL_POOL_KEEP)
      slot_write_history(hr, chunk, hist + slot_plane(1 - t.turn, t.slot, cap, leads, hist_len, lead), t.n0, t.c, hist_len);
    return;
  }
  const long long j0 = (long long)blockIdx.x * g.tile;
  if (j0 >= t.m) return;
  float *bl, *xs, *os;
  rate_lds(g, rate_smem, bl, xs, os);
  const RateRow rw{chunk, hr, out + (t.out_off * leads + (long long)lead * t.m), t.n0, t.c, t.m0, t.m, hist_len};
  const long long left = t.m - j0;
  rate_tile(rw, j0, (int)(left < g.tile ? left : g.tile), g, bank, bl, xs, os);
}

long long rate_gcd(long long a, long long b) { return b ? rate_gcd(b, a % b) : a; }

// the geometry of a pair -> null, or the rule that is broken
const char* rate_geom(int up, int down, int ntaps, RateGeom& g) {
  if (up < 1 || down < 1 || up > 65535 || down > 65535) return "1 <= up, down <= 65535";
  if (rate_gcd(up, down) != 1) return "up / down in lowest terms";
  g.up = up, g.down = down, g.half = 10 * (up > down ? up : down);
  g.ntaps = 2 * g.half + 1;
  if (ntaps != g.ntaps) return "ntaps = 20 max(up, down) + 1";
  g.K = (2 * g.half + up) / up;
  g.bank_floats = (g.K * up + 3) & ~3;
  g.tile = RATE_TILE_MAX;
  auto span = [&](int tile) { return (long long)(tile - 1) * down / up + g.K + 2; };
  while (g.tile > RATE_TILE_MIN && span(g.tile) > RATE_SPAN_CAP) g.tile >>= 1;
  const long long sp = (span(g.tile) + 8 + 3) & ~3LL;     // (+ the shift of up to 3 words and the rest of the last group)
  if (g.bank_floats + sp + g.tile + 8 > RATE_LDS_FLOATS) return "a bank and a tile's input span that fit 64 KB of LDS";
  g.span_floats = (int)sp;
  g.dinv = 0;
  for (int v = 1; v < up; ++v)
    if ((long long)v * (down % up) % up == 1) { g.dinv = v; break; }
  return nullptr;
}

size_t rate_lds_bytes(const RateGeom& g) { return (size_t)(g.bank_floats + g.span_floats + g.tile + 8) * sizeof(float); }

// ceil(a / b) for b > 0
long long rate_ceil_div(long long a, long long b) { return a >= 0 ? (a + b - 1) / b : -((-a) / b); }

const char* rate_pool_fault(const RatePoolRow* tab, int rows, long long cap, int leads, const RateGeom& g, int hist_len,
                            long long x_total, long long out_total, bool walk, int* bad) {
  *bad = -1;
  if (rows < 1) return "rows >= 1";
  if (cap < 1) return "capacity >= 1";
  if (leads < 1) return "leads >= 1";
  if ((long long)rows * leads > 65535) return "rows * leads <= 65535";
  if (hist_len < g.K) return "hist_len >= 2 half / up + 1";
  if (x_total < 0 || out_total < 0) return "x_total, out_total >= 0";
  if (!walk) return nullptr;
  const long long big = 1LL << 40;
  const SlotRules rules{1, false, "0 <= n0, m0 <= 2^40, 0 <= c < 2^30 and m >= 0",
                        "T = n0 + c >= 1 without RAL_POOL_KEEP, or T = -1 with RAL_POOL_KEEP"};
  auto in_range = [&](const RatePoolRow& t) {
    return !(t.n0 < 0 || t.n0 > big || t.m0 < 0 || t.m0 > big || t.c < 0 || t.c > 0x3fffffff || t.m < 0);
  };
  auto own = [&](const RatePoolRow& t) -> const char* {
    if (t.out_off < 0 || t.out_off + t.m > out_total) return "the emitted samples inside the packed output";
    if (t.m == 0) return nullptr;
    const long long n1 = t.n0 + t.c, last = t.m0 + t.m - 1;
    if (n1 < 1) return "a sample received before anything is emitted";
    if (t.T < 0 ? last * g.down + g.half >= n1 * g.up : last * g.down >= n1 * g.up)
      return "outputs that are final: (m0 + m - 1) down + half < (n0 + c) up, or m0 + m <= ceil(T up / down) at the end";
    long long oldest = (t.m0 * g.down + g.half) / g.up - (g.K - 1);
    if (oldest < 0) oldest = 0;
    if (oldest < t.n0 - hist_len) return "the oldest sample of output m0 inside the history";
    return nullptr;
  };
  return slots_walk(tab, rows, cap, x_total, rules, in_range, SlotNoRule{}, own, bad);
}

}  // namespace

extern "C" int ral_rate_records(const float* x, int64_t R, int leads, int64_t T, int up, int down, const float* bank, int ntaps,
                                float* y, int64_t T_out, ral_stream s) {
  if (!x || !bank || !y) return ral_fail("rate_records: null pointer");
  RateGeom g;
  long long tiles = 0;
  const char* why = rate_geom(up, down, ntaps, g);
  if (!why && (R < 1 || leads < 1 || T < 1 || T > (1LL << 40))) why = "R >= 1, leads >= 1, 1 <= T <= 2^40";
  if (!why && T_out != rate_ceil_div(T * up, down)) why = "T_out = ceil(T up / down)";
  if (!why && ((tiles = (T_out + g.tile - 1) / g.tile) > 0xffffffLL || R * leads > 65535))
    why = "R * leads <= 65535 and fewer than 2^24 tiles per record";
  if (why)
    return ral_fail("rate_records: need %s (R=%lld leads=%d T=%lld up=%d down=%d ntaps=%d T_out=%lld)", why, (long long)R, leads,
                (long long)T, up, down, ntaps, (long long)T_out);
  const size_t lds = rate_lds_bytes(g);
  k_rate_records<<<dim3((unsigned)tiles, (unsigned)(R * leads)), RATE_THREADS, lds, (hipStream_t)s>>>(x, T, T_out, g, bank, y);
  HIP_OK(hipGetLastError());
  return 0;
}

extern "C" int ral_rate_pool(float* hist, const float* x, int64_t x_total, const ral_rate_row* table, int rows,
                             ral_rate_row* table_dev, int upload, int64_t capacity, int leads, int up, int down, const float* bank,
                             int ntaps, int hist_len, float* out, int64_t out_total, ral_stream s) {
  if (!hist || !x || !table || !table_dev || !bank || !out) return ral_fail("rate_pool: null pointer");
  RateGeom g;
  int bad = -1;
  long long tiles = 0;
  const char* why = rate_geom(up, down, ntaps, g);
  if (!why) why = rate_pool_fault(table, rows, capacity, leads, g, hist_len, x_total, out_total, upload != 0, &bad);
  if (!why) {
    long long m_max = 0;
    for (int r = 0; r < rows; ++r) m_max = table[r].m > m_max ? table[r].m : m_max;
    tiles = (m_max + g.tile - 1) / g.tile;
    if (tiles > 0xffffffLL) why = "fewer than 2^24 tiles of outputs per row";
  }
  const int rc = why ? -1 : upload ? slots_upload(table, rows, table_dev, (hipStream_t)s) : 0;
  if (!rc)
    k_rate_pool<<<dim3((unsigned)tiles + 1, (unsigned)(rows * leads)), RATE_THREADS, rate_lds_bytes(g), (hipStream_t)s>>>(
        hist, x, table_dev, capacity, leads, hist_len, g, bank, out);
  return table_done("rate_pool", rc, why, bad, "rows=%d capacity=%lld leads=%d up=%d down=%d ntaps=%d hist_len=%d x_total=%lld "
                    "out_total=%lld", rows, (long long)capacity, leads, up, down, ntaps, hist_len, (long long)x_total,
                    (long long)out_total);
}
