// HBM-bound kernels around the transformer stack: conv stem (+LeakyReLU +BatchNorm),
// output conv, loss/SNR/RMSE reduction, fused flat Adam.  (gfx950)
//
// Reference behaviour: model/raletransformer.py:568-572, 636, 676-678;
// local_utils/evaluate.py:10-51; denoise_train.py:24,53 (Adam lr 1e-3, mse mean).
#include <vector>

#include "ral_device.hpp"
#include "ral_kernels.hpp"
#include "ral_slots.hpp"

// block-wide sum of NV per-thread values -> double atomics into out[0..NV)
template <int NV>
RAL_DEV void block_atomic_sums(const float (&v)[NV], double* __restrict__ out, double* red /* LDS NV*nwaves */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = group_sum<64>(v[i]);
    if (lane == 0) red[wave * NV + i] = (double)s;
  }
  __syncthreads();
  if (threadIdx.x < NV) {
    double t = 0.0;
    for (int w = 0; w < nw; ++w) t += red[w * NV + threadIdx.x];
    atomicAdd(out + threadIdx.x, t);
  }
  __syncthreads();
}

// ---------------------------------------------------------------------------------
// conv1: Conv1d(leads, 8, k3, p1) + LeakyReLU(0.2) -> a0 (B, L, 8) token-major.
// MODE 0: training, also accumulates per-channel sum / sum of squares (double).
// MODE 1: eval, applies BatchNorm with the running statistics and writes x0 directly.
// ---------------------------------------------------------------------------------
template <int LEADS, int MODE>
__global__ __launch_bounds__(256) void k_conv1_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                   const float* __restrict__ bias, float* __restrict__ out,
                                                   double* __restrict__ stats, const float* __restrict__ bnw,
                                                   const float* __restrict__ bnb, const float* __restrict__ rmean,
                                                   const float* __restrict__ rvar, int L, int Lp, int B) {
  // L: samples of a window (row stride of x); Lp >= L: token slots per window in `out` (a window length that is not a multiple
  // of 256 runs on the next multiple, ral_api.hip: the slots past L are written as zeros and are not part of the statistics)
  __shared__ double red[16 * 4];
  float wr[8][LEADS][3], br[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    br[o] = bias[o];
#pragma unroll
    for (int c = 0; c < LEADS; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) wr[o][c][k] = w[(o * LEADS + c) * 3 + k];
  }
  float sc[8], sh[8];
  if (MODE == 1) {
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      sc[o] = bnw[o] / sqrtf(rvar[o] + 1e-5f);
      sh[o] = bnb[o] - rmean[o] * sc[o];
    }
  }
  float acc[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  const size_t total = (size_t)B * Lp;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / Lp), l = (int)(i - (size_t)b * Lp);
    if (l >= L) {
      float4* pz = reinterpret_cast<float4*>(out + i * 8);
      pz[0] = make_float4(0.f, 0.f, 0.f, 0.f); pz[1] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    float xv[LEADS][3];
#pragma unroll
    for (int c = 0; c < LEADS; ++c) {
      const float* xr = x + ((size_t)b * LEADS + c) * L;
      xv[c][0] = l > 0 ? xr[l - 1] : 0.f;
      xv[c][1] = xr[l];
      xv[c][2] = l < L - 1 ? xr[l + 1] : 0.f;
    }
    float y[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float a = br[o];
#pragma unroll
      for (int c = 0; c < LEADS; ++c)
#pragma unroll
        for (int k = 0; k < 3; ++k) a = fmaf(wr[o][c][k], xv[c][k], a);
      a = a > 0.f ? a : 0.2f * a;
      if (MODE == 0) { acc[o] += a; acc[8 + o] += a * a; }
      else a = a * sc[o] + sh[o];
      y[o] = a;
    }
    float4* po = reinterpret_cast<float4*>(out + i * 8);
    po[0] = make_float4(y[0], y[1], y[2], y[3]);
    po[1] = make_float4(y[4], y[5], y[6], y[7]);
  }
  if (MODE == 0) block_atomic_sums<16>(acc, stats, red);
}

// stats: [sum(8), sumsq(8)] double; ss: [scale(8), shift(8), mean(8), rstd(8)] float
// The stem's BatchNorm in ONE launch (training): every workgroup forms the eight channels' scale / shift from the (all-reduced)
// sums itself - eight lanes of double arithmetic - and applies them to its share of the tokens; workgroup 0 also leaves ss
// (scale, shift, mean, rstd: the backward reads them) and the running statistics, (a finalise kernel and an apply kernel were two
// launches on the one stream that runs at the start of a step.)
__global__ __launch_bounds__(256) void k_bn_train8(const double* __restrict__ stats, double count, const float* __restrict__ bnw,
                                                   const float* __restrict__ bnb, float* __restrict__ ss, float* __restrict__ rmean,
                                                   float* __restrict__ rvar, const float* __restrict__ a0, float* __restrict__ x0,
                                                   size_t ntok) {
  __shared__ float sc_[8], sh_[8];
  if (threadIdx.x < 8) {
    const int c = threadIdx.x;
    const double mean = stats[c] / count;
    double var = stats[8 + c] / count - mean * mean;
    if (var < 0.0) var = 0.0;
    const float rstd = (float)(1.0 / sqrt(var + 1e-5));
    const float sc = bnw[c] * rstd, sh = bnb[c] - (float)mean * sc;
    sc_[c] = sc; sh_[c] = sh;
    if (blockIdx.x == 0) {
      ss[c] = sc; ss[8 + c] = sh; ss[16 + c] = (float)mean; ss[24 + c] = rstd;
      rmean[c] = 0.9f * rmean[c] + 0.1f * (float)mean;
      const double unb = count > 1.0 ? var * count / (count - 1.0) : var;
      rvar[c] = 0.9f * rvar[c] + 0.1f * (float)unb;
    }
  }
  __syncthreads();
  const float4 s0 = make_float4(sc_[0], sc_[1], sc_[2], sc_[3]), s1 = make_float4(sc_[4], sc_[5], sc_[6], sc_[7]);
  const float4 h0 = make_float4(sh_[0], sh_[1], sh_[2], sh_[3]), h1 = make_float4(sh_[4], sh_[5], sh_[6], sh_[7]);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < ntok * 2; i += (size_t)gridDim.x * blockDim.x) {
    const float4 v = reinterpret_cast<const float4*>(a0)[i];
    const bool hi = i & 1;
    reinterpret_cast<float4*>(x0)[i] = f4add(f4mul(v, hi ? s1 : s0), hi ? h1 : h0);
  }
}

// ---------------------------------------------------------------------------------
// output stage: z = u0 + x0 (token-major, 8 ch); y = Conv1d(8, leads, k3, p1)(z^T)
// ---------------------------------------------------------------------------------
template <int LEADS>
__global__ __launch_bounds__(256) void k_final_fwd(const float* __restrict__ u0, const float* __restrict__ x0,
                                                   const float* __restrict__ w, const float* __restrict__ bias,
                                                   float* __restrict__ y, int L, int Lp, int B) {
  // L: samples per window of y; Lp >= L: token slots per window of u0 / x0 (the slots past L do not exist for the conv: zero halo)
  float wr[LEADS][8][3];
#pragma unroll
  for (int o = 0; o < LEADS; ++o)
#pragma unroll
    for (int c = 0; c < 8; ++c)
#pragma unroll
      for (int k = 0; k < 3; ++k) wr[o][c][k] = w[(o * 8 + c) * 3 + k];
  const size_t total = (size_t)B * L;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (size_t)b * L);
    float acc[LEADS];
#pragma unroll
    for (int o = 0; o < LEADS; ++o) acc[o] = bias[o];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int ll = l + k - 1;
      if (ll < 0 || ll >= L) continue;
      const size_t t = (size_t)b * Lp + ll;
      const float4 a0 = reinterpret_cast<const float4*>(u0)[t * 2], a1 = reinterpret_cast<const float4*>(u0)[t * 2 + 1];
      const float4 b0 = reinterpret_cast<const float4*>(x0)[t * 2], b1 = reinterpret_cast<const float4*>(x0)[t * 2 + 1];
      const float z[8] = {a0.x + b0.x, a0.y + b0.y, a0.z + b0.z, a0.w + b0.w,
                          a1.x + b1.x, a1.y + b1.y, a1.z + b1.z, a1.w + b1.w};
#pragma unroll
      for (int o = 0; o < LEADS; ++o)
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[o] = fmaf(wr[o][c][k], z[c], acc[o]);
    }
#pragma unroll
    for (int o = 0; o < LEADS; ++o) y[((size_t)b * LEADS + o) * L + l] = acc[o];
  }
}

// (loss_commit: ral_device.hpp)
__global__ __launch_bounds__(256) void k_loss(const float* __restrict__ pred, const float* __restrict__ target,
                                              float* __restrict__ dy, float* __restrict__ snr,
                                              float* __restrict__ rmse, double* __restrict__ loss_sum, int n,
                                              float gscale, double* __restrict__ fin, double fin_scale, int fin3) {
  __shared__ double red[2 * 4];
  const size_t base = (size_t)blockIdx.x * n;
  float v[2] = {0.f, 0.f};
  for (int i = threadIdx.x; i < n; i += blockDim.x) {
    const float p = pred[base + i], t = target[base + i], d = p - t;
    v[0] += d * d;
    v[1] += t * t;
    if (dy) dy[base + i] = d * gscale;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float s0 = group_sum<64>(v[0]), s1 = group_sum<64>(v[1]);
  if (lane == 0) { red[wave * 2] = s0; red[wave * 2 + 1] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double sse = 0, sy2 = 0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { sse += red[w * 2]; sy2 += red[w * 2 + 1]; }
    const float mse = (float)(sse / n), my2 = (float)(sy2 / n);
    const float sn = 10.0f * log10f(my2 / mse), rm = sqrtf(mse);
    if (snr) snr[blockIdx.x] = sn;
    if (rmse) rmse[blockIdx.x] = rm;
    if (loss_sum) loss_commit(loss_sum, sse / n, fin, fin_scale, fin3, (double)sn, (double)rm);
  }
}

// The same reduction with one WAVE per window (n a multiple of 4): 16-byte loads, four of each operand in flight per lane,
// persistent workgroups (at most 512) that add their share of the loss with ONE atomic each - a workgroup per window
// was 2048 same-address double atomics in a row (~12 ns per link: most of the kernel's 30 us at batch 2048) on top of one
// memory round trip per 4-byte element.
#define LOSS_W_WAVES 8
__global__ __launch_bounds__(64 * LOSS_W_WAVES) void k_loss_w(const float* __restrict__ pred, const float* __restrict__ target,
                                                float* __restrict__ dy, float* __restrict__ snr,
                                                float* __restrict__ rmse, double* __restrict__ loss_sum, int n, int B,
                                                float gscale, double* __restrict__ fin, double fin_scale, int fin3) {
  __shared__ double red[3][LOSS_W_WAVES];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n4 = n >> 2;
  double mine = 0.0, msnr = 0.0, mrmse = 0.0;   // (lane 0: sums over this wave's windows of sse / n, SNR, RMSE)
  // a wave takes its windows two at a time: both windows' loads (up to 4 x 16 bytes per lane and operand, indices past the
  // end clamped) are requested before either is reduced - one memory round trip per pair
  const int stride = gridDim.x * LOSS_W_WAVES;
  for (int w = blockIdx.x * LOSS_W_WAVES + wave; w < B; w += 2 * stride) {
    const bool two = w + stride < B;
    const int wb = two ? w + stride : w;
    const float4* pa = reinterpret_cast<const float4*>(pred + (size_t)w * n);
    const float4* ta = reinterpret_cast<const float4*>(target + (size_t)w * n);
    const float4* pb = reinterpret_cast<const float4*>(pred + (size_t)wb * n);
    const float4* tb = reinterpret_cast<const float4*>(target + (size_t)wb * n);
    float4* da = dy ? reinterpret_cast<float4*>(dy + (size_t)w * n) : nullptr;
    float4* db = dy ? reinterpret_cast<float4*>(dy + (size_t)wb * n) : nullptr;
    float va0 = 0.f, va1 = 0.f, vb0 = 0.f, vb1 = 0.f;
    for (int i0 = 0; i0 < n4; i0 += 4 * 64) {
      float4 pav[4], tav[4], pbv[4], tbv[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 64 + lane, j = i < n4 ? i : 0;
        pav[k] = pa[j]; tav[k] = ta[j]; pbv[k] = pb[j]; tbv[k] = tb[j];
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = i0 + k * 64 + lane;
        if (i < n4) {
          const float4 d = f4sub(pav[k], tav[k]);
          va0 += f4dot(d, d); va1 += f4dot(tav[k], tav[k]);
          if (da) da[i] = f4scale(d, gscale);
          if (two) {
            const float4 e = f4sub(pbv[k], tbv[k]);
            vb0 += f4dot(e, e); vb1 += f4dot(tbv[k], tbv[k]);
            if (db) db[i] = f4scale(e, gscale);
          }
        }
      }
    }
    const float sa0 = group_sum<64>(va0), sa1 = group_sum<64>(va1), sb0 = group_sum<64>(vb0), sb1 = group_sum<64>(vb1);
    if (lane == 0) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 1 && !two) break;
        const double sse = (double)(h ? sb0 : sa0);
        const float mse = (float)(sse / n), my2 = (float)((double)(h ? sb1 : sa1) / n);
        const float sn = 10.0f * log10f(my2 / mse), rm = sqrtf(mse);
        const int ww = h ? wb : w;
        if (snr) snr[ww] = sn;
        if (rmse) rmse[ww] = rm;
        mine += sse / n; msnr += (double)sn; mrmse += (double)rm;
      }
    }
  }
  if (lane == 0) { red[0][wave] = mine; red[1][wave] = msnr; red[2][wave] = mrmse; }
  __syncthreads();
  if (threadIdx.x == 0 && loss_sum) {
    double t[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ((red[k][0] + red[k][1]) + (red[k][2] + red[k][3])) + ((red[k][4] + red[k][5]) + (red[k][6] + red[k][7]));
    loss_commit(loss_sum, t[0], fin, fin_scale, fin3, t[1], t[2]);
  }
}

// ---------------------------------------------------------------------------------
// fused flat Adam (torch.optim.Adam defaults, no weight decay / amsgrad)
// ---------------------------------------------------------------------------------
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, size_t n4, float step, float b1, float b2, float omb1, float omb2,
                       float eps, float sqrt_bc2, float gscale, double* __restrict__ zero64) {
  // (zero64: the 64 BatchNorm sums of the model, cleared here for the next step's stem: the last kernel of a step instead of a
  // fill kernel in front of the first one)
  if (zero64 && blockIdx.x == 0 && threadIdx.x < 64) zero64[threadIdx.x] = 0.0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    float4 pp = reinterpret_cast<float4*>(p)[i];
    const float4 gg = f4scale(reinterpret_cast<const float4*>(g)[i], gscale);
    float4 mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
#define UPD(f)                                              \
    mm.f = b1 * mm.f + omb1 * gg.f;                         \
    vv.f = b2 * vv.f + omb2 * gg.f * gg.f;                  \
    pp.f -= step * mm.f / (sqrtf(vv.f) / sqrt_bc2 + eps);
    UPD(x) UPD(y) UPD(z) UPD(w)
#undef UPD
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  }
}

// ---------------------------------------------------------------------------------
static inline int ew_grid(size_t n, int per = 256) {
  size_t g = (n + per - 1) / per;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

void launch_conv1_fwd(int leads, int mode, const float* x, const float* w, const float* b, float* out, double* stats,
                      const float* bnw, const float* bnb, const float* rmean, const float* rvar, int L, int Lp, int B,
                      hipStream_t s) {
  // training: every workgroup ends with 16 double atomics on the same 16 addresses (~15 ns per link of a same-address
  // chain): 4096 workgroups were a 56 us kernel for 38 MB of traffic, 512 are an 18 us one
  const int grid = ew_grid((size_t)B * Lp, mode == 0 ? 2048 : 256);
#define CASE(ld)                                                                                             \
  case ld:                                                                                                   \
    if (mode == 0) k_conv1_fwd<ld, 0><<<grid, 256, 0, s>>>(x, w, b, out, stats, bnw, bnb, rmean, rvar, L, Lp, B); \
    else k_conv1_fwd<ld, 1><<<grid, 256, 0, s>>>(x, w, b, out, stats, bnw, bnb, rmean, rvar, L, Lp, B);           \
    break;
  switch (leads) { CASE(1) CASE(2) }
#undef CASE
}

void launch_bn_train8(const double* stats, double count, const float* bnw, const float* bnb, float* ss, float* rmean, float* rvar,
                      const float* a0, float* x0, size_t ntok, hipStream_t s) {
  const int g = ew_grid(ntok * 2);
  k_bn_train8<<<g < 2048 ? g : 2048, 256, 0, s>>>(stats, count, bnw, bnb, ss, rmean, rvar, a0, x0, ntok);
}

void launch_final_fwd(int leads, const float* u0, const float* x0, const float* w, const float* b, float* y, int L, int Lp,
                      int B, hipStream_t s) {
  const int grid = ew_grid((size_t)B * L);
  if (leads == 1) k_final_fwd<1><<<grid, 256, 0, s>>>(u0, x0, w, b, y, L, Lp, B);
  else k_final_fwd<2><<<grid, 256, 0, s>>>(u0, x0, w, b, y, L, Lp, B);
}

static constexpr int LOSS_GRID = 256;   // workgroup cap of k_loss_w (measured below)
void launch_loss(const float* pred, const float* target, float* dy, float* snr, float* rmse, double* loss_sum,
                 int n, int B, float gscale, hipStream_t s, double* fin, double fin_scale, int fin3) {
  if (n % 4 == 0) {
    // (a workgroup ends with atomics on the same words - its share of the sum(s) and its arrival: at batch 2048 x 1024 floats
    // 512 four-wave workgroups were 19 us, 256 eight-wave ones 12.8 with two words in one cache line and 18.8 with four;
    // 128 / 64 workgroups: 13.8 / 13.1 - fewer links but half the CUs pulling the 24 MB.  256 and one line per word)
    const int g = (B + LOSS_W_WAVES - 1) / LOSS_W_WAVES;
    k_loss_w<<<g < LOSS_GRID ? g : LOSS_GRID, 64 * LOSS_W_WAVES, 0, s>>>(pred, target, dy, snr, rmse, loss_sum, n, B, gscale, fin, fin_scale, fin3);
  } else {
    k_loss<<<B, 256, 0, s>>>(pred, target, dy, snr, rmse, loss_sum, n, gscale, fin, fin_scale, fin3);
  }
}

// the three buffers a backward pass starts from, zeroed by ONE launch (they were three fill kernels of ~5 us, each with its launch
// gap, between the loss and the first backward kernel: nothing else runs there)
__global__ void k_zero_bwd(float4* __restrict__ grads, size_t n4, double* __restrict__ sums, int nsums, unsigned* __restrict__ gmax, int ngmax) {
  const size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (size_t i = i0; i < n4; i += (size_t)gridDim.x * blockDim.x) grads[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  if (i0 < (size_t)nsums) sums[i0] = 0.0;
  if (i0 < (size_t)ngmax) gmax[i0] = 0u;
}
void launch_zero_bwd(float* grads, size_t nfloat, double* sums, int nsums, unsigned* gmax, int ngmax, hipStream_t s) {
  k_zero_bwd<<<512, 256, 0, s>>>(reinterpret_cast<float4*>(grads), nfloat / 4, sums, nsums, gmax, ngmax);
}

void launch_adam(float* p, const float* g, float* m, float* v, size_t n, double lr, double b1, double b2, double eps,
                 int step, float gscale, hipStream_t s, double* zero64) {
  // scalars are formed in double on the host and rounded once, as torch.optim.Adam does
  const double bc1 = 1.0 - pow(b1, (double)step);
  const double bc2 = 1.0 - pow(b2, (double)step);
  k_adam<<<ew_grid(n / 4), 256, 0, s>>>(p, g, m, v, n / 4, (float)(lr / bc1), (float)b1, (float)b2, (float)(1.0 - b1),
                                        (float)(1.0 - b2), (float)eps, (float)sqrt(bc2), gscale, zero64);
}

// ---------------------------------------------------------------------------------
// 12-lead adapter convolutions (reference model/ralenet_12leads.py:683-709):
// Conv1d(cin, cout, k13, p6) [+ LeakyReLU(0.01)], channel-major (B, C, L).  One workgroup per window:
// input rows staged in LDS with a zero halo, weights in LDS.
// ---------------------------------------------------------------------------------
#define K13 13
__global__ __launch_bounds__(256) void k_conv13_fwd(const float* __restrict__ x, const float* __restrict__ w,
                                                    const float* __restrict__ bias, float* __restrict__ y, int B,
                                                    int cin, int cout, int L, int lrelu) {
  extern __shared__ float4 smem4[];
  float* xs = reinterpret_cast<float*>(smem4);  // cin x (L + 12)
  float* ws = xs + cin * (L + 12);              // cout x cin x 13
  const int LP = L + 12;
  for (int i = threadIdx.x; i < cout * cin * K13; i += blockDim.x) ws[i] = w[i];
  for (int win = blockIdx.x; win < B; win += gridDim.x) {
    __syncthreads();
    for (int i = threadIdx.x; i < cin * LP; i += blockDim.x) {
      const int c = i / LP, p = i - c * LP - 6;
      xs[i] = (p >= 0 && p < L) ? x[((size_t)win * cin + c) * L + p] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < cout * L; i += blockDim.x) {
      const int co = i / L, l = i - co * L;
      float acc = bias[co];
      for (int ci = 0; ci < cin; ++ci) {
        const float* wr = ws + (co * cin + ci) * K13;
        const float* xr = xs + ci * LP + l;
#pragma unroll
        for (int k = 0; k < K13; ++k) acc = fmaf(wr[k], xr[k], acc);
      }
      if (lrelu) acc = acc > 0.f ? acc : 0.01f * acc;
      y[((size_t)win * cout + co) * L + l] = acc;
    }
  }
}

// gradients: dz = dy * lrelu'(y);  dx = conv^T(dz);  gw += dz (*) x;  gb += sum dz
__global__ __launch_bounds__(256) void k_conv13_bwd(const float* __restrict__ x, const float* __restrict__ y,
                                                    const float* __restrict__ dy, const float* __restrict__ w,
                                                    float* __restrict__ gw, float* __restrict__ gb,
                                                    float* __restrict__ dx, int B, int cin, int cout, int L, int lrelu) {
  extern __shared__ float4 smem4[];
  const int LP = L + 12, nw = cout * cin * K13;
  float* xs = reinterpret_cast<float*>(smem4);  // cin x LP
  float* ds = xs + cin * LP;                    // cout x LP
  float* ws = ds + cout * LP;
  for (int i = threadIdx.x; i < nw; i += blockDim.x) ws[i] = w[i];
  float gacc[4] = {0.f, 0.f, 0.f, 0.f};          // 936 weight entries max / 256 threads
  float gbacc = 0.f;
  for (int win = blockIdx.x; win < B; win += gridDim.x) {
    __syncthreads();
    for (int i = threadIdx.x; i < cin * LP; i += blockDim.x) {
      const int c = i / LP, p = i - c * LP - 6;
      xs[i] = (p >= 0 && p < L) ? x[((size_t)win * cin + c) * L + p] : 0.f;
    }
    for (int i = threadIdx.x; i < cout * LP; i += blockDim.x) {
      const int c = i / LP, p = i - c * LP - 6;
      float g = 0.f;
      if (p >= 0 && p < L) {
        const size_t o = ((size_t)win * cout + c) * L + p;
        g = dy[o];
        if (lrelu && y[o] <= 0.f) g *= 0.01f;
      }
      ds[i] = g;
    }
    __syncthreads();
    if (dx) {
      for (int i = threadIdx.x; i < cin * L; i += blockDim.x) {
        const int ci = i / L, l = i - ci * L;
        float acc = 0.f;
        for (int co = 0; co < cout; ++co) {
          const float* wr = ws + (co * cin + ci) * K13;
          const float* dr = ds + co * LP + l + 12;   // dz[co][l + 6 - k] at padded index l + 12 - k
#pragma unroll
          for (int k = 0; k < K13; ++k) acc = fmaf(wr[k], dr[-k], acc);
        }
        dx[((size_t)win * cin + ci) * L + l] = acc;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = threadIdx.x + 256 * j;
      if (e < nw) {
        const int co = e / (cin * K13), ci = (e / K13) % cin, k = e % K13;
        const float* dr = ds + co * LP + 6;       // dz[co][l]
        const float* xr = xs + ci * LP + k;       // x[ci][l - 6 + k] at padded index l + k
        float s = 0.f;
        for (int l = 0; l < L; ++l) s = fmaf(dr[l], xr[l], s);
        gacc[j] += s;
      }
    }
    if ((int)threadIdx.x < cout) {
      const float* dr = ds + threadIdx.x * LP + 6;
      float s = 0.f;
      for (int l = 0; l < L; ++l) s += dr[l];
      gbacc += s;
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = threadIdx.x + 256 * j;
    if (e < nw) atomicAdd(gw + e, gacc[j]);
  }
  if ((int)threadIdx.x < cout) atomicAdd(gb + threadIdx.x, gbacc);
}

// what both launchers refuse before any HIP call (-> the offending argument, or nullptr): a request that fails here never
// reaches RAL_SET_LDS or the launch.  rows: LDS rows of L + 12 floats (cin forward, cin + cout backward)
static constexpr size_t CONV13_LDS_MAX = 160 * 1024;   // LDS of one gfx950 CU
static const char* conv13_refusal(int B, int cin, int cout, int L, int rows, size_t* lds) {
  if (cin < 1 || cout < 1 || cin > 12 || cout > 12 || cin * cout * K13 > 1024) return "unsupported channel counts";
  if (B < 1) return "B must be at least 1";
  if (L < 1) return "L must be at least 1";
  *lds = ((size_t)rows * ((size_t)L + 12) + (size_t)cout * cin * K13 + 4) * sizeof(float);
  if (*lds > CONV13_LDS_MAX) return "L needs more than the 160 KB of LDS";
  return nullptr;
}

int launch_conv13_fwd(const float* x, const float* w, const float* b, float* y, int B, int cin, int cout, int L,
                      int lrelu, hipStream_t s, const char** why) {
  size_t lds = 0;
  *why = !x ? "x is NULL" : !w ? "w is NULL" : !b ? "b is NULL" : !y ? "y is NULL" : conv13_refusal(B, cin, cout, L, cin, &lds);
  if (*why) return -1;
  RAL_SET_LDS(k_conv13_fwd, lds);
  k_conv13_fwd<<<B < 2048 ? B : 2048, 256, lds, s>>>(x, w, b, y, B, cin, cout, L, lrelu);
  return 0;
}

int launch_conv13_bwd(const float* x, const float* y, const float* dy, const float* w, float* gw, float* gb,
                      float* dx, int B, int cin, int cout, int L, int lrelu, hipStream_t s, const char** why) {
  size_t lds = 0;   // (dx is optional: NULL = no input gradient)
  *why = !x ? "x is NULL" : !y ? "y is NULL" : !dy ? "dy is NULL" : !w ? "w is NULL" : !gw ? "gw is NULL" : !gb ? "gb is NULL" :
         conv13_refusal(B, cin, cout, L, cin + cout, &lds);
  if (*why) return -1;
  RAL_SET_LDS(k_conv13_bwd, lds);
  k_conv13_bwd<<<B < 512 ? B : 512, 256, lds, s>>>(x, y, dy, w, gw, gb, dx, B, cin, cout, L, lrelu);
  return 0;
}

// ---------------------------------------------------------------------------------
// transposed copies of the weight matrices for the backward GEMMs (dX = dY W): with W^T row-major the
// A-operand fragment of those products is one 16-byte load, like in the forward pass
// ---------------------------------------------------------------------------------
__global__ void k_transpose_mats(const float* __restrict__ src, float* __restrict__ dst, const int4* __restrict__ desc,
                                 int nmat) {
  // desc[i] = (offset, rows, cols, first flat element index of this matrix in the launch)
  const int total = desc[nmat - 1].w + desc[nmat - 1].y * desc[nmat - 1].z;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    int lo = 0, hi = nmat - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (desc[mid].w <= e) lo = mid; else hi = mid - 1; }
    const int4 d = desc[lo];
    const int i = e - d.w, r = i / d.z, c = i - r * d.z;
    dst[d.x + c * d.y + r] = src[d.x + i];
  }
}

void launch_transpose_mats(const float* src, float* dst, const void* desc, int nmat, int total, hipStream_t s) {
  int grid = (total + 255) / 256;
  if (grid > 2048) grid = 2048;
  k_transpose_mats<<<grid, 256, 0, s>>>(src, dst, reinterpret_cast<const int4*>(desc), nmat);
}

// =================================================================================
// Record windowing + noise mixing in front of the model: one iteration of the reference's
// `batch_norm_snr_iter` (local_utils/local_utils.py:116-130) on the GPU --
//   clean = np_norm(segment, dim=0)                (per-lead z-score over the whole segment, population std, :261-266)
//   noisy = clean + sqrt(P_clean / 10^(snr/10) / P_noise) * noise      (`Gnoisegen`, :86-114)
//   '(b l) c -> b c l' windows of L samples, fp32
// Statistics are double sums (like the reference's float64 numpy arithmetic); the element-wise pass works in double and
// rounds once, so outputs equal the reference's `torch.FloatTensor(...)` casts up to the summation order of the sums.
// Both kernels are one HBM pass: (T, leads) row-major in, channel-major windows out.
// =================================================================================
#define RAL_PREP_MAXL 16
__global__ __launch_bounds__(256) void k_prep_stats(const float* __restrict__ sig, const float* __restrict__ noise,
                                                    long long T, int leads, double* __restrict__ sums) {
  __shared__ double red[2 * RAL_PREP_MAXL + 1];
  for (int i = threadIdx.x; i < 2 * leads + 1; i += blockDim.x) red[i] = 0.0;
  __syncthreads();
  double sx[RAL_PREP_MAXL], sxx[RAL_PREP_MAXL], snn = 0.0;
#pragma unroll
  for (int c = 0; c < RAL_PREP_MAXL; ++c) { sx[c] = 0.0; sxx[c] = 0.0; }
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < T; t += (long long)gridDim.x * blockDim.x) {
#pragma unroll
    for (int c = 0; c < RAL_PREP_MAXL; ++c) {
      if (c < leads) {
        const double x = sig[t * leads + c], n = noise[t * leads + c];
        sx[c] += x; sxx[c] += x * x; snn += n * n;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < RAL_PREP_MAXL; ++c) {
    if (c < leads) { atomicAdd(&red[c], sx[c]); atomicAdd(&red[leads + c], sxx[c]); }
  }
  atomicAdd(&red[2 * leads], snn);
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * leads + 1; i += blockDim.x) atomicAdd(sums + i, red[i]);
}

__global__ __launch_bounds__(256) void k_prep_mix(const float* __restrict__ sig, const float* __restrict__ noise,
                                                  const double* __restrict__ sums, long long T, int leads, int L,
                                                  double snr_db, float* __restrict__ noisy, float* __restrict__ clean) {
  // P_clean = sum(clean^2) / T = leads (every lead has unit population variance); P_noise = sum(noise^2) / T
  const double scale = sqrt((double)leads / pow(10.0, snr_db / 10.0) / (sums[2 * leads] / (double)T));
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < T; t += (long long)gridDim.x * blockDim.x) {
    const long long b = t / L;
    const int l = (int)(t - b * L);
    for (int c = 0; c < leads; ++c) {
      const double mean = sums[c] / (double)T;
      const double var = sums[leads + c] / (double)T - mean * mean;
      const double xn = ((double)sig[t * leads + c] - mean) / sqrt(var);
      const size_t o = ((size_t)b * leads + c) * L + l;
      clean[o] = (float)xn;
      noisy[o] = (float)(xn + scale * (double)noise[t * leads + c]);
    }
  }
}

int launch_prep_windows(const float* sig, const float* noise, long long T, int leads, int L, double snr_db, double* sums,
                        float* noisy, float* clean, hipStream_t s) {
  if (leads < 1 || leads > RAL_PREP_MAXL || L < 1 || T < L || T % L != 0) return -1;
  (void)hipMemsetAsync(sums, 0, (2 * leads + 1) * sizeof(double), s);
  const int grid = (int)((T + 255) / 256 < 2048 ? (T + 255) / 256 : 2048);
  k_prep_stats<<<grid, 256, 0, s>>>(sig, noise, T, leads, sums);
  k_prep_mix<<<grid, 256, 0, s>>>(sig, noise, sums, T, leads, L, snr_db, noisy, clean);
  return 0;
}

// =================================================================================
// Streaming of long records around the inference forward (BASELINE config 5).  The reference cuts the
// 650 000-sample MIT-BIH records into fixed chunks and z-scores them (local_utils/local_utils.py:116-130, np_norm
// :261-266); here a group of R records (R, leads, T) is cut into windows of L samples every `hop` samples (the last
// window of a record is right-aligned), every window is z-scored per lead, and after the model the windows are
// de-normalised and stitched back: overlapping regions keep the centre of each window, the record edges keep the
// whole window.  One wave per (window, lead); mean and standard deviation go to a side buffer for the way back.
// =================================================================================
RAL_DEV void stream_geom(long long T, int L, int hop, int& n_reg, int& n) {
  n_reg = (int)((T - L) / hop) + 1;
  n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
}

// The stitch rule: which window keeps which samples of its record.  h = (L - hop) / 2; window 0 keeps [0, hop + h), window k
// [k hop + h, (k + 1) hop + h), the last window [last_begin, T) (a single window keeps the whole record).  The kept ranges are
// disjoint and cover [0, T): k_stream_stitch maps a sample to its window (stream_owner), k_newrale_back and k_live_emit a window
// to its samples (stream_kept).
struct StreamKeep {
  int n_reg, n, h;
  long long last_begin;   // first sample the last window keeps
};
RAL_DEV StreamKeep stream_keep(long long T, int L, int hop) {
  StreamKeep s;
  stream_geom(T, L, hop, s.n_reg, s.n);
  s.h = (L - hop) >> 1;
  s.last_begin = s.n > 1 ? (long long)(s.n - 2) * hop + L - s.h : 0;
  return s;
}
// A live stream whose end T is not known yet: every window is regular and none is the last (n = n_reg = INT_MAX), so
// stream_start and stream_kept answer for window k < INT_MAX - 1 without reading T.
RAL_DEV StreamKeep stream_keep_open(int L, int hop) {
  StreamKeep s;
  s.n_reg = s.n = 0x7fffffff;
  s.h = (L - hop) >> 1;
  s.last_begin = 0;
  return s;
}
RAL_DEV long long stream_start(const StreamKeep& s, int k, long long T, int L, int hop) {   // first sample of window k
  return k < s.n_reg ? (long long)k * hop : T - L;
}
RAL_DEV int stream_owner(const StreamKeep& s, long long t, int hop) {
  if (s.n == 1 || t >= s.last_begin) return s.n - 1;
  return t < s.h ? 0 : (int)((t - s.h) / hop);
}
RAL_DEV void stream_kept(const StreamKeep& s, int k, long long T, int hop, long long& b, long long& e) {
  b = k == 0 ? 0 : (k == s.n - 1 ? s.last_begin : (long long)k * hop + s.h);
  e = k == s.n - 1 ? T : (long long)(k + 1) * hop + s.h;
}

// The z-score of one lead of one window by one wave (lane = threadIdx.x & 63), src(l) its samples l in [0, L): mean, population
// std with a floor of 1e-6 (as np_norm; constant leads stay finite), dst[l] = (src(l) - mean) / std.  src may read dst.  Every
// window gather (k_stream_windows, k_live_windows, k_newrale_front) runs these sums, so they all produce the same bits.
template <class Src>
RAL_DEV void zscore_wave(const Src& src, float* dst, int L, float& mean, float& sd) {
  const int lane = threadIdx.x & 63;
  float sum = 0.f;
  for (int l = lane; l < L; l += 64) sum += src(l);
  mean = group_sum<64>(sum) / (float)L;
  float ss = 0.f;
  for (int l = lane; l < L; l += 64) { const float d = src(l) - mean; ss = fmaf(d, d, ss); }   // (second pass: L1 hits)
  sd = fmaxf(sqrtf(group_sum<64>(ss) / (float)L), 1e-6f);
  const float inv = 1.0f / sd;
  for (int l = lane; l < L; l += 64) dst[l] = (src(l) - mean) * inv;
}

__global__ __launch_bounds__(64) void k_stream_windows(const float* __restrict__ rec, long long T, int leads, int L, int hop,
                                                       long long w0, float* __restrict__ win, float* __restrict__ stats) {
  int n_reg, n;
  stream_geom(T, L, hop, n_reg, n);
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;   // window of this launch, lead
  const long long gw = w0 + i;
  const long long r = gw / n;
  const int k = (int)(gw - r * n);
  const long long start = k < n_reg ? (long long)k * hop : T - L;
  const float* src = rec + (r * leads + c) * T + start;
  float mean, sd;
  zscore_wave([=](int l) { return src[l]; }, win + ((size_t)i * leads + c) * L, L, mean, sd);
  if (threadIdx.x == 0) { stats[(gw * leads + c) * 2] = mean; stats[(gw * leads + c) * 2 + 1] = sd; }
}

__global__ __launch_bounds__(256) void k_stream_stitch(const float* __restrict__ y, const float* __restrict__ stats, long long R,
                                                       long long T, int leads, int L, int hop, float* __restrict__ out) {
  const StreamKeep sk = stream_keep(T, L, hop);
  const long long total = R * leads * T;
  for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const long long rc = e / T, t = e - rc * T;
    const long long r = rc / leads;
    const int c = (int)(rc - r * leads);
    const int k = stream_owner(sk, t, hop);
    const long long off = t - stream_start(sk, k, T, L, hop);
    const long long gw = r * sk.n + k;
    const float mean = stats[(gw * leads + c) * 2], sd = stats[(gw * leads + c) * 2 + 1];
    out[e] = fmaf(y[(gw * leads + c) * L + off], sd, mean);
  }
}

int launch_stream_windows(const float* rec, long long R, long long T, int leads, int L, int hop, long long w0, int nw,
                          float* win, float* stats, hipStream_t s) {
  if (R < 1 || leads < 1 || L < 64 || L % 64 != 0 || L > 2048 || T < L || hop < 1 || hop > L || nw < 1 || w0 < 0) return -1;
  const long long n_reg = (T - L) / hop + 1, n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
  if (w0 + nw > R * n) return -1;
  k_stream_windows<<<nw * leads, 64, 0, s>>>(rec, T, leads, L, hop, w0, win, stats);
  return 0;
}

int launch_stream_stitch(const float* y, const float* stats, long long R, long long T, int leads, int L, int hop, float* out,
                         hipStream_t s) {
  if (R < 1 || leads < 1 || T < L || hop < 1 || hop > L || ((L - hop) & 1)) return -1;
  const long long total = R * leads * T;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  k_stream_stitch<<<grid, 256, 0, s>>>(y, stats, R, T, leads, L, hop, out);
  return 0;
}

// =================================================================================
// Live streams (LiveDenoiser, infer.py): S streams advance in lockstep by a chunk of C samples.  A stream keeps the last L
// samples it has received, `hist` (S, leads, L); with the chunk `x` (S, leads, C) they form V = hist ++ x, samples
// [base, base + L + C) of the stream (base = samples received before the chunk - L; positions below 0 are never read).  The
// windows are those of the offline path (stream_keep: T >= 0, the stream ends at T; stream_keep_open: T < 0, the end is not
// known), numbered as there: the windows k0 .. k0 + nw - 1 of every stream, all inside V, are window gw = s nw + j of a call.
// k_live_windows gathers them straight from hist and x and z-scores them (zscore_wave); its workgroups past the windows
// write the last L samples of V to hist_out (another buffer than hist: no workgroup reads what another one writes).
// k_live_emit de-normalises the model output and writes the samples [lo, lo + m) of the stream that the windows keep
// (stream_kept) into out (S, leads, m).  Both take absolute positions; with T < 0 and k0 > 0 their results depend only on
// positions relative to base, so a captured push serves every later push that advances by a multiple of hop.
// =================================================================================
__global__ __launch_bounds__(64) void k_live_windows(const float* __restrict__ hist, const float* __restrict__ x,
                                                     float* __restrict__ hist_out, int leads, int L, int hop, int C,
                                                     long long base, int k0, int nw, long long T, long long w0, int nb,
                                                     float* __restrict__ win, float* __restrict__ stats) {
  const int nwl = nb * leads;
  if ((int)blockIdx.x >= nwl) {   // the history of one (stream, lead): V[C, C + L)
    const size_t sc = blockIdx.x - nwl;
    const float* hr = hist + sc * L;
    const float* xr = x + sc * C;
    float* dst = hist_out + sc * L;
    for (int l = threadIdx.x; l < L; l += 64) dst[l] = C + l < L ? hr[C + l] : xr[C + l - L];
    return;
  }
  const StreamKeep sk = T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop);
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;   // window of this launch, lead
  const long long gw = w0 + i;
  const long long s = gw / nw;
  const int j = (int)(gw - s * nw);
  const int o = (int)(stream_start(sk, k0 + j, T, L, hop) - base);   // the window is V[o, o + L)
  const float* hr = hist + (s * leads + c) * L;
  const float* xr = x + (s * leads + c) * C - L;
  float mean, sd;
  zscore_wave([=](int l) { const int v = o + l; return v < L ? hr[v] : xr[v]; }, win + ((size_t)i * leads + c) * L, L, mean, sd);
  if (threadIdx.x == 0) { stats[(gw * leads + c) * 2] = mean; stats[(gw * leads + c) * 2 + 1] = sd; }
}

// y (nb, leads, L): the model output for windows [w0, w0 + nb) of the call; last_y / last_stats (optional): window j = nw - 1
// of every stream is also kept whole, (S, leads, L) and (S, leads, 2), for a later call with T known.
__global__ __launch_bounds__(64) void k_live_emit(const float* __restrict__ y, const float* __restrict__ stats, int leads, int L,
                                                  int hop, int k0, int nw, long long T, long long w0, long long lo, int m,
                                                  float* __restrict__ out, float* __restrict__ last_y,
                                                  float* __restrict__ last_stats) {
  const StreamKeep sk = T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop);
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;
  const long long gw = w0 + i;
  const long long s = gw / nw;
  const int j = (int)(gw - s * nw), k = k0 + j;
  const long long start = stream_start(sk, k, T, L, hop);
  long long b, e;
  stream_kept(sk, k, T, hop, b, e);
  b = b > lo ? b : lo;                   // (the kept range lies inside the window: stream_kept; clipped to it all the same)
  b = b > start ? b : start;
  e = e < lo + m ? e : lo + m;
  e = e < start + L ? e : start + L;
  const float mean = stats[(gw * leads + c) * 2], sd = stats[(gw * leads + c) * 2 + 1];
  const float* yr = y + ((size_t)i * leads + c) * L;
  float* dst = out + (s * leads + c) * m - lo;
  for (long long t = b + threadIdx.x; t < e; t += 64) dst[t] = fmaf(yr[t - start], sd, mean);
  if (last_y && j == nw - 1) {
    float* ly = last_y + (s * leads + c) * L;
    for (int l = threadIdx.x; l < L; l += 64) ly[l] = yr[l];
    if (threadIdx.x == 0) { last_stats[(s * leads + c) * 2] = mean; last_stats[(s * leads + c) * 2 + 1] = sd; }
  }
}

// The host side of the same geometry (stream_geom / stream_start), for argument checks: window k of a stream ending at T (T < 0:
// open) starts at *start; false if there is no window k.
static bool live_window_start(long long T, int L, int hop, long long k, long long& start) {
  if (T < 0) { start = k * hop; return k < 0x7ffffffeLL; }
  const long long n_reg = (T - L) / hop + 1, n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
  start = k < n_reg ? k * hop : T - L;
  return k < n && n < 0x7fffffffLL;
}

// lmul / lmax: the window lengths of the caller's kernels (L a multiple of lmul in [lmul, lmax])
static bool live_geom_ok(long long S, int leads, int L, int hop, long long k0, int nw, long long T, long long w0, int nb,
                         int lmul = 64, int lmax = 2048) {
  if (S < 1 || leads < 1 || L < lmul || L % lmul != 0 || L > lmax || hop < 1 || hop > L || ((L - hop) & 1)) return false;
  if (nw < 0 || k0 < 0 || nb < 0 || w0 < 0 || (T >= 0 && T < L) || w0 + nb > S * nw) return false;
  long long st;
  return nw == 0 || live_window_start(T, L, hop, k0 + nw - 1, st);
}

// every window k0 .. k0 + nw - 1 inside V: the first one starts at or after base, the last one ends at or before base + L + C
static bool live_windows_in_v(int L, int hop, int C, long long base, long long k0, int nw, long long T) {
  if (nw == 0) return true;
  long long first, last;
  live_window_start(T, L, hop, k0, first);
  live_window_start(T, L, hop, k0 + nw - 1, last);
  return first >= base && last + L <= base + L + C;
}

int launch_live_windows(const float* hist, const float* x, float* hist_out, long long S, int leads, int L, int hop, int C,
                        long long base, long long k0, int nw, long long T, long long w0, int nb, float* win, float* stats,
                        hipStream_t s) {
  if (!live_geom_ok(S, leads, L, hop, k0, nw, T, w0, nb) || C < 0 || (nb == 0 && !hist_out)) return -1;
  if (!live_windows_in_v(L, hop, C, base, k0, nw, T)) return -1;
  const long long grid = (long long)nb * leads + (hist_out ? S * leads : 0);
  if (grid > 0x7fffffffLL) return -1;
  k_live_windows<<<(int)grid, 64, 0, s>>>(hist, x, hist_out, leads, L, hop, C, base, (int)k0, nw, T, w0, nb, win, stats);
  return 0;
}

int launch_live_emit(const float* y, const float* stats, long long S, int leads, int L, int hop, long long k0, int nw, long long T,
                     long long w0, int nb, long long lo, int m, float* out, float* last_y, float* last_stats, hipStream_t s) {
  if (!live_geom_ok(S, leads, L, hop, k0, nw, T, w0, nb) || nb < 1 || lo < 0 || m < 0 || (!last_y != !last_stats)) return -1;
  if ((long long)nb * leads > 0x7fffffffLL) return -1;
  k_live_emit<<<nb * leads, 64, 0, s>>>(y, stats, leads, L, hop, (int)k0, nw, T, w0, lo, m, out, last_y, last_stats);
  return 0;
}

// =================================================================================
// Record streaming through the 12-lead adapter (NewRALE, reference model/ralenet_12leads.py:698-709): the steps around the
// inner RA-LENet as two kernels.  k_newrale_front: window gather + per-lead z-score (k_stream_windows' arithmetic) + conv1
// (12 -> 6) + conv2 (6 -> 2) -> the inner model's input (nw, 2, L).  k_newrale_back: conv3 (2 -> 6) + conv4 (6 -> 12) +
// de-normalisation, written straight into the record for the samples the window keeps (k_stream_stitch's rule).
// One workgroup per window, the whole window staged in LDS with a 6-sample zero halo on each row (the Conv1d padding of
// every adapter conv): at L = 1024 the front kernel holds 12 + 6 rows of 1036 floats (75 KB, two workgroups per CU), the
// back kernel 2 + 6 rows (33 KB).  Every thread computes 4 consecutive samples of every output channel from a 16-sample
// register window per input row; the weights are wave-uniform loads from the parameter buffer.  The sums run in
// k_conv13_fwd's order (bias, then input channel, then tap), so the results equal the unfused launches.
// =================================================================================
#define NR_LEADS 12
#define NR_MID 6
#define NR_PT 4   // consecutive output samples per thread
// offsets in the adapter's flat parameter buffer (NewRALE.SHAPES, every tensor padded to a multiple of 4 floats)
#define NR_C1W 0
#define NR_C1B 936
#define NR_C2W 944
#define NR_C2B 1100
#define NR_C3W 1104
#define NR_C3B 1260
#define NR_C4W 1268
#define NR_C4B 2204

// acc[co][p] = b[co] + sum_ci sum_k w[(co CIN + ci) 13 + k] * xs[ci LP + l0 + p + k]: output samples l0 .. l0 + 3 of a
// Conv1d(CIN, COUT, k13, p6) whose input rows (stride LP) carry a 6-sample halo in front (l0 % 4 == 0, LP % 4 == 0)
template <int CIN, int COUT>
RAL_DEV void conv13_tile(const float* __restrict__ xs, int LP, int l0, const float* __restrict__ w, const float* __restrict__ b,
                         float (&acc)[COUT][NR_PT]) {
#pragma unroll
  for (int co = 0; co < COUT; ++co)
#pragma unroll
    for (int p = 0; p < NR_PT; ++p) acc[co][p] = b[co];
  for (int ci = 0; ci < CIN; ++ci) {
    float xr[NR_PT + 12];
    const float4* xv = reinterpret_cast<const float4*>(xs + ci * LP + l0);
#pragma unroll
    for (int j = 0; j < (NR_PT + 12) / 4; ++j) {
      const float4 v = xv[j];
      xr[4 * j] = v.x; xr[4 * j + 1] = v.y; xr[4 * j + 2] = v.z; xr[4 * j + 3] = v.w;
    }
#pragma unroll
    for (int co = 0; co < COUT; ++co)
#pragma unroll
      for (int k = 0; k < K13; ++k) {
        const float wk = w[(co * CIN + ci) * K13 + k];
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) acc[co][p] = fmaf(wk, xr[p + k], acc[co][p]);
      }
  }
}

RAL_DEV float lrelu001(float v) { return v > 0.f ? v : 0.01f * v; }

// zero the halo columns [0, 6) and [L + 6, L + 12) of `rows` rows of stride L + 12 (the window loops write the interiors only)
RAL_DEV void zero_halos(float* xs, int rows, int L) {
  for (int i = threadIdx.x; i < rows * 12; i += blockDim.x) {
    const int row = i / 12, j = i - row * 12;
    xs[row * (L + 12) + (j < 6 ? j : L + j)] = 0.f;
  }
}

// The record kernels and the live ones are ONE body each, templated on where a window comes from (k_newrale_front) and where
// its kept samples go (k_newrale_back): the live bits equal the record bits by construction.
// Window sources: window(sk, i, src) returns the number gw of window i of the launch (its stats slot) and sets the reader
// src(c, l) of its sample l of lead c; write_history is what the workgroups past the windows do (live calls only).
struct NrRecordWindows {   // windows [w0, w0 + nw) of a record group (R, 12, T), numbered as in k_stream_windows
  const float* rec;
  long long T, w0;
  int L, hop;
  struct Reader {
    const float* p;
    long long T;
    RAL_DEV float operator()(int c, int l) const { return p[c * T + l]; }
  };
  RAL_DEV StreamKeep keep() const { return stream_keep(T, L, hop); }
  RAL_DEV long long window(const StreamKeep& sk, int i, Reader& src) const {
    const long long gw = w0 + i, r = gw / sk.n;
    const int k = (int)(gw - r * sk.n);
    src.p = rec + r * NR_LEADS * T + stream_start(sk, k, T, L, hop);
    src.T = T;
    return gw;
  }
  RAL_DEV void write_history(int, int) const {}
};

struct NrLiveWindows {     // a live call (k_live_windows' geometry, 12 leads): window gw = s nw + j is window k0 + j of stream s
  const float* hist;       // (S, 12, L)
  const float* x;          // (S, 12, C)
  float* hist_out;         // (S, 12, L) or null
  long long S, base, T, w0;
  int L, hop, C, k0, nw;
  struct Reader {          // the window is V[o, o + L) of V = hist ++ x
    const float* hr;
    const float* xr;
    int o, L, C;
    RAL_DEV float operator()(int c, int l) const { const int v = o + l; return v < L ? hr[c * L + v] : xr[c * C + v]; }
  };
  RAL_DEV StreamKeep keep() const { return T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop); }
  RAL_DEV long long window(const StreamKeep& sk, int i, Reader& src) const {
    const long long gw = w0 + i, s = gw / nw;
    const int j = (int)(gw - s * nw);
    src.o = (int)(stream_start(sk, k0 + j, T, L, hop) - base);
    src.hr = hist + s * NR_LEADS * L;
    src.xr = x + s * NR_LEADS * C - L;
    src.L = L;
    src.C = C;
    return gw;
  }
  // workgroup g of ng writes V[C, C + L) of the (stream, lead) rows g, g + ng, ... into hist_out (another buffer than hist)
  RAL_DEV void write_history(int g, int ng) const {
    for (long long r = g; r < S * NR_LEADS; r += ng) {
      const float* hr = hist + r * L;
      const float* xr = x + r * C;
      float* dst = hist_out + r * L;
      for (int l = threadIdx.x; l < L; l += blockDim.x) dst[l] = C + l < L ? hr[C + l] : xr[C + l - L];
    }
  }
};

// Where the kept samples of a window of k_newrale_back go: window(sk, i) -> its number gw, the samples [ob, oe) of the window
// it keeps, and the element out[dst + c * stride + l] that takes its sample l of lead c; src: where its inner output is read
// (window i of the launch at i * 2 L, a pool's kept window at its slot); ly: where the inner output of the window is kept
// whole (live calls, the last window of every stream), or null.
struct NrKept {
  long long gw, dst, stride;
  long long src;           // the window's inner output is iy[src, src + 2 L)
  int ob, oe;
  float* ly;
};

struct NrRecordKeep {      // into the record group (R, 12, T): k_stream_stitch's rule
  float* out;
  long long T, w0;
  int L, hop;
  RAL_DEV StreamKeep keep() const { return stream_keep(T, L, hop); }
  RAL_DEV NrKept window(const StreamKeep& sk, int i) const {
    NrKept kp;
    kp.gw = w0 + i;
    const long long r = kp.gw / sk.n;
    const int k = (int)(kp.gw - r * sk.n);
    const long long start = stream_start(sk, k, T, L, hop);
    long long kb, ke;
    stream_kept(sk, k, T, hop, kb, ke);
    kp.ob = (int)(kb - start);
    kp.oe = (int)(ke - start);
    kp.dst = r * NR_LEADS * T + start;
    kp.stride = T;
    kp.src = (long long)i * 2 * L;
    kp.ly = nullptr;
    return kp;
  }
  RAL_DEV void keep_stats(const NrKept&, const float*) const {}
};

struct NrLiveKeep {        // into a live call's out (S, 12, m): the samples in [lo, lo + m), sample t at t - lo (k_live_emit)
  float* out;
  float* last_y;           // (S, 2, L) or null
  float* last_stats;       // (S, 12, 2) or null (with last_y)
  long long T, w0, lo;
  int L, hop, k0, nw, m;
  RAL_DEV StreamKeep keep() const { return T < 0 ? stream_keep_open(L, hop) : stream_keep(T, L, hop); }
  RAL_DEV NrKept window(const StreamKeep& sk, int i) const {
    NrKept kp;
    kp.gw = w0 + i;
    const long long s = kp.gw / nw;
    const int j = (int)(kp.gw - s * nw), k = k0 + j;
    const long long start = stream_start(sk, k, T, L, hop);
    long long b, e;
    stream_kept(sk, k, T, hop, b, e);
    b = b > lo ? b : lo;                 // (clipped to the window as in k_live_emit)
    b = b > start ? b : start;
    e = e < lo + m ? e : lo + m;
    e = e < start + L ? e : start + L;
    kp.ob = (int)(b - start);
    kp.oe = e > b ? (int)(e - start) : kp.ob;
    kp.dst = s * NR_LEADS * m + start - lo;   // (negative for start < lo: only l >= ob, t >= lo, is written)
    kp.stride = m;
    kp.src = (long long)i * 2 * L;
    kp.ly = last_y && j == nw - 1 ? last_y + s * 2 * L : nullptr;
    return kp;
  }
  RAL_DEV void keep_stats(const NrKept& kp, const float* stats) const {   // (mean, std) of the 12 leads of a kept window
    if (kp.ly && threadIdx.x < 2 * NR_LEADS)
      last_stats[(kp.gw / nw) * 2 * NR_LEADS + threadIdx.x] = stats[kp.gw * 2 * NR_LEADS + threadIdx.x];
  }
};

// nwg workgroups take the windows [0, nw) of the launch in turn; workgroups nwg .. gridDim.x - 1 write the history
template <class Win>
__global__ __launch_bounds__(256) void k_newrale_front(Win win, int nw, int nwg, const float* __restrict__ prm,
                                                       float* __restrict__ inner, float* __restrict__ stats) {
  if ((int)blockIdx.x >= nwg) {
    win.write_history((int)blockIdx.x - nwg, (int)gridDim.x - nwg);
    return;
  }
  extern __shared__ float4 smem4[];
  const int L = win.L, LP = L + 12;
  float* xs = reinterpret_cast<float*>(smem4);   // 12 x LP: the window, z-scored in place
  float* a1 = xs + NR_LEADS * LP;                // 6 x LP: conv1's output
  zero_halos(xs, NR_LEADS + NR_MID, L);
  const StreamKeep sk = win.keep();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int i = blockIdx.x; i < nw; i += nwg) {
    typename Win::Reader src;
    const long long gw = win.window(sk, i, src);
    __syncthreads();   // (the previous window's readers are done; the halos are written)
    for (int e = threadIdx.x; e < NR_LEADS * L; e += blockDim.x) {
      const int c = e / L, l = e - c * L;
      xs[c * LP + 6 + l] = src(c, l);
    }
    __syncthreads();
    // z-score, one wave per lead (zscore_wave: k_stream_windows' bits)
    for (int c = wave; c < NR_LEADS; c += blockDim.x >> 6) {
      float* row = xs + c * LP + 6;
      float mean, sd;
      zscore_wave([=](int l) { return row[l]; }, row, L, mean, sd);
      if (lane == 0) { stats[(gw * NR_LEADS + c) * 2] = mean; stats[(gw * NR_LEADS + c) * 2 + 1] = sd; }
    }
    __syncthreads();
    for (int l0 = NR_PT * threadIdx.x; l0 < L; l0 += NR_PT * blockDim.x) {   // conv1 + LeakyReLU -> a1
      float acc[NR_MID][NR_PT];
      conv13_tile<NR_LEADS, NR_MID>(xs, LP, l0, prm + NR_C1W, prm + NR_C1B, acc);
#pragma unroll
      for (int co = 0; co < NR_MID; ++co)
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) a1[co * LP + 6 + l0 + p] = lrelu001(acc[co][p]);
    }
    __syncthreads();
    for (int l0 = NR_PT * threadIdx.x; l0 < L; l0 += NR_PT * blockDim.x) {   // conv2 + LeakyReLU -> inner (nw, 2, L)
      float acc[2][NR_PT];
      conv13_tile<NR_MID, 2>(a1, LP, l0, prm + NR_C2W, prm + NR_C2B, acc);
#pragma unroll
      for (int co = 0; co < 2; ++co)
        *reinterpret_cast<float4*>(inner + ((size_t)i * 2 + co) * L + l0) =
            make_float4(lrelu001(acc[co][0]), lrelu001(acc[co][1]), lrelu001(acc[co][2]), lrelu001(acc[co][3]));
    }
  }
}

template <class Dst>
__global__ __launch_bounds__(256) void k_newrale_back(Dst dst, int nw, const float* __restrict__ iy,
                                                      const float* __restrict__ stats, const float* __restrict__ prm) {
  extern __shared__ float4 smem4[];
  const int L = dst.L, LP = L + 12;
  float* ys = reinterpret_cast<float*>(smem4);   // 2 x LP: the inner model's output
  float* a3 = ys + 2 * LP;                       // 6 x LP: conv3's output
  zero_halos(ys, 2 + NR_MID, L);
  const StreamKeep sk = dst.keep();
  for (int i = blockIdx.x; i < nw; i += gridDim.x) {
    const NrKept kp = dst.window(sk, i);
    const long long gw = kp.gw;
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * L; e += blockDim.x) {
      const int c = e / L, l = e - c * L;
      const float v = iy[kp.src + e];
      ys[c * LP + 6 + l] = v;
      if (kp.ly) kp.ly[e] = v;
    }
    dst.keep_stats(kp, stats);
    __syncthreads();
    for (int l0 = NR_PT * threadIdx.x; l0 < L; l0 += NR_PT * blockDim.x) {   // conv3 + LeakyReLU -> a3
      float acc[NR_MID][NR_PT];
      conv13_tile<2, NR_MID>(ys, LP, l0, prm + NR_C3W, prm + NR_C3B, acc);
#pragma unroll
      for (int co = 0; co < NR_MID; ++co)
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) a3[co * LP + 6 + l0 + p] = lrelu001(acc[co][p]);
    }
    __syncthreads();
    // conv4 on the 4-sample tiles that hold kept samples; de-normalise; write the kept ones
    for (int l0 = (kp.ob & ~(NR_PT - 1)) + NR_PT * threadIdx.x; l0 < kp.oe; l0 += NR_PT * blockDim.x) {
      float acc[NR_LEADS][NR_PT];
      conv13_tile<NR_MID, NR_LEADS>(a3, LP, l0, prm + NR_C4W, prm + NR_C4B, acc);
#pragma unroll
      for (int c = 0; c < NR_LEADS; ++c) {
        const float mean = stats[(gw * NR_LEADS + c) * 2], sd = stats[(gw * NR_LEADS + c) * 2 + 1];
#pragma unroll
        for (int p = 0; p < NR_PT; ++p) {
          const int l = l0 + p;
          if (l >= kp.ob && l < kp.oe) dst.out[kp.dst + c * kp.stride + l] = fmaf(acc[c][p], sd, mean);
        }
      }
    }
  }
}

static constexpr int NR_GRID = 2048;   // workgroup cap of the windows of one launch (grid-stride beyond)
static size_t newrale_front_lds(int L) { return (size_t)(NR_LEADS + NR_MID) * (L + 12) * sizeof(float); }
static size_t newrale_back_lds(int L) { return (size_t)(2 + NR_MID) * (L + 12) * sizeof(float); }

static bool newrale_stream_args_ok(long long R, long long T, int L, int hop, long long w0, int nw) {
  if (R < 1 || L < 16 || L % 16 != 0 || L > 1024 || T < L || hop < 1 || hop > L || ((L - hop) & 1) || nw < 1 || w0 < 0) return false;
  const long long n_reg = (T - L) / hop + 1, n = n_reg + (((T - L) % hop) != 0 ? 1 : 0);
  return n <= 0x7fffffffLL && w0 + nw <= R * n;
}

int launch_newrale_front(const float* rec, long long R, long long T, int L, int hop, long long w0, int nw, const float* prm,
                         float* inner, float* stats, hipStream_t s) {
  if (!newrale_stream_args_ok(R, T, L, hop, w0, nw)) return -1;
  const size_t lds = newrale_front_lds(L);
  RAL_SET_LDS(k_newrale_front<NrRecordWindows>, lds);
  const int grid = nw < NR_GRID ? nw : NR_GRID;
  k_newrale_front<<<grid, 256, lds, s>>>(NrRecordWindows{rec, T, w0, L, hop}, nw, grid, prm, inner, stats);
  return 0;
}

int launch_newrale_back(const float* iy, const float* stats, const float* prm, long long R, long long T, int L, int hop,
                        long long w0, int nw, float* out, hipStream_t s) {
  if (!newrale_stream_args_ok(R, T, L, hop, w0, nw)) return -1;
  const size_t lds = newrale_back_lds(L);
  RAL_SET_LDS(k_newrale_back<NrRecordKeep>, lds);
  k_newrale_back<<<nw < NR_GRID ? nw : NR_GRID, 256, lds, s>>>(NrRecordKeep{out, T, w0, L, hop}, nw, iy, stats, prm);
  return 0;
}

// Live 12-lead streams (NewRALELiveDenoiser): the record kernels' bodies on k_live_windows' / k_live_emit's geometry.  L as for
// the record kernels (a multiple of 16 in [16, 1024]).
int launch_newrale_live_front(const float* hist, const float* x, float* hist_out, long long S, int L, int hop, int C,
                              long long base, long long k0, int nw, long long T, long long w0, int nb, const float* prm,
                              float* inner, float* stats, hipStream_t s) {
  if (!live_geom_ok(S, NR_LEADS, L, hop, k0, nw, T, w0, nb, 16, 1024) || C < 0 || (nb == 0 && !hist_out) || hist_out == hist)
    return -1;
  if (!live_windows_in_v(L, hop, C, base, k0, nw, T)) return -1;
  const long long rows = S * NR_LEADS;
  const int nwg = nb < NR_GRID ? nb : NR_GRID;
  const int nhg = hist_out ? (int)(rows < NR_GRID ? rows : NR_GRID) : 0;    // history workgroups, rows in turn
  const size_t lds = newrale_front_lds(L);
  RAL_SET_LDS(k_newrale_front<NrLiveWindows>, lds);
  k_newrale_front<<<nwg + nhg, 256, lds, s>>>(NrLiveWindows{hist, x, hist_out, S, base, T, w0, L, hop, C, (int)k0, nw}, nb, nwg,
                                              prm, inner, stats);
  return 0;
}

int launch_newrale_live_back(const float* iy, const float* stats, const float* prm, long long S, int L, int hop, long long k0,
                             int nw, long long T, long long w0, int nb, long long lo, int m, float* out, float* last_y,
                             float* last_stats, hipStream_t s) {
  if (!live_geom_ok(S, NR_LEADS, L, hop, k0, nw, T, w0, nb, 16, 1024) || nb < 1 || lo < 0 || m < 0 || (!last_y != !last_stats))
    return -1;
  const size_t lds = newrale_back_lds(L);
  RAL_SET_LDS(k_newrale_back<NrLiveKeep>, lds);
  k_newrale_back<<<nb < NR_GRID ? nb : NR_GRID, 256, lds, s>>>(NrLiveKeep{out, last_y, last_stats, T, w0, lo, L, hop, (int)k0, nw, m},
                                                               nb, iy, stats, prm);
  return 0;
}

// =================================================================================
// Stream pool (LivePool / NewRALELivePool, infer.py): the live kernels with every per-call scalar replaced by a row of a table,
// ral_pool_row (include/ralenet.h), one row per stream the call names.  The slots, their two history planes of L samples and
// the rows' shared fields follow the slot protocol (ral_slots.hpp); the history workgroups of the call's first gather launch
// write the next history.  V of a row is its history ++ its chunk, samples [n0 - L, n0 + c) of the stream.  Window gw of the
// call is window k0 + (gw - w_off) of the row found by pool_find_row (the rows' w_off are the prefix sums of their nw).  The
// window arithmetic is that of the live kernels: zscore_wave, stream_keep / stream_keep_open, stream_start, stream_kept.
// =================================================================================
typedef ral_pool_row PoolRow;

// the row that holds window gw of the call: the last one with w_off <= gw (rows without windows share the w_off of the next
// row with some, or the total behind the last one, so they are never the answer for gw below the total)
RAL_DEV int pool_find_row(const PoolRow* __restrict__ tab, int rows, long long gw) {
  int a = 0, b = rows - 1;
  while (a < b) {
    const int mid = (a + b + 1) >> 1;
    if (tab[mid].w_off <= gw) a = mid; else b = mid - 1;
  }
  return a;
}

// What a workgroup derives from its row is the same in every lane.  Passing it through readfirstlane keeps it in scalar
// registers: observed with -Rpass-analysis=kernel-resource-usage for gfx950, k_newrale_back<NrPoolKeep> needs 135 VGPRs
// without these calls and 110 with them.
RAL_DEV int pool_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
RAL_DEV long long pool_uniform(long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(unsigned long long)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)((unsigned long long)v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}

RAL_DEV StreamKeep pool_keep(const PoolRow& t, int L, int hop) { return t.T < 0 ? stream_keep_open(L, hop) : stream_keep(t.T, L, hop); }

// the samples [b, e) of the stream that window k of row t (starting at `start`) gives to this call: what the window keeps
// (stream_kept), inside [lo, lo + m) and inside the window, as k_live_emit clips them
RAL_DEV void pool_kept(const StreamKeep& sk, const PoolRow& t, int k, long long start, int L, int hop, long long& b, long long& e) {
  stream_kept(sk, k, t.T, hop, b, e);
  b = b > t.lo ? b : t.lo;
  b = b > start ? b : start;
  e = e < t.lo + t.m ? e : t.lo + t.m;
  e = e < start + L ? e : start + L;
}

// the next history of (row, lead): V[c, c + L), the last L samples the stream has received after this call
RAL_DEV void pool_write_history(const PoolRow& t, int c, int leads, int L, long long cap, float* hist,
                                const float* __restrict__ x) {
  slot_write_history(hist + slot_plane(t.turn, t.slot, cap, leads, L, c), x + t.x_off * leads + (long long)c * t.c,
                     hist + slot_plane(1 - t.turn, t.slot, cap, leads, L, c), t.n0, t.c, L);
}

__global__ __launch_bounds__(64) void k_pool_windows(float* hist, const float* __restrict__ x, const PoolRow* __restrict__ tab,
                                                     int rows, long long cap, int leads, int L, int hop, long long w0, int nb,
                                                     float* __restrict__ win, float* __restrict__ stats) {
  const int nwl = nb * leads;
  if ((int)blockIdx.x >= nwl) {   // the history of one (row, lead)
    const int rc = blockIdx.x - nwl, r = rc / leads;
    const PoolRow t = tab[r];
    if (t.flags & RAL_POOL_KEEP) pool_write_history(t, rc - r * leads, leads, L, cap, hist, x);
    return;
  }
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;   // window of this launch, lead
  const long long gw = w0 + i;
  const PoolRow t = tab[pool_find_row(tab, rows, gw)];
  const StreamKeep sk = pool_keep(t, L, hop);
  const int j = (int)(gw - t.w_off);
  const int o = (int)(stream_start(sk, (int)t.k0 + j, t.T, L, hop) - (t.n0 - L));   // the window is V[o, o + L)
  const float* hr = hist + slot_plane(t.turn, t.slot, cap, leads, L, c);
  const float* xr = x + t.x_off * leads + (long long)c * t.c - L;
  float mean, sd;
  zscore_wave([=](int l) { const int v = o + l; return v < L ? hr[v] : xr[v]; }, win + ((size_t)i * leads + c) * L, L, mean, sd);
  if (threadIdx.x == 0) { stats[(gw * leads + c) * 2] = mean; stats[(gw * leads + c) * 2 + 1] = sd; }
}

// y (nb, leads, L) and stats: the model output and (mean, std) of windows [w0, w0 + nb) of the call.  from_last: window gw is
// the one window of row gw, and y / stats are the kept windows of the slots, (capacity, leads, L) and (capacity, leads, 2).
__global__ __launch_bounds__(64) void k_pool_emit(const float* __restrict__ y, const float* __restrict__ stats,
                                                  const PoolRow* __restrict__ tab, int rows, int leads, int L, int hop,
                                                  long long w0, int from_last, float* __restrict__ out,
                                                  float* __restrict__ last_y, float* __restrict__ last_stats) {
  const int i = blockIdx.x / leads, c = blockIdx.x - i * leads;
  const long long gw = w0 + i;
  const PoolRow t = tab[from_last ? (int)gw : pool_find_row(tab, rows, gw)];
  const StreamKeep sk = pool_keep(t, L, hop);
  const int j = from_last ? 0 : (int)(gw - t.w_off), k = (int)t.k0 + j;
  const long long start = stream_start(sk, k, t.T, L, hop);
  long long b, e;
  pool_kept(sk, t, k, start, L, hop, b, e);
  const long long sw = from_last ? (long long)t.slot : gw;            // the window's place in stats
  const float mean = stats[(sw * leads + c) * 2], sd = stats[(sw * leads + c) * 2 + 1];
  const float* yr = y + ((size_t)(from_last ? t.slot : i) * leads + c) * L;
  float* dst = out + t.out_off * leads + (long long)c * t.m - t.lo;
  for (long long p = b + threadIdx.x; p < e; p += 64) dst[p] = fmaf(yr[p - start], sd, mean);
  if (last_y && (t.flags & RAL_POOL_KEEP) && j == t.nw - 1) {
    float* ly = last_y + ((size_t)t.slot * leads + c) * L;
    for (int l = threadIdx.x; l < L; l += 64) ly[l] = yr[l];
    if (threadIdx.x == 0) { last_stats[((size_t)t.slot * leads + c) * 2] = mean; last_stats[((size_t)t.slot * leads + c) * 2 + 1] = sd; }
  }
}

// The table is checked here, on the host, before anything reaches the device (slots_walk, ral_slots.hpp, with the window pools'
// own rules).  -> null if the table is sound, else the rule that is broken, with *bad the row that breaks it (-1: the geometry).
// x_total / out_total: samples per lead in the packed chunk / output buffer (ignored when negative: the emit / gather does not
// touch that buffer).  from_last: the table of an emit of kept windows (one window per row, the last regular one before n0).
// walk = false (a launch that reuses the device copy of a table checked at its upload): the geometry only.
static const char* pool_table_fault(const PoolRow* tab, int rows, long long cap, int leads, int L, int hop, int lmul, int lmax,
                                    long long x_total, long long out_total, bool from_last, bool walk, int* bad) {
  *bad = -1;
  if (rows < 1) return "rows >= 1";
  if (cap < 1) return "capacity >= 1";
  if (leads < 1) return "leads >= 1";
  if (L < lmul || L % lmul != 0 || L > lmax) return lmul == 64 ? "L a multiple of 64 and <= 2048" : "L a multiple of 16 in [16, 1024]";
  if (hop < 1 || hop > L || ((L - hop) & 1)) return "1 <= hop <= L with L - hop even";
  if (!walk) return nullptr;
  const SlotRules rules{L, true, "n0, c, nw, m, k0, lo >= 0 and c < 2^30",
                        "T = n0 + c >= L without RAL_POOL_KEEP, or T = -1 with RAL_POOL_KEEP and c >= 1"};
  long long w_sum = 0;
  auto in_range = [](const PoolRow& t) {
    return !(t.n0 < 0 || t.c < 0 || t.c > 0x3fffffff || t.nw < 0 || t.m < 0 || t.k0 < 0 || t.lo < 0);
  };
  auto early = [&](const PoolRow& t) -> const char* {
    if (t.w_off != w_sum) return "w_off the prefix sum of nw";
    w_sum += t.nw;
    return nullptr;
  };
  auto own = [&](const PoolRow& t) -> const char* {
    if (out_total >= 0 && (t.out_off < 0 || t.out_off + t.m > out_total)) return "the emitted samples inside the packed output";
    if (t.lo + t.m > t.n0 + t.c) return "lo + m <= n0 + c (nothing emitted that was not received)";
    if (from_last) {   // the last regular window complete at n0: it ends at or before n0, the next one would not
      long long st;
      if (t.T < 0 || t.nw != 1 || t.n0 < L || !live_window_start(t.T, L, hop, t.k0, st) || t.k0 * hop + L > t.n0 ||
          (t.k0 + 1) * hop + L <= t.n0)
        return "from_last rows with T known, nw = 1, n0 >= L and k0 the last regular window complete at n0";
    } else if (t.nw > 0) {
      long long first, last;
      if (!live_window_start(t.T, L, hop, t.k0, first) || !live_window_start(t.T, L, hop, t.k0 + t.nw - 1, last))
        return "windows k0 .. k0 + nw - 1 in the stream";
      if (first < t.n0 - L || first < 0) return "the first window at or after the history, max(n0 - L, 0)";
      if (last + L > t.n0 + t.c) return "the last window inside the received samples, n0 + c";
      if (t.lo < first || t.lo + t.m > last + L) return "[lo, lo + m) inside the windows";
    }
    return nullptr;
  };
  if (const char* why = slots_walk(tab, rows, cap, x_total, rules, in_range, early, own, bad)) return why;
  return w_sum <= 0x7fffffffLL ? nullptr : "at most 2^31 - 1 windows";
}

static long long pool_windows_total(const PoolRow* tab, int rows) { return tab[rows - 1].w_off + tab[rows - 1].nw; }

// the checks of a gather / an emit launch: the table (walked when it is uploaded), then the launch's own arguments
static const char* pool_gather_fault(const PoolRow* tab, int rows, long long cap, int leads, int L, int hop, int lmul, int lmax,
                                     long long x_total, int upload, int write_hist, long long w0, int nb, int* bad) {
  *bad = -1;
  if (x_total < 0) return "x_total >= 0";
  if (const char* why = pool_table_fault(tab, rows, cap, leads, L, hop, lmul, lmax, x_total, -1, false, upload != 0, bad)) return why;
  if (w0 < 0 || nb < 0 || w0 + nb > pool_windows_total(tab, rows)) return "a window range inside the call's windows";
  if (nb == 0 && !write_hist) return "nb >= 1 or write_hist";
  if ((long long)nb * leads + (write_hist ? (long long)rows * leads : 0) > 0x7fffffffLL) return "at most 2^31 - 1 workgroups";
  return nullptr;
}

static const char* pool_emit_fault(const PoolRow* tab, int rows, long long cap, int leads, int L, int hop, int lmul, int lmax,
                                   long long out_total, int upload, long long w0, int nb, int from_last, const float* last_y,
                                   const float* last_stats, int* bad) {
  *bad = -1;
  if (out_total < 0) return "out_total >= 0";
  if (const char* why = pool_table_fault(tab, rows, cap, leads, L, hop, lmul, lmax, -1, out_total, from_last != 0, upload != 0, bad))
    return why;
  if (w0 < 0 || nb < 1 || w0 + nb > pool_windows_total(tab, rows)) return "a window range of nb >= 1 windows inside the call's";
  if (!last_y != !last_stats) return "last_y and last_stats both given or both null";
  if (from_last && last_y) return "last_y and last_stats null with from_last";
  if ((long long)nb * leads > 0x7fffffffLL) return "at most 2^31 - 1 workgroups";
  return nullptr;
}

int launch_pool_windows(float* hist, const float* x, long long x_total, const ral_pool_row* tab, int rows, ral_pool_row* tab_dev,
                        int upload, long long cap, int leads, int L, int hop, int write_hist, long long w0, int nb, float* win,
                        float* stats, hipStream_t s, const char** why, int* bad) {
  if ((*why = pool_gather_fault(tab, rows, cap, leads, L, hop, 64, 2048, x_total, upload, write_hist, w0, nb, bad))) return -1;
  const long long grid = (long long)nb * leads + (write_hist ? (long long)rows * leads : 0);
  if (upload && slots_upload(tab, rows, tab_dev, s)) return -2;
  k_pool_windows<<<(int)grid, 64, 0, s>>>(hist, x, tab_dev, rows, cap, leads, L, hop, w0, nb, win, stats);
  return 0;
}

int launch_pool_emit(const float* y, const float* stats, const ral_pool_row* tab, int rows, ral_pool_row* tab_dev, int upload,
                     long long cap, int leads, int L, int hop, long long w0, int nb, int from_last, float* out,
                     long long out_total, float* last_y, float* last_stats, hipStream_t s, const char** why, int* bad) {
  if ((*why = pool_emit_fault(tab, rows, cap, leads, L, hop, 64, 2048, out_total, upload, w0, nb, from_last, last_y, last_stats, bad)))
    return -1;
  if (upload && slots_upload(tab, rows, tab_dev, s)) return -2;
  k_pool_emit<<<nb * leads, 64, 0, s>>>(y, stats, tab_dev, rows, leads, L, hop, w0, from_last, out, last_y, last_stats);
  return 0;
}

// 12-lead pool streams (NewRALELivePool): the bodies of k_newrale_front / k_newrale_back on the pool's table.  The stream
// geometry differs from row to row, so keep() is a placeholder and window() works out the row's own.
struct NrPoolWindows {
  float* hist;             // (2, capacity, 12, L)
  const float* x;          // the packed chunks
  const PoolRow* tab;
  long long cap, w0;
  int rows, L, hop;
  typedef NrLiveWindows::Reader Reader;
  RAL_DEV StreamKeep keep() const { return stream_keep_open(L, hop); }
  RAL_DEV long long window(const StreamKeep&, int i, Reader& src) const {
    const long long gw = w0 + i;
    const PoolRow t = tab[pool_find_row(tab, rows, gw)];
    const StreamKeep sk = pool_keep(t, L, hop);
    const int j = (int)(gw - t.w_off);
    src.o = pool_uniform((int)(stream_start(sk, (int)t.k0 + j, t.T, L, hop) - (t.n0 - L)));
    src.hr = hist + pool_uniform((long long)slot_plane(t.turn, t.slot, cap, NR_LEADS, L));
    src.xr = x + pool_uniform((long long)(t.x_off * NR_LEADS - L));
    src.L = L;
    src.C = pool_uniform(t.c);
    return gw;
  }
  // workgroup g of ng writes the next history of the (row, lead) pairs g, g + ng, ... of the rows that stay open
  RAL_DEV void write_history(int g, int ng) const {
    for (int rc = g; rc < rows * NR_LEADS; rc += ng) {
      const int r = rc / NR_LEADS;
      const PoolRow t = tab[r];
      if (t.flags & RAL_POOL_KEEP) pool_write_history(t, rc - r * NR_LEADS, NR_LEADS, L, cap, hist, x);
    }
  }
};

struct NrPoolKeep {        // into the packed output of a pool call: row t's samples [lo, lo + m) as (12, m) at out_off * 12
  float* out;
  float* last_y;           // (capacity, 2, L) or null
  float* last_stats;       // (capacity, 12, 2) or null (with last_y)
  const PoolRow* tab;
  long long w0;
  int rows, L, hop, from_last;
  RAL_DEV StreamKeep keep() const { return stream_keep_open(L, hop); }
  RAL_DEV NrKept window(const StreamKeep&, int i) const {
    NrKept kp;
    const long long g = w0 + i;
    const PoolRow t = tab[from_last ? (int)g : pool_find_row(tab, rows, g)];
    const StreamKeep sk = pool_keep(t, L, hop);
    const int j = from_last ? 0 : (int)(g - t.w_off), k = (int)t.k0 + j;
    const long long start = stream_start(sk, k, t.T, L, hop);
    long long b, e;
    pool_kept(sk, t, k, start, L, hop, b, e);
    kp.gw = pool_uniform(from_last ? (long long)t.slot : g);    // (from_last: stats are the slots' kept ones)
    kp.ob = pool_uniform((int)(b - start));
    kp.oe = e > b ? pool_uniform((int)(e - start)) : kp.ob;
    kp.dst = pool_uniform((long long)(t.out_off * NR_LEADS + start - t.lo));
    kp.stride = pool_uniform(t.m);
    kp.src = pool_uniform((from_last ? (long long)t.slot : (long long)i) * 2 * L);
    const long long keep_at = last_y && (t.flags & RAL_POOL_KEEP) && j == t.nw - 1 ? (long long)t.slot * 2 * L : -1;
    kp.ly = pool_uniform(keep_at) >= 0 ? last_y + pool_uniform(keep_at) : nullptr;
    return kp;
  }
  RAL_DEV void keep_stats(const NrKept& kp, const float* stats) const {
    if (kp.ly && threadIdx.x < 2 * NR_LEADS)
      last_stats[((kp.ly - last_y) / (2 * L)) * 2 * NR_LEADS + threadIdx.x] = stats[kp.gw * 2 * NR_LEADS + threadIdx.x];
  }
};

int launch_newrale_pool_front(float* hist, const float* x, long long x_total, const ral_pool_row* tab, int rows,
                              ral_pool_row* tab_dev, int upload, long long cap, int L, int hop, int write_hist, long long w0,
                              int nb, const float* prm, float* inner, float* stats, hipStream_t s, const char** why, int* bad) {
  if ((*why = pool_gather_fault(tab, rows, cap, NR_LEADS, L, hop, 16, 1024, x_total, upload, write_hist, w0, nb, bad))) return -1;
  if (upload && slots_upload(tab, rows, tab_dev, s)) return -2;
  const long long hrows = (long long)rows * NR_LEADS;
  const int nwg = nb < NR_GRID ? nb : NR_GRID;
  const int nhg = write_hist ? (int)(hrows < NR_GRID ? hrows : NR_GRID) : 0;
  const size_t lds = newrale_front_lds(L);
  RAL_SET_LDS(k_newrale_front<NrPoolWindows>, lds);
  k_newrale_front<<<nwg + nhg, 256, lds, s>>>(NrPoolWindows{hist, x, tab_dev, cap, w0, rows, L, hop}, nb, nwg, prm, inner, stats);
  return 0;
}

int launch_newrale_pool_back(const float* iy, const float* stats, const float* prm, const ral_pool_row* tab, int rows,
                             ral_pool_row* tab_dev, int upload, long long cap, int L, int hop, long long w0, int nb, int from_last,
                             float* out, long long out_total, float* last_y, float* last_stats, hipStream_t s, const char** why,
                             int* bad) {
  if ((*why = pool_emit_fault(tab, rows, cap, NR_LEADS, L, hop, 16, 1024, out_total, upload, w0, nb, from_last, last_y, last_stats,
                              bad)))
    return -1;
  if (upload && slots_upload(tab, rows, tab_dev, s)) return -2;
  const size_t lds = newrale_back_lds(L);
  RAL_SET_LDS(k_newrale_back<NrPoolKeep>, lds);
  k_newrale_back<<<nb < NR_GRID ? nb : NR_GRID, 256, lds, s>>>(NrPoolKeep{out, last_y, last_stats, tab_dev, w0, rows, L, hop, from_last},
                                                               nb, iy, stats, prm);
  return 0;
}
