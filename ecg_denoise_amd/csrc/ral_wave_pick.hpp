// What one wave of 64 picks from the values its lanes hold, for the kernels that give a beat to a wave (ral_delineate.hip,
// ral_pst.hip): the largest value, the largest and the smallest index, and the largest value with the smallest index that has
// it - butterflies over __shfl_xor, after which every lane holds the result - and the clamp of an index into a record.
#pragma once
#include "ral_device.hpp"

constexpr int DL_WAVE = 64;

RAL_DEV float delin_max(float v) {
#pragma unroll
  for (int o = DL_WAVE / 2; o; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, DL_WAVE));
  return v;
}

RAL_DEV long long delin_shfl(long long v, int o) {
  const int lo = __shfl_xor((int)(v & 0xffffffffLL), o, DL_WAVE), hi = __shfl_xor((int)(v >> 32), o, DL_WAVE);
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

RAL_DEV long long delin_imax(long long v) {
#pragma unroll
  for (int o = DL_WAVE / 2; o; o >>= 1) {
    const long long w = delin_shfl(v, o);
    v = w > v ? w : v;
  }
  return v;
}

RAL_DEV long long delin_imin(long long v) {
#pragma unroll
  for (int o = DL_WAVE / 2; o; o >>= 1) {
    const long long w = delin_shfl(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// the largest value and the smallest index that has it, the same in every lane
RAL_DEV void delin_argmax(float& v, long long& at) {
#pragma unroll
  for (int o = DL_WAVE / 2; o; o >>= 1) {
    const float w = __shfl_xor(v, o, DL_WAVE);
    const long long wa = delin_shfl(at, o);
    if (w > v || (w == v && wa < at)) v = w, at = wa;
  }
}

RAL_DEV long long delin_clamp(long long t, long long top) { return t < 0 ? 0 : (t > top ? top : t); }
