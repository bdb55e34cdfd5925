// Lane-map check of v_mfma_f32_32x32x16_f16 (gfx950) with exact integer data: lane l (r = l & 31, h = l >> 5) holds
// A[row r][k = 8h + j] and B[k = 8h + j][col r], j = 0..7; D[row][col] sits in lane col + 32 * ((row >> 2) & 1),
// register (row & 3) + 4 * (row >> 3).  Prints the number of mismatches (0 expected).
//   hipcc --offload-arch=gfx950 -O3 -o mfma32_map_probe tools/diag/mfma32_map_probe.hip && ./mfma32_map_probe
#include <hip/hip_runtime.h>
#include <stdio.h>

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ void k_map(const float* A, const float* B, float* D) {   // A 32x16, B 16x32, D 32x32, row-major
  const int l = threadIdx.x, r = l & 31, h = l >> 5;
  h8 a, b;
  for (int j = 0; j < 8; ++j) { a[j] = (_Float16)A[r * 16 + 8 * h + j]; b[j] = (_Float16)B[(8 * h + j) * 32 + r]; }
  f32x16 c;
  for (int i = 0; i < 16; ++i) c[i] = 0.f;
  c = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  for (int i = 0; i < 16; ++i) D[((i & 3) + 8 * (i >> 2) + 4 * h) * 32 + r] = c[i];
}

int main() {
  float hA[512], hB[512], hD[1024], *A, *B, *D;
  for (int i = 0; i < 512; ++i) { hA[i] = (float)((i * 7 + 3) % 13 - 6); hB[i] = (float)((i * 5 + 1) % 11 - 5); }
  if (hipMalloc(&A, sizeof hA) != hipSuccess || hipMalloc(&B, sizeof hB) != hipSuccess || hipMalloc(&D, sizeof hD) != hipSuccess) return 2;
  (void)hipMemcpy(A, hA, sizeof hA, hipMemcpyHostToDevice); (void)hipMemcpy(B, hB, sizeof hB, hipMemcpyHostToDevice);
  k_map<<<1, 64>>>(A, B, D);
  if (hipMemcpy(hD, D, sizeof hD, hipMemcpyDeviceToHost) != hipSuccess) return 2;
  int bad = 0;
  for (int i = 0; i < 32; ++i)
    for (int j = 0; j < 32; ++j) {
      float s = 0.f;
      for (int k = 0; k < 16; ++k) s += hA[i * 16 + k] * hB[k * 32 + j];
      bad += s != hD[i * 32 + j];
    }
  printf("v_mfma_f32_32x32x16_f16 lane map: %d mismatches of 1024\n", bad);
  return bad != 0;
}
