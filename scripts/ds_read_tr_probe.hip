// Verify the lane <-> element map of ds_read_b64_tr_b16 on gfx950 HW, and
// the address formulas the flash v3 kernels use to feed the B operand of
// mfma_f32_32x32x16_bf16 from a ROW-major LDS image.
//
// Assumed (per 16-lane group, lanes 16g .. 16g+15, i = lane & 15):
//   lane i supplies the address of row (i >> 2), columns 4*(i & 3) .. +3 of
//   a 4-row x 16-column block of 16-bit elements;
//   lane i receives column i of the block, row q in element q.
//
// Test 1: plain [32][128] image, group g reads rows 4g .. 4g+3, cols 0..15.
// Test 2: the swizzled dual-use images of flash_attn.hip (v3_off<SWB>, 256-
//   and 128-byte rows) read with v3_tr_addr: lane (ln = l & 31, hi = l >> 5)
//   must get T[16*c2 + 8*hi + 4*e + q][32*t + ln] in element q of read e,
//   i.e. the natural-k B fragment of the 32x32x16 MFMA.
//
// Build+run (GPU box):
//   hipcc --offload-arch=gfx950 -O2 scripts/ds_read_tr_probe.hip \
//       -o scripts/ds_read_tr_probe && scripts/ds_read_tr_probe
#include <hip/hip_runtime.h>
#include <cstdio>

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

__device__ __forceinline__ s16x4 tr_read(const char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)p);
}

// keep in step with flash_attn.hip
template <int SWB>
__device__ __forceinline__ int v3_off(int row, int ch) {
  if (SWB == 256)
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  return 128 * row + 16 * (ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)));
}
template <int SWB>
__device__ __forceinline__ int v3_tr_addr(int lane, int row0, int col0) {
  const int i = lane & 15;
  const int row = row0 + (i >> 2);
  const int col = col0 + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
  return v3_off<SWB>(row, col >> 3) + 2 * (col & 7);
}

__global__ void plain_kernel(short* out) {
  __shared__ __attribute__((aligned(16))) char img[32 * 256];
  const int l = threadIdx.x;
  for (int e = l; e < 32 * 128; e += 64)
    reinterpret_cast<short*>(img)[e] = (short)e;  // T[r][c] = 128 r + c
  __syncthreads();
  const int g = l >> 4, i = l & 15;
  s16x4 v = tr_read(img + (4 * g + (i >> 2)) * 256 + 8 * (i & 3));
  for (int q = 0; q < 4; ++q) out[l * 4 + q] = v[q];
}

template <int SWB>
__global__ void frag_kernel(short* out) {
  constexpr int COLS = SWB / 2;
  __shared__ __attribute__((aligned(16))) char img[32 * SWB];
  const int l = threadIdx.x;
  for (int e = l; e < 32 * COLS; e += 64) {
    const int r = e / COLS, c = e % COLS;
    *reinterpret_cast<short*>(img + v3_off<SWB>(r, c >> 3) + 2 * (c & 7)) =
        (short)(128 * r + c);
  }
  __syncthreads();
  const int hi = l >> 5;
  int n = 0;
  for (int c2 = 0; c2 < 2; ++c2)
    for (int t = 0; t < COLS / 32; ++t)
      for (int e = 0; e < 2; ++e) {
        s16x4 v = tr_read(
            img + v3_tr_addr<SWB>(l, 16 * c2 + 8 * hi + 4 * e, 32 * t));
        for (int q = 0; q < 4; ++q) out[(n * 64 + l) * 4 + q] = v[q];
        ++n;
      }
}

template <int SWB>
static int check_frag(short* out) {
  constexpr int COLS = SWB / 2;
  hipLaunchKernelGGL(frag_kernel<SWB>, dim3(1), dim3(64), 0, 0, out);
  if (hipDeviceSynchronize() != hipSuccess) return 1;
  int bad = 0, n = 0;
  for (int c2 = 0; c2 < 2; ++c2)
    for (int t = 0; t < COLS / 32; ++t)
      for (int e = 0; e < 2; ++e, ++n)
        for (int l = 0; l < 64; ++l)
          for (int q = 0; q < 4; ++q) {
            const int want =
                128 * (16 * c2 + 8 * (l >> 5) + 4 * e + q) + 32 * t + (l & 31);
            const int got = out[(n * 64 + l) * 4 + q];
            if (got != want && bad++ < 5)
              printf("SWB=%d c2=%d t=%d e=%d lane=%d q=%d got %d want %d\n",
                     SWB, c2, t, e, l, q, got, want);
          }
  printf("DS_READ_TR B-FRAGMENT SWB=%d: %s\n", SWB, bad ? "FAIL" : "OK");
  return bad != 0;
}

int main() {
  short* out;
  if (hipMallocManaged(&out, 64 * 64 * 4 * sizeof(short)) != hipSuccess)
    return 2;
  hipLaunchKernelGGL(plain_kernel, dim3(1), dim3(64), 0, 0, out);
  if (hipDeviceSynchronize() != hipSuccess) return 2;
  int bad = 0;
  for (int l = 0; l < 64; ++l)
    for (int q = 0; q < 4; ++q) {
      const int want = 128 * (4 * (l >> 4) + q) + (l & 15);
      if (out[l * 4 + q] != want && bad++ < 5)
        printf("plain lane=%d q=%d got %d want %d\n", l, q, out[l * 4 + q],
               want);
    }
  printf("DS_READ_TR LANE MAP: %s\n", bad ? "FAIL" : "OK");
  int rc = bad != 0;
  rc |= check_frag<256>(out);
  rc |= check_frag<128>(out);
  return rc;
}
