// What the split-KV decode kernels share (decode_attn.hip, bf16 caches;
// decode_attn_q8.hip, int8 caches): vector types, the tile constants, the
// layout of the wave-private V image in LDS, and small device helpers.
// Include it inside the file's target-attribute region: the helpers use
// compiler builtins only, because a header function compiled with other
// target features than its caller is not inlined.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int DS_THREADS = 256;
constexpr int DS_WAVES = 4;
constexpr int DS_TILE = 64;    // keys per wave step
constexpr int DS_HEADS = 16;   // query heads per block (MFMA N)
// "not visible" score and empty running max: finite (-ffast-math)
constexpr float DS_NEG = -1e30f;

// V image: row stride 256 B for D = 128 / 96, 128 B for D = 64.
constexpr int ds_rowb(int d) { return d == 64 ? 128 : 256; }

// Byte offset of 16-byte chunk `ch` of row `row`.  A transposed read takes,
// per 32-lane half, 32 bytes (chunk pair ch>>1) of 8 consecutive rows: the
// XOR sends those 8 rows to 8 different 32-byte slots of the 256 bytes the
// 64 read banks span.  A 16-byte staging store of 8 lanes covers 8 chunks of
// one row, which stay 8 different chunks mod 8 (32 store banks).
template <int RB>
__device__ __forceinline__ int ds_voff(int row, int ch) {
  if (RB == 256) return 256 * row + 16 * (ch ^ ((row & 7) << 1));
  return 128 * row + 16 * (ch ^ (((row >> 1) & 3) << 1));
}

__device__ __forceinline__ short ds_bf16bits(float f) {
  return __builtin_bit_cast(short, (__bf16)f);  // v_cvt_pk_bf16_f32, RNE
}

__device__ __forceinline__ float ds_exp(float x) {
  return __builtin_amdgcn_exp2f(x * 1.4426950408889634f);
}

__device__ __forceinline__ float ds_shfl_xor(float v, int mask) {
  const int src = ((int)__builtin_amdgcn_mbcnt_hi(
                       ~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) ^ mask) << 2;
  return __builtin_bit_cast(
      float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, v)));
}

__device__ __forceinline__ void ds_block_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ bf16x8 ds_zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = 0;
  return z;
}

__device__ __forceinline__ float ds_bf16_f32(short v) {
  return __builtin_bit_cast(float, ((unsigned int)(unsigned short)v) << 16);
}

// lgkmcnt(0) only: the wave-private V image must not drain the prefetch.
__device__ __forceinline__ void ds_wait_lds() {
  __builtin_amdgcn_s_waitcnt(0xC07F);
}

}  // namespace
