// Weight-streaming GEMM for 1..16-row decode on MI355X (gfx950).
//
//   Yt[out, rows] = W[out, K] . Xt[K, rows]      fp32 accumulate, bf16 out
//   w      [out, K]   bf16, or int8 with scale [out] fp32 (W8A16: the int8
//                     values become bf16 exactly, the accumulator is scaled
//                     once at the end; x is never quantised)
//   x      [rows, K]  bf16, 1 <= rows <= 16, K % 64 == 0
//   y      [rows, out] bf16
// A decode step reads every weight once whatever the batch, so the kernel is
// a weight stream whose M dimension is the weight rows: one
// mfma_f32_16x16x32_bf16 takes 16 weight rows x 32 k as A and 32 k x 16 batch
// columns as B, and the reuse of x across the batch comes from the
// instruction.
//
// Grid = ceil(out / 16) blocks x 256 threads, one launch, no workspace, no
// atomics.  A block owns 16 output features; its four waves take the k-steps
// round-robin, each with its own accumulator, and are merged once at the end
// through LDS in wave order; wave 0 stores.  The split depends on (K, out,
// weight dtype) only, never on rows, and a column of the MFMA result depends
// on that column of B alone, so row i of the result has the same bits
// whatever else is in the batch.
//
// Operands go global memory -> registers -> MFMA, no LDS.  Per k-step lane
// (r = l % 16, g = l / 16) loads the 64 contiguous bytes of weight row
// row0 + r that start at byte 256 * step + 64 * g, as four 16-byte loads: a
// wave reads 256 contiguous bytes of each of its 16 rows per step.
//   bf16: 64 bytes = 32 k, a k-step is 128 k.  MFMA j takes the lane's j-th
//         16 bytes, so its k slot (g, e) is k0 + 32 g + 8 j + e.
//   int8: 64 bytes = 64 k, a k-step is 256 k.  The j-th 16 bytes give two A
//         fragments (low and high 8 values), k0 + 64 g + 16 j + 8 h + e.
// A dot product does not care about the order of k: the B fragment is read
// from x with the same bijection, i.e. lane (n = l % 16, g) loads the 64
// (bf16) or 128 (int8) contiguous bytes of x row n at the same k.  x is at
// most 16 x K x 2 bytes and stays in L2.
//
// Nothing outside w and x is read.  Lanes with n >= rows read x row 0 again
// (the same addresses as lane n = 0): their columns of the result are copies
// of column 0 and are never stored.  Weight rows past `out` in the last tile
// are clamped to out - 1 and not stored either.  K % 64 == 0 makes a lane's
// piece lie entirely inside or outside [0, K): the one partial k-step at the
// end of K is loaded under that predicate, with zeros outside.
//
// Latency: each wave keeps DG_PF whole k-steps of A and B in flight ahead of
// its MFMAs, in a ring of DG_PF + 1 register stages indexed at compile time.
// The loads of the steady loop are unconditional straight-line code, which
// is what lets the compiler wait for the oldest stage only (vmcnt counts
// loads in order; a load under a branch forces a wait for everything).

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) int i32x4;
typedef __attribute__((ext_vector_type(16))) signed char i8x16;

constexpr int DG_THREADS = 256;
constexpr int DG_WAVES = 4;
constexpr int DG_TILE = 16;         // output features per block (MFMA M)
constexpr int DG_STEP_BYTES = 256;  // weight bytes per row and k-step
constexpr int DG_PF = 2;            // k-steps in flight ahead of the MFMAs
constexpr int DG_NS = DG_PF + 1;    // register stages

template <bool W8>
struct DgStage {
  static constexpr int KS = W8 ? 256 : 128;  // k per step
  static constexpr int NB = W8 ? 8 : 4;      // 16-byte pieces of x per lane
  i32x4 a[4];    // the lane's 64 weight bytes
  bf16x8 b[NB];  // x at the same k, 8 values per piece
};

__device__ __forceinline__ short dg_bf16bits(float f) {
  return __builtin_bit_cast(short, (__bf16)f);
}

// 8 int8 values -> bf16, exact (|q| <= 128 has at most 8 significant bits)
template <int H>
__device__ __forceinline__ bf16x8 dg_cvt8(i32x4 v) {
  const i8x16 q = __builtin_bit_cast(i8x16, v);
  bf16x8 out;
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = dg_bf16bits((float)q[8 * H + e]);
  return out;
}

// wp / xp point at the lane's piece of step 0; the step lies inside [0, K)
template <bool W8>
__device__ __forceinline__ void dg_load(DgStage<W8>& s, const char* wp,
                                        const bf16_t* xp, long step) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    s.a[j] = *reinterpret_cast<const i32x4*>(wp + step * DG_STEP_BYTES +
                                             16 * j);
#pragma unroll
  for (int p = 0; p < DgStage<W8>::NB; ++p)
    s.b[p] = *reinterpret_cast<const bf16x8*>(xp + step * DgStage<W8>::KS +
                                              8 * p);
}

template <bool W8>
__device__ __forceinline__ void dg_mma(const DgStage<W8>& s, f32x4 (&acc)[2]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if constexpr (W8) {
      acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          dg_cvt8<0>(s.a[j]), s.b[2 * j], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          dg_cvt8<1>(s.a[j]), s.b[2 * j + 1], acc[1], 0, 0, 0);
    } else {
      acc[j & 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
          __builtin_bit_cast(bf16x8, s.a[j]), s.b[j], acc[j & 1], 0, 0, 0);
    }
  }
}

// Register budget: three stages are 96 VGPRs for bf16 (4 waves/SIMD) and 144
// for int8, whose x pieces are twice as long (2 waves/SIMD; asking for 3
// makes the compiler spill).
template <bool W8>
__global__ __launch_bounds__(DG_THREADS)
__attribute__((amdgpu_waves_per_eu(W8 ? 2 : 4)))
void decode_gemm_kernel(const void* __restrict__ w,
                        const float* __restrict__ scale,
                        const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                        int rows, int K, int out) {
  constexpr int KS = DgStage<W8>::KS;
  __shared__ f32x4 part[DG_WAVES - 1][64];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int row0 = blockIdx.x * DG_TILE;

  // A: weight row row0 + n (clamped), B: x row n (row 0 for n >= rows)
  const int wrow = row0 + n < out ? row0 + n : out - 1;
  const char* wp = reinterpret_cast<const char*>(w) +
                   (long)wrow * K * (W8 ? 1 : 2) + 64 * g;
  const bool has_x = n < rows;
  const bf16_t* xp = x + (has_x ? (long)n * K : 0) + (KS / 4) * g;

  // whole k-steps: this wave owns wave, wave + 4, ...; `mine` of them
  const int nfull = K / KS;
  const int mine = (nfull - wave + DG_WAVES - 1) / DG_WAVES;
  f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
  DgStage<W8> st[DG_NS];
  const long s0 = wave;  // global step of local step i: s0 + DG_WAVES * i
  if (mine >= DG_PF) {
    static_assert(DG_PF == 2 && DG_NS == 3, "the ring below is written out");
    dg_load<W8>(st[0], wp, xp, s0);
    dg_load<W8>(st[1], wp, xp, s0 + DG_WAVES);
    // Whole turns of the ring, branch-free inside: each of the three phases
    // loads local step i + 2 and consumes step i.  The 0..2 steps that do
    // not fill a turn are loaded and consumed after the loop.
    const int turns = (mine - DG_PF) / DG_NS;
    const int rem = (mine - DG_PF) % DG_NS;
    long nxt = s0 + DG_WAVES * DG_PF;
    for (int t = 0; t < turns; ++t, nxt += DG_WAVES * DG_NS) {
      dg_load<W8>(st[2], wp, xp, nxt);
      dg_mma<W8>(st[0], acc);
      dg_load<W8>(st[0], wp, xp, nxt + DG_WAVES);
      dg_mma<W8>(st[1], acc);
      dg_load<W8>(st[1], wp, xp, nxt + 2 * DG_WAVES);
      dg_mma<W8>(st[2], acc);
    }
    if (rem >= 1) dg_load<W8>(st[2], wp, xp, nxt);
    dg_mma<W8>(st[0], acc);
    if (rem >= 2) dg_load<W8>(st[0], wp, xp, nxt + DG_WAVES);
    dg_mma<W8>(st[1], acc);
    if (rem >= 1) dg_mma<W8>(st[2], acc);
    if (rem >= 2) dg_mma<W8>(st[0], acc);
  } else if (mine == 1) {
    dg_load<W8>(st[0], wp, xp, s0);
    dg_mma<W8>(st[0], acc);
  }
  // the partial step at the end of K, if any, belongs to the next wave in turn
  if (nfull * KS < K && wave == nfull % DG_WAVES) {
    const bool inside = (long)nfull * KS + (KS / 4) * g < K;
#pragma unroll
    for (int j = 0; j < 4; ++j) st[0].a[j] = i32x4{0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < DgStage<W8>::NB; ++p)
      st[0].b[p] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (inside) dg_load<W8>(st[0], wp, xp, nfull);
    dg_mma<W8>(st[0], acc);
  }

  // ---- merge the four waves in wave order, wave 0 stores -----------------
  // the lane holds features row0 + 4g .. 4g + 3 of batch row n
  f32x4 sum = acc[0] + acc[1];
  if (wave > 0) part[wave - 1][lane] = sum;
  __syncthreads();
  if (wave != 0 || !has_x) return;
#pragma unroll
  for (int v = 0; v < DG_WAVES - 1; ++v) sum += part[v][lane];
  const int o0 = row0 + 4 * g;
  if (W8) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      sum[r] *= scale[o0 + r < out ? o0 + r : out - 1];
  }
  bf16x4 ov;
#pragma unroll
  for (int r = 0; r < 4; ++r) ov[r] = dg_bf16bits(sum[r]);
  bf16_t* yp = y + (long)n * out + o0;
  if ((out & 3) == 0) {  // y rows are 8-byte aligned, groups of 4 are whole
    if (o0 < out) *reinterpret_cast<bf16x4*>(yp) = ov;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (o0 + r < out) reinterpret_cast<short*>(yp)[r] = ov[r];
  }
}

}  // namespace

// scale is read only when w8 != 0.  All shape checks are the binding's.
extern "C" void fs_decode_gemm(const void* w, const float* scale,
                               const void* x, void* y, int rows, int K,
                               int out, int w8, hipStream_t s) {
  const dim3 grid((out + DG_TILE - 1) / DG_TILE);
  if (w8)
    hipLaunchKernelGGL((decode_gemm_kernel<true>), grid, dim3(DG_THREADS), 0,
                       s, w, scale, (const bf16_t*)x, (bf16_t*)y, rows, K,
                       out);
  else
    hipLaunchKernelGGL((decode_gemm_kernel<false>), grid, dim3(DG_THREADS), 0,
                       s, w, scale, (const bf16_t*)x, (bf16_t*)y, rows, K,
                       out);
}
