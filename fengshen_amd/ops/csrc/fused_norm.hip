// Register-resident RMSNorm with the residual adds fused in (gfx950).
//
// One row per block iteration, 256 threads, V = ceil(H / 2048) 8-element
// vectors per thread (16 B for bf16/fp16, 32 B for fp32); thread t owns
// vectors t, t + 256, ... of every row of its grid-stride loop, so:
//   * the row of x (and delta / g_h / g_res) is read from HBM once and lives
//     in registers; nothing but the cross-wave partial sums touches LDS
//   * the next row's loads are issued before the current row's reduction,
//     so HBM latency overlaps the barrier
//   * the weight-gradient partial sums stay in registers across rows; each
//     block stores one fp32 partial row to a [grid, H] workspace and a second
//     small kernel sums the partial rows per column in a fixed order (no
//     atomics, no zero-fill, bitwise reproducible)
// The cross-wave reduction is double-buffered on the row parity: a wave can
// only overwrite a buffer after passing the next row's barrier, which every
// wave reaches after its reads of that buffer, so one barrier per row is
// enough.
//
// The row sums are taken in exactly the order the LDS-staged kernels in
// kernels.hip take them as hipcc (ROCm 7.2, -O3 -ffast-math) compiles them:
// column ownership, the per-vector pair order of row_partial(), the wave
// butterfly, then (w0 + w2) + (w1 + w3); the element-wise expressions are
// associated as theirs.  So h and g are bit-identical to those kernels and a
// model's outputs do not move when it switches over.  That is why the block
// is 256 threads with up to four vectors per thread (the third is half
// populated at H = 5120) and not one vector per thread: a different
// ownership changes the sums, and one flipped bf16 ulp in 1e5 is enough to
// decorrelate the rounding of every later layer.  The equality holds for the
// compiler named above and is asserted by
// tests/test_fused_norm_gpu.py::test_bit_identical_to_composition.
//
// fwd:  sum = round_T(x + delta)           (written only when delta != null)
//       h   = sum * rsqrt(mean(sum^2) + eps) * w      (from the ROUNDED sum)
// bwd:  g   = round_T(round_T(ir*(g_h*w - xhat*mean(g_h*w*xhat))) + g_res)
//       gw  = sum_rows g_h * xhat
// H outside [256, 8192] is not covered: fs_fused_norm_vectors() returns 0 and
// the caller dispatches to the LDS-staged kernels in kernels.hip.

#include "common.h"

enum FsDtype { FS_F32 = 0, FS_BF16 = 1, FS_F16 = 2 };

namespace {

template <typename T>
__device__ __forceinline__ float round_to(float v) {
  return to_f32<T>(from_f32<T>(v));
}

constexpr int FN_THREADS = 256;
constexpr int FN_WAVES = FN_THREADS / WAVE_SIZE;

// Sum over the 4 waves of the block; every thread returns the same bits, in
// the association block_reduce_sum() produces for 4 waves.
__device__ __forceinline__ float fn_block_sum(float v, float* red) {
#pragma clang fp reassociate(off)
  v = wave_reduce_sum(v);
  if ((threadIdx.x & (WAVE_SIZE - 1)) == 0) red[threadIdx.x / WAVE_SIZE] = v;
  __syncthreads();
  const float a = red[0] + red[2];
  const float b = red[1] + red[3];
  return a + b;
}

// acc + sum_i a[i] * b[i] over one 8-element vector, in the pair order the
// LDS kernels' reductions compile to: two lanes of products, pairs (6,7),
// (2,3), (4,5), (0,1) chained by fma, the two lanes added, then acc.
__device__ __forceinline__ float row_partial(float acc, const float (&a)[8],
                                             const float (&b)[8]) {
#pragma clang fp reassociate(off) contract(off)
  float lo = a[6] * b[6];
  float hi = a[7] * b[7];
  lo = __builtin_fmaf(a[2], b[2], lo);
  hi = __builtin_fmaf(a[3], b[3], hi);
  lo = __builtin_fmaf(a[4], b[4], lo);
  hi = __builtin_fmaf(a[5], b[5], hi);
  lo = __builtin_fmaf(a[0], b[0], lo);
  hi = __builtin_fmaf(a[1], b[1], hi);
  const float s = lo + hi;
  return acc + s;
}

// The element-wise forms below are written in the association the LDS
// kernels compile to, with reassociation off so that it is kept.
__device__ __forceinline__ float norm_out(float x, float ir, float w) {
#pragma clang fp reassociate(off)
  return (w * ir) * x;
}

__device__ __forceinline__ float norm_grad(float gyw, float xh, float dot,
                                           float ir) {
#pragma clang fp reassociate(off) contract(off)
  return __builtin_fmaf(-dot, xh, gyw) * ir;
}

// round_T(inner) + g_res.  For T = float the rounding is the one of the
// product that ends norm_grad(); the empty asm keeps the backend from fusing
// that product into this add (an fma would skip it).  The 16-bit types round
// explicitly and need no such fence.
template <typename T>
__device__ __forceinline__ float add_rounded(float inner, float r) {
  float t = round_to<T>(inner);
  if constexpr (sizeof(T) == 4) asm volatile("" : "+v"(t));
  return t + r;
}

__device__ __forceinline__ float row_mean(float sum, int H) {
#pragma clang fp reassociate(off)
  return sum / H;
}

__device__ __forceinline__ void zero8(float (&v)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = 0.f;
}

// A row vector as loaded (16 B for bf16/fp16): the prefetched next row waits
// in this form, at half the registers of its fp32 expansion.
template <typename T> struct raw8 { short8_t v; };
template <> struct raw8<float> { float4_t lo, hi; };

template <typename T>
__device__ __forceinline__ raw8<T> raw_zero() {
  raw8<T> r;
  r.v = short8_t{0, 0, 0, 0, 0, 0, 0, 0};
  return r;
}
template <>
__device__ __forceinline__ raw8<float> raw_zero<float>() {
  raw8<float> r;
  r.lo = float4_t{0.f, 0.f, 0.f, 0.f};
  r.hi = r.lo;
  return r;
}

template <typename T>
__device__ __forceinline__ raw8<T> raw_load(const T* p) {
  raw8<T> r;
  r.v = *reinterpret_cast<const short8_t*>(p);
  return r;
}
template <>
__device__ __forceinline__ raw8<float> raw_load<float>(const float* p) {
  raw8<float> r;
  r.lo = reinterpret_cast<const float4_t*>(p)[0];
  r.hi = reinterpret_cast<const float4_t*>(p)[1];
  return r;
}

template <typename T>
__device__ __forceinline__ void unpack8(const raw8<T>& r, float (&out)[8]) {
  load8<T>(reinterpret_cast<const T*>(&r.v), out);
}
template <>
__device__ __forceinline__ void unpack8<float>(const raw8<float>& r,
                                               float (&out)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) { out[i] = r.lo[i]; out[4 + i] = r.hi[i]; }
}

template <typename T, int V, bool HAS_DELTA>
__global__ __launch_bounds__(FN_THREADS) void res_rms_norm_fwd_kernel(
    const T* __restrict__ x, const T* __restrict__ delta,
    const T* __restrict__ w, T* __restrict__ sum_out, T* __restrict__ h_out,
    float* __restrict__ invrms, int rows, int H, float eps) {
  __shared__ float red[2][FN_WAVES];
  int c[V];
  bool act[V];
  raw8<T> wr[V], xr[V], dr[V];
  int row = blockIdx.x;
#pragma unroll
  for (int p = 0; p < V; ++p) {
    c[p] = (threadIdx.x + p * FN_THREADS) * 8;
    act[p] = c[p] < H;
    wr[p] = xr[p] = dr[p] = raw_zero<T>();
    if (act[p]) {
      wr[p] = raw_load<T>(w + c[p]);
      if (row < rows) {
        xr[p] = raw_load<T>(x + (long)row * H + c[p]);
        if (HAS_DELTA) dr[p] = raw_load<T>(delta + (long)row * H + c[p]);
      }
    }
  }
  int buf = 0;
  for (; row < rows; row += gridDim.x) {
    float v[V][8];
#pragma unroll
    for (int p = 0; p < V; ++p) {
      unpack8<T>(xr[p], v[p]);
      if (HAS_DELTA) {
        float dv[8];
        unpack8<T>(dr[p], dv);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[p][i] = round_to<T>(v[p][i] + dv[i]);
      }
    }
    const int nrow = row + gridDim.x;
    if (nrow < rows) {  // next row in flight across the barrier
#pragma unroll
      for (int p = 0; p < V; ++p)
        if (act[p]) {
          xr[p] = raw_load<T>(x + (long)nrow * H + c[p]);
          if (HAS_DELTA) dr[p] = raw_load<T>(delta + (long)nrow * H + c[p]);
        }
    }
    float ss = 0.f;
#pragma unroll
    for (int p = 0; p < V; ++p) {
      if (HAS_DELTA && act[p]) store8<T>(sum_out + (long)row * H + c[p], v[p]);
      ss = row_partial(ss, v[p], v[p]);
    }
    ss = fn_block_sum(ss, red[buf]);
    buf ^= 1;
    const float ir = rsqrtf(ss / H + eps);
    if (threadIdx.x == 0) invrms[row] = ir;
#pragma unroll
    for (int p = 0; p < V; ++p)
      if (act[p]) {
        float wv[8], o[8];
        unpack8<T>(wr[p], wv);
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = norm_out(v[p][i], ir, wv[i]);
        store8<T>(h_out + (long)row * H + c[p], o);
      }
  }
}

template <typename T, int V, bool HAS_RES>
__global__ __launch_bounds__(FN_THREADS) void res_rms_norm_bwd_kernel(
    const T* __restrict__ gh, const T* __restrict__ gres,
    const T* __restrict__ x, const T* __restrict__ w,
    const float* __restrict__ invrms, T* __restrict__ g_out,
    float* __restrict__ gw_part, int rows, int H) {
  __shared__ float red[2][FN_WAVES];
  int c[V];
  bool act[V];
  float acc[V][8];
  raw8<T> wr[V], xr[V], gr[V], rr[V];
  int row = blockIdx.x;
#pragma unroll
  for (int p = 0; p < V; ++p) {
    c[p] = (threadIdx.x + p * FN_THREADS) * 8;
    act[p] = c[p] < H;
    zero8(acc[p]);
    wr[p] = xr[p] = gr[p] = rr[p] = raw_zero<T>();
    if (act[p]) {
      wr[p] = raw_load<T>(w + c[p]);
      if (row < rows) {
        xr[p] = raw_load<T>(x + (long)row * H + c[p]);
        gr[p] = raw_load<T>(gh + (long)row * H + c[p]);
        if (HAS_RES) rr[p] = raw_load<T>(gres + (long)row * H + c[p]);
      }
    }
  }
  int buf = 0;
  for (; row < rows; row += gridDim.x) {
    const float ir = invrms[row];
    float xh[V][8], gyw[V][8];
    raw8<T> rcur[V];
    float dot = 0.f;
#pragma unroll
    for (int p = 0; p < V; ++p) {
      float xv[8], gv[8], wv[8];
      unpack8<T>(xr[p], xv);
      unpack8<T>(gr[p], gv);
      unpack8<T>(wr[p], wv);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xh[p][i] = xv[i] * ir;
        gyw[p][i] = gv[i] * wv[i];
        acc[p][i] += gv[i] * xh[p][i];
      }
      dot = row_partial(dot, gyw[p], xh[p]);
      rcur[p] = rr[p];
    }
    const int nrow = row + gridDim.x;
    if (nrow < rows) {  // next row in flight across the barrier
#pragma unroll
      for (int p = 0; p < V; ++p)
        if (act[p]) {
          xr[p] = raw_load<T>(x + (long)nrow * H + c[p]);
          gr[p] = raw_load<T>(gh + (long)nrow * H + c[p]);
          if (HAS_RES) rr[p] = raw_load<T>(gres + (long)nrow * H + c[p]);
        }
    }
    dot = row_mean(fn_block_sum(dot, red[buf]), H);
    buf ^= 1;
#pragma unroll
    for (int p = 0; p < V; ++p)
      if (act[p]) {
        float o[8], r[8];
        unpack8<T>(rcur[p], r);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          o[i] = norm_grad(gyw[p][i], xh[p][i], dot, ir);
          if (HAS_RES) o[i] = add_rounded<T>(o[i], r[i]);
        }
        store8<T>(g_out + (long)row * H + c[p], o);
      }
  }
#pragma unroll
  for (int p = 0; p < V; ++p)
    if (act[p]) {
      float4_t* q =
          reinterpret_cast<float4_t*>(gw_part + (long)blockIdx.x * H + c[p]);
      float4_t lo = {acc[p][0], acc[p][1], acc[p][2], acc[p][3]};
      float4_t hi = {acc[p][4], acc[p][5], acc[p][6], acc[p][7]};
      q[0] = lo;
      q[1] = hi;
    }
}

// gw[col] = sum_p part[p][col], p in a fixed order: 8 interleaved slices per
// column, each summed front to back, then the 8 slice sums front to back.
template <typename T>
__global__ __launch_bounds__(512) void rms_norm_gw_reduce_kernel(
    const float* __restrict__ part, T* __restrict__ gw, int P, int H) {
  __shared__ float sm[8][64];
  const int tx = threadIdx.x & 63;
  const int ty = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + tx;
  float s = 0.f;
  if (col < H)
    for (int p = ty; p < P; p += 8) s += part[(long)p * H + col];
  sm[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && col < H) {
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) t += sm[i][tx];
    gw[col] = from_f32<T>(t);
  }
}

#define FN_DISPATCH_DTYPE(dtype, T, ...)                      \
  switch (dtype) {                                            \
    case FS_F32: { using T = float; __VA_ARGS__; break; }     \
    case FS_BF16: { using T = bf16_t; __VA_ARGS__; break; }   \
    case FS_F16: { using T = fp16_t; __VA_ARGS__; break; }    \
  }

#define FN_DISPATCH_V(nv, V, ...)                             \
  switch (nv) {                                               \
    case 1: { constexpr int V = 1; __VA_ARGS__; break; }      \
    case 2: { constexpr int V = 2; __VA_ARGS__; break; }      \
    case 3: { constexpr int V = 3; __VA_ARGS__; break; }      \
    case 4: { constexpr int V = 4; __VA_ARGS__; break; }      \
  }

#define FN_DISPATCH_BOOL(flag, B, ...)                        \
  if (flag) { constexpr bool B = true; __VA_ARGS__; }         \
  else { constexpr bool B = false; __VA_ARGS__; }

}  // namespace

extern "C" {

// Vectors per thread of the register-resident kernels for this H, or 0 when
// H is left to the LDS-staged kernels: rows under half a wave of vectors
// (H < 256) would idle nearly the whole block, rows over 8192 need more than
// four vectors per thread.
int fs_fused_norm_vectors(int H) {
  if (H % 8 != 0 || H < 256 || H > 8192) return 0;
  return (H + FN_THREADS * 8 - 1) / (FN_THREADS * 8);
}

// Backward grid: at most 1024 blocks (4 per CU), which keeps the [grid, H]
// fp32 partials at 21 MB each way at H = 5120, 1.6 % of the row traffic at
// 32768 rows.
int fs_fused_norm_bwd_grid(int rows, int H) {
  if (fs_fused_norm_vectors(H) == 0) return 0;
  const int g = rows < 1024 ? rows : 1024;
  return g < 1 ? 1 : g;
}

void fs_res_rms_norm_fwd(const void* x, const void* delta, const void* w,
                         void* sum_out, void* h_out, float* invrms, int rows,
                         int H, float eps, int dtype, hipStream_t s) {
  const int nv = fs_fused_norm_vectors(H);
  int grid = rows < FS_MAX_BLOCKS ? rows : FS_MAX_BLOCKS;
  if (grid < 1) grid = 1;
  FN_DISPATCH_DTYPE(dtype, T,
    FN_DISPATCH_V(nv, V,
      FN_DISPATCH_BOOL(delta != nullptr, HD,
        hipLaunchKernelGGL((res_rms_norm_fwd_kernel<T, V, HD>), dim3(grid),
                           dim3(FN_THREADS), 0, s, (const T*)x,
                           (const T*)delta, (const T*)w, (T*)sum_out,
                           (T*)h_out, invrms, rows, H, eps))));
}

// gw_part: [fs_fused_norm_bwd_grid(rows, H), H] fp32 workspace, fully written.
void fs_res_rms_norm_bwd(const void* gh, const void* gres, const void* x,
                         const void* w, const float* invrms, void* g_out,
                         float* gw_part, void* gw, int rows, int H, int dtype,
                         hipStream_t s) {
  const int nv = fs_fused_norm_vectors(H);
  const int grid = fs_fused_norm_bwd_grid(rows, H);
  FN_DISPATCH_DTYPE(dtype, T,
    FN_DISPATCH_V(nv, V,
      FN_DISPATCH_BOOL(gres != nullptr, HR,
        hipLaunchKernelGGL((res_rms_norm_bwd_kernel<T, V, HR>), dim3(grid),
                           dim3(FN_THREADS), 0, s, (const T*)gh,
                           (const T*)gres, (const T*)x, (const T*)w, invrms,
                           (T*)g_out, gw_part, rows, H))));
  FN_DISPATCH_DTYPE(dtype, T,
    hipLaunchKernelGGL((rms_norm_gw_reduce_kernel<T>), dim3((H + 63) / 64),
                       dim3(512), 0, s, (const float*)gw_part, (T*)gw, grid,
                       H));
}

}  // extern "C"
