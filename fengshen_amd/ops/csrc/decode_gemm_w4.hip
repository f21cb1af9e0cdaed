// Split-K weight-streaming GEMM for int4 weights, 1..16-row decode on MI355X
// (gfx950).
//
//   Y[rows, out] = X[rows, K] . dequant(W)^T     fp32 accumulate, bf16 out
//   qweight [out_pad/16, K/128, 64, 16] uint8    utils/quantize.py: pack_int4
//   scales  [K/128, out_pad] bf16                one per (feature, 128 k)
//   x       [rows, K] bf16, 1 <= rows <= 16, K % 128 == 0
// out_pad is out rounded up to 64; pad rows hold u = 8 (q = 0) and scale 0,
// so no weight row is clamped or predicated.
//
// Grid = (ceil(out_pad / (64 TW)), ksplit) x 256 threads.  A block owns 64 TW
// output features and one chunk of whole 128-k groups; wave w owns the TW
// 16-row tiles w, w + 4, ... of the block over the whole chunk.  ksplit is a
// function of (K, out_pad, TW) only (w4_pick_ksplit), never of rows, and a
// column of the MFMA result depends on that column of B alone, so row i of
// the result has the same bits whatever else is in the batch.
//
// x goes through LDS once per block.  Thread (n = tid / 16, c = tid % 16)
// copies, for each group of the chunk, the 16 bytes x[n, 128 G + 8 c .. + 8]
// (16 lanes read 256 contiguous bytes) to
//     xs + 4096 G + 256 c + 16 (n ^ c),
// zeros for n >= rows.  The B fragment of MFMA j of lane (n = l % 16,
// g = l / 16) is k slot (g, e) <-> k = 128 G + 32 g + 8 j + e, i.e. piece
// c = 4 g + j of row n: one ds_read_b128 at 256 c + 16 (n ^ c).  The XOR
// makes both sides conflict-free (docs/KERNELS.md has the arithmetic).  One
// barrier follows the copy; the k loop has none.  Chunks of more than
// W4_MAXG groups (only with an explicit ksplit) take several such passes.
//
// Weights go HBM -> registers -> MFMA, no LDS.  A wave step is one group of
// each of its TW tiles: one 16-byte load per lane and tile (1 KB contiguous
// per instruction) plus the lane's four bf16 scales (8 bytes).  W4_PF steps
// are in flight ahead of the MFMAs in a ring of W4_PF + 1 register stages
// indexed at compile time.  Every load of the loop is unconditional: the
// group index is clamped to the last group of the chunk instead, so the
// loads past its end read again what the wave has just fetched, and the
// compiler waits with a counted vmcnt.
//
// Unpack: ((dw >> 4 i) & 0x000F000F) | 0x43004300 is the bf16 pair
// (128 + u[2i], 128 + u[2i+1]), exact because a bf16 in [128, 256) has an ulp
// of 1.  128 + u = 136 + q, so the group's MFMAs start from
// -136 sum_{k in group} x[n, k], which the staging threads compute once per
// block (16-lane butterfly, fp32) and keep in LDS next to x.  Each group is
// accumulated into temporaries of its own and folded into the accumulator as
// acc = fma(scale, tmp, acc).
//
// ksplit == 1 stores bf16 y; otherwise every block stores its fp32 partial
// to part[split, n, 0..out_pad) and w4_reduce_kernel sums the splits in
// order.  No atomics: the same inputs give the same bits.

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

constexpr int W4_THREADS = 256;
constexpr int W4_MAXG = 8;           // groups of x in LDS at a time
constexpr int W4_XG_BYTES = 4096;    // 16 rows x 128 k x 2 bytes
constexpr int W4_MIN_BLOCKS = 512;   // what ksplit = 0 aims for
constexpr int W4_DEFAULT_TW = 1;     // scripts/decode_gemm_w4_bench.py

template <int TW>
struct W4Stage {
  u32x4 w[TW];  // the lane's 32 weights of one group, per tile
  u32x2 s[TW];  // the lane's four scales of that group, per tile
};

__device__ __forceinline__ short w4_bf16bits(float f) {
  return __builtin_bit_cast(short, (__bf16)f);
}

// 8 offset-binary nibbles -> bf16 128 + u, in bf16x8 element order
__device__ __forceinline__ bf16x8 w4_cvt(unsigned dw) {
  u32x4 v;
#pragma unroll
  for (int i = 0; i < 4; ++i)
    v[i] = ((dw >> (4 * i)) & 0x000F000Fu) | 0x43004300u;
  return __builtin_bit_cast(bf16x8, v);
}

// wp / sp point at the lane's piece of group 0 of each tile
template <int TW>
__device__ __forceinline__ void w4_load(W4Stage<TW>& st,
                                        const u32x4* const (&wp)[TW],
                                        const char* const (&sp)[TW], int G,
                                        long sstride) {
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    st.w[i] = wp[i][(long)G * 64];
    st.s[i] = *reinterpret_cast<const u32x2*>(sp[i] + G * sstride);
  }
}

// one group: xg / cg are the group's x image and bias terms in LDS
template <int TW>
__device__ __forceinline__ void w4_step(const W4Stage<TW>& st, const char* xg,
                                        const float* cg,
                                        const int (&roff)[4], int n,
                                        f32x4 (&acc)[TW]) {
  bf16x8 b[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    b[j] = *reinterpret_cast<const bf16x8*>(xg + roff[j]);
  const float nc = cg[n];  // -136 sum of x[n] over the group
  f32x4 t0[TW], t1[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    t0[i] = f32x4{nc, nc, nc, nc};
    t1[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  // j outer, tile inner, two temporaries per tile: no MFMA reads the result
  // of the one before it
#pragma unroll
  for (int j = 0; j < 4; ++j) {
#pragma unroll
    for (int i = 0; i < TW; ++i) {
      if (j & 1)
        t1[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w4_cvt(st.w[i][j]),
                                                        b[j], t1[i], 0, 0, 0);
      else
        t0[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w4_cvt(st.w[i][j]),
                                                        b[j], t0[i], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const f32x4 d = t0[i] + t1[i];
    acc[i][0] = fmaf(__uint_as_float(st.s[i][0] << 16), d[0], acc[i][0]);
    acc[i][1] = fmaf(__uint_as_float(st.s[i][0] & 0xFFFF0000u), d[1],
                     acc[i][1]);
    acc[i][2] = fmaf(__uint_as_float(st.s[i][1] << 16), d[2], acc[i][2]);
    acc[i][3] = fmaf(__uint_as_float(st.s[i][1] & 0xFFFF0000u), d[3],
                     acc[i][3]);
  }
}

template <int TW>
__global__ __launch_bounds__(W4_THREADS, TW == 1 ? 4 : 3)
void decode_gemm_w4_kernel(const u32x4* __restrict__ qw,
                           const bf16_t* __restrict__ scales,
                           const bf16_t* __restrict__ x,
                           bf16_t* __restrict__ y, float* __restrict__ part,
                           int rows, int K, int out, int out_pad) {
  constexpr int PF = 8 / TW;   // steps in flight: 8 weight loads per wave
  constexpr int NS = PF + 1;   // register stages
  __shared__ __attribute__((aligned(16))) char xs[W4_MAXG * W4_XG_BYTES];
  __shared__ float cs[W4_MAXG * 16];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, n = lane & 15;
  const int ngroups = K >> 7, ntiles = out_pad >> 4;

  // this block's groups: the first K/128 % ksplit splits get one more
  const int ksplit = gridDim.y, split = blockIdx.y;
  const int base = ngroups / ksplit, rem = ngroups % ksplit;
  const int G0 = split * base + (split < rem ? split : rem);
  const int ng = base + (split < rem ? 1 : 0);

  // this wave's tiles; a tile past the end (TW = 2, odd number of 64-row
  // blocks) streams the last tile again and stores nothing
  int tile[TW];
  const u32x4* wp[TW];
  const char* sp[TW];
  const long sstride = (long)out_pad * 2;
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int t = (blockIdx.x * TW + i) * 4 + wave;
    tile[i] = t < ntiles ? t : -1;
    const int tc = t < ntiles ? t : ntiles - 1;
    wp[i] = qw + (long)tc * ngroups * 64 + lane;
    sp[i] = reinterpret_cast<const char*>(scales) + (16 * tc + 4 * g) * 2;
  }

  // staging: thread (sn, c) owns piece c of row sn of every group
  const int sn = tid >> 4, c = tid & 15;
  char* const sw = xs + 256 * c + 16 * (sn ^ c);
  int roff[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    roff[j] = 256 * (4 * g + j) + 16 * (n ^ (4 * g + j));

  f32x4 acc[TW];
#pragma unroll
  for (int i = 0; i < TW; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  W4Stage<TW> st[NS];
  const int glast = G0 + ng - 1;  // loads past the chunk re-read its end

  for (int p0 = 0; p0 < ng; p0 += W4_MAXG) {
    const int np = ng - p0 < W4_MAXG ? ng - p0 : W4_MAXG;
    const int Gp = G0 + p0;
    // the first PF steps' weights are on their way while x is staged
#pragma unroll
    for (int s = 0; s < PF; ++s)
      w4_load<TW>(st[s], wp, sp, Gp + s < glast ? Gp + s : glast, sstride);

    if (p0) __syncthreads();  // the previous pass has read its x
    if (sn < rows) {
      const bf16_t* xp = x + (long)sn * K + (long)Gp * 128 + 8 * c;
      for (int Gb = 0; Gb < np; Gb += 5) {  // five loads in flight
        bf16x8 v[5];
#pragma unroll
        for (int u = 0; u < 5; ++u)
          if (Gb + u < np)
            v[u] = *reinterpret_cast<const bf16x8*>(xp + (Gb + u) * 128);
#pragma unroll
        for (int u = 0; u < 5; ++u) {
          const int G = Gb + u;
          if (G >= np) break;
          *reinterpret_cast<bf16x8*>(sw + G * W4_XG_BYTES) = v[u];
          float sum = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e)
            sum += __uint_as_float((unsigned)(unsigned short)v[u][e] << 16);
#pragma unroll
          for (int m = 1; m < 16; m <<= 1) sum += __shfl_xor(sum, m, 16);
          if (c == 0) cs[G * 16 + sn] = -136.f * sum;
        }
      }
    } else {
      for (int G = 0; G < np; ++G) {
        *reinterpret_cast<bf16x8*>(sw + G * W4_XG_BYTES) =
            bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
        if (c == 0) cs[G * 16 + sn] = 0.f;
      }
    }
    __syncthreads();

    // step i of the pass consumes stage i % NS and loads step i + PF
    for (int b0 = 0; b0 < np; b0 += NS) {
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const int i = b0 + s;
        if (i >= np) break;
        const int Gn = Gp + i + PF;
        w4_load<TW>(st[(s + PF) % NS], wp, sp, Gn < glast ? Gn : glast,
                    sstride);
        w4_step<TW>(st[s], xs + i * W4_XG_BYTES, cs + i * 16, roff, n, acc);
      }
    }
  }

  // the lane holds features 16 tile + 4 g .. + 3 of batch row n
  if (n >= rows) return;
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    if (tile[i] < 0) continue;
    const int o0 = 16 * tile[i] + 4 * g;
    if (ksplit > 1) {
      *reinterpret_cast<f32x4*>(part + ((long)split * rows + n) * out_pad +
                                o0) = acc[i];
      continue;
    }
    bf16x4 ov;
#pragma unroll
    for (int r = 0; r < 4; ++r) ov[r] = w4_bf16bits(acc[i][r]);
    bf16_t* yp = y + (long)n * out + o0;
    if ((out & 3) == 0) {  // y rows are 8-byte aligned, groups of 4 are whole
      if (o0 < out) *reinterpret_cast<bf16x4*>(yp) = ov;
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (o0 + r < out) reinterpret_cast<short*>(yp)[r] = ov[r];
    }
  }
}

// y[n, o] = bf16(sum over splits, in split order, of part[s, n, o])
__global__ __launch_bounds__(W4_THREADS)
void w4_reduce_kernel(const float* __restrict__ part, bf16_t* __restrict__ y,
                      int rows, int out, int out_pad, int ksplit) {
  const long idx = (long)blockIdx.x * W4_THREADS + threadIdx.x;
  if (idx >= (long)rows * out) return;
  const int n = (int)(idx / out), o = (int)(idx % out);
  const float* p = part + (long)n * out_pad + o;
  const long sstride = (long)rows * out_pad;
  float sum = p[0];
  for (int s = 1; s < ksplit; ++s) sum += p[s * sstride];
  reinterpret_cast<short*>(y)[idx] = w4_bf16bits(sum);
}

int w4_pick_ksplit(int ngroups, int out_pad, int tw) {
  const int nbx = (out_pad + 64 * tw - 1) / (64 * tw);
  const int lo = (ngroups + W4_MAXG - 1) / W4_MAXG;   // the chunk fits in LDS
  const int hi = ngroups >= 2 ? ngroups / 2 : 1;      // and has >= 2 groups
  const int want = (W4_MIN_BLOCKS + nbx - 1) / nbx;
  const int ks = want < hi ? want : hi;
  return ks > lo ? ks : lo;
}

}  // namespace

// tw = 0: the default.  All shape checks are the binding's.
extern "C" int fs_decode_gemm_w4_tw(int tw) {
  return tw == 0 ? W4_DEFAULT_TW : tw;
}

// the split count that ksplit = 0 stands for; depends on shapes only
extern "C" int fs_decode_gemm_w4_ksplit(int K, int out_pad, int tw) {
  return w4_pick_ksplit(K / 128, out_pad, fs_decode_gemm_w4_tw(tw));
}

// part is read and written only when ksplit > 1: [ksplit, rows, out_pad]
extern "C" void fs_decode_gemm_w4(const void* qw, const void* scales,
                                  const void* x, void* y, float* part,
                                  int rows, int K, int out, int out_pad,
                                  int ksplit, int tw, hipStream_t s) {
  tw = fs_decode_gemm_w4_tw(tw);
  const dim3 grid((out_pad + 64 * tw - 1) / (64 * tw), ksplit);
  if (tw == 2)
    hipLaunchKernelGGL((decode_gemm_w4_kernel<2>), grid, dim3(W4_THREADS), 0,
                       s, (const u32x4*)qw, (const bf16_t*)scales,
                       (const bf16_t*)x, (bf16_t*)y, part, rows, K, out,
                       out_pad);
  else
    hipLaunchKernelGGL((decode_gemm_w4_kernel<1>), grid, dim3(W4_THREADS), 0,
                       s, (const u32x4*)qw, (const bf16_t*)scales,
                       (const bf16_t*)x, (bf16_t*)y, part, rows, K, out,
                       out_pad);
  if (ksplit > 1) {
    const long total = (long)rows * out;
    hipLaunchKernelGGL(w4_reduce_kernel,
                       dim3((total + W4_THREADS - 1) / W4_THREADS),
                       dim3(W4_THREADS), 0, s, part, (bf16_t*)y, rows, out,
                       out_pad, ksplit);
  }
}
