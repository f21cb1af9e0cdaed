// Split-KV grouped decode attention over an int8 KV cache (gfx950), and the
// kernel that quantises prefilled K/V rows into that cache.
//
// Cache format: K and V are int8 [b, nkv, L, D], symmetric, with one fp32
// scale per cached row, ksc / vsc [b, nkv, L].  For a row x[0..D) in fp32:
//   amax = max|x|, scale = amax / 127, inv = amax > 0 ? 127 / amax : 0,
//   q = clamp(rint(x * inv), -127, 127), dequant = q * scale
// (q8_row_scale / q8_pack16 below, used by both kernels).
//
// decode_split_q8_kernel is a sibling of decode_split_kernel
// (decode_attn.hip): same grid (nsplit, nkv * ceil(G/16), b) x 256 threads,
// same chunking from pos_b inside the kernel, four waves taking 64-key tiles
// round-robin with private (m, l, O), one merge through LDS, the same fp32
// partials [b, nh, nsplit, D+2] merged by decode_combine_kernel.  What
// differs is how K and V get from HBM to the MFMA operands:
//   K   a lane's 16-byte load is 16 int8 of key 16t + l%16, elements
//       d = 64c + 16(l/16) + (0..15).  Bytes 0-7 become the A fragment of
//       k step 2c, bytes 8-15 that of k step 2c+1; the query fragments use
//       the same d <-> k-slot map, and the sum over k does not mind the
//       order.  int8 -> bf16 is exact.  The row scale multiplies the score
//       after the MFMA; the 4 scales of a lane's 4 keys are one 16-byte load.
//   V   a lane's 16-byte load is 16 int8 of one row, converted to two bf16x8
//       and stored as chunks 2v, 2v+1 of the bf16 row-major LDS image that
//       decode_split_kernel uses (ds_voff keeps bit 0 of the chunk index, so
//       the pair is 32 contiguous bytes).  The transposed reads and the
//       Ot = Vt . Pt MFMAs are unchanged.  The row scale rides P: the B
//       operand is bf16(p * vsc[key]), l accumulates the unscaled p.
// Row pos_b: every wave quantises the roped k (fp32, not rounded to bf16
// first) and the v row of qkv in wave-uniform code before the key loop; the
// wave whose tile holds pos_b attends to these int8 values and scales, which
// are what later steps read.  Head group 0 of the split whose chunk holds
// pos_b writes them.  Rows >= pos_b of all four tensors: K/V loads are
// predicated off on the key index; a 16-byte scale load may cover such rows
// (L % 4 == 0 keeps it inside the tensor) and its values are replaced by
// select on the key index, so whatever bits they hold cannot reach the result.

#include "common.h"

// Packed fp32 VALU forms are kept out of this file's code.
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

#include "decode_split.h"

extern "C" void fs_decode_combine(const float* ws, void* ctx, int b, int nh,
                                  int d, int nsplit, hipStream_t s);

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;  // 16 int8

// ---- the cache format ------------------------------------------------------
__device__ __forceinline__ void q8_row_scale(float amax, float& scale,
                                             float& inv) {
  scale = amax / 127.f;
  inv = amax > 0.f ? 127.f / amax : 0.f;
}

__device__ __forceinline__ i32x4 q8_pack16(const float* x, float inv) {
  i32x4 out;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    unsigned int w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float r = __builtin_rintf(x[4 * i + j] * inv);
      r = __builtin_fminf(__builtin_fmaxf(r, -127.f), 127.f);
      w |= ((unsigned int)(int)r & 0xffu) << (8 * j);
    }
    out[i] = (int)w;
  }
  return out;
}

// byte j of w, sign-extended (one v_cvt_f32_i32 with a byte select)
__device__ __forceinline__ float q8_byte_f32(int w, int j) {
  return (float)((int)((unsigned int)w << (24 - 8 * j)) >> 24);
}

// 16 int8 -> bf16, exact: elements 0-7 in lo, 8-15 in hi
__device__ __forceinline__ void q8_cvt16(i32x4 raw, bf16x8& lo, bf16x8& hi) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    lo[e] = ds_bf16bits(q8_byte_f32(raw[e >> 2], e & 3));
    hi[e] = ds_bf16bits(q8_byte_f32(raw[2 + (e >> 2)], e & 3));
  }
}

__device__ __forceinline__ float q8_amax8(const float* x, float a) {
#pragma unroll
  for (int j = 0; j < 8; ++j) a = __builtin_fmaxf(a, __builtin_fabsf(x[j]));
  return a;
}

__device__ __forceinline__ void q8_bf16x8_f32(const bf16_t* p, float* x) {
  const bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = ds_bf16_f32(v[j]);
}

// Elements d0..d0+7 of a head row of qkv, roped at this position in fp32
// (rotate-half convention of decode_attn_kernel), not rounded.
template <int D, bool ROPE>
__device__ __forceinline__ void q8_rope8(const bf16_t* __restrict__ row,
                                         int d0, const float* __restrict__ cs,
                                         const float* __restrict__ sn,
                                         float* x) {
  q8_bf16x8_f32(row + d0, x);
  if (ROPE) {
    const bool lo = d0 < D / 2;
    float y[8];
    q8_bf16x8_f32(row + (lo ? d0 + D / 2 : d0 - D / 2), y);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      x[j] = x[j] * cs[d0 + j] + (lo ? -y[j] : y[j]) * sn[d0 + j];
  }
}

template <int D, bool ROPE>
__global__ __launch_bounds__(DS_THREADS)
void decode_split_q8_kernel(const bf16_t* __restrict__ qkv,
                            signed char* __restrict__ kq,
                            float* __restrict__ ksc,
                            signed char* __restrict__ vq,
                            float* __restrict__ vsc,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t,
                            const long* __restrict__ pos_p, int pos_n,
                            float* __restrict__ ws, bf16_t* __restrict__ ctx,
                            int nh, int nkv, int cache_len, float scale) {
  constexpr int NC = D / 32;         // k steps of St
  constexpr int NKL = D / 64;        // 16-byte K loads per lane and 16 keys
  constexpr int NDT = D / 16;        // 16-row tiles of Ot
  constexpr int RB = ds_rowb(D);
  constexpr int LPR = D / 16;        // lanes (16-byte loads) per V row
  constexpr int RPI = DS_TILE / LPR; // rows staged per load instruction
  constexpr int OS = D + 4;          // fp32 row stride of the merge image

  // wave-private V images; reused for the end-of-block merge
  __shared__ __attribute__((aligned(16))) char v_lds[DS_WAVES][DS_TILE * RB];
  static_assert(DS_HEADS * OS * 4 + DS_HEADS * 8 <= DS_TILE * RB, "merge");

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, hh = lane & 15;
  const int split = blockIdx.x, nsplit = gridDim.x;
  const int G = nh / nkv;
  const int ngrp = (G + DS_HEADS - 1) / DS_HEADS;
  const int kvh = blockIdx.y / ngrp, hg = blockIdx.y % ngrp;
  const int b = blockIdx.z;

  // clamped where it is read: a bad value changes keys, never an address
  long praw = pos_p[pos_n == 1 ? 0 : b];
  praw = praw < 0 ? 0 : (praw > cache_len - 1 ? cache_len - 1 : praw);
  const int pos = __builtin_amdgcn_readfirstlane((int)praw);

  const long W = (long)(nh + 2 * nkv) * D;
  const bf16_t* qrow = qkv + b * W;
  const bf16_t* knew = qrow + (long)nh * D + kvh * D;
  const bf16_t* vnew = knew + (long)nkv * D;
  const float* cs = cos_t + (long)pos * D;
  const float* sn = sin_t + (long)pos * D;
  const long soff = ((long)b * nkv + kvh) * (long)cache_len;
  const long coff = soff * D;
  const signed char* kbase = kq + coff;
  const signed char* vbase = vq + coff;
  const float* ksb = ksc + soff;
  const float* vsb = vsc + soff;

  // this split's chunk of [0, pos]: equal parts rounded up to whole tiles
  const int nkeys = pos + 1;
  const int clen = ((nkeys + nsplit - 1) / nsplit + DS_TILE - 1) & ~(DS_TILE - 1);
  const int start = split * clen;
  const int end = start + clen < nkeys ? start + clen : nkeys;

  const int vrow = lane / LPR, vl = lane % LPR;

  // Row pos of K and V, quantised from qkv by every wave (uniform control
  // flow).  K: lane (hh, g) holds d = 64c + 16g + (0..15), the row spans the
  // 4 values of g.  V: lane vl holds d = 16 vl + (0..15), the row spans LPR
  // consecutive lanes.
  i32x4 knew_q[NKL], vnew_q;
  float knew_s, vnew_s;
  {
    float x[NKL][16], amax = 0.f, inv;
#pragma unroll
    for (int c = 0; c < NKL; ++c) {
      q8_rope8<D, ROPE>(knew, 64 * c + 16 * g, cs, sn, x[c]);
      q8_rope8<D, ROPE>(knew, 64 * c + 16 * g + 8, cs, sn, x[c] + 8);
      amax = q8_amax8(x[c] + 8, q8_amax8(x[c], amax));
    }
    amax = __builtin_fmaxf(amax, ds_shfl_xor(amax, 16));
    amax = __builtin_fmaxf(amax, ds_shfl_xor(amax, 32));
    q8_row_scale(amax, knew_s, inv);
#pragma unroll
    for (int c = 0; c < NKL; ++c) knew_q[c] = q8_pack16(x[c], inv);

    float y[16];
    q8_bf16x8_f32(vnew + 16 * vl, y);
    q8_bf16x8_f32(vnew + 16 * vl + 8, y + 8);
    amax = q8_amax8(y + 8, q8_amax8(y, 0.f));
#pragma unroll
    for (int m = 1; m < LPR; m <<= 1)
      amax = __builtin_fmaxf(amax, ds_shfl_xor(amax, m));
    q8_row_scale(amax, vnew_s, inv);
    vnew_q = q8_pack16(y, inv);
  }

  // the one writer of cache row pos for this (b, KV head)
  if (hg == 0 && pos >= start && pos < end && wave == 0) {
    const long roff = coff + (long)pos * D;
    if (hh == 0) {
#pragma unroll
      for (int c = 0; c < NKL; ++c)
        *reinterpret_cast<i32x4*>(kq + roff + 64 * c + 16 * g) = knew_q[c];
    }
    if (vrow == 0) *reinterpret_cast<i32x4*>(vq + roff + 16 * vl) = vnew_q;
    if (lane == 0) {
      ksc[soff + pos] = knew_s;
      vsc[soff + pos] = vnew_s;
    }
  }

  // B operand of St: head hh of this group; k slot 8g + j of k step c holds
  // d = 64(c/2) + 16g + 8(c%2) + j, the map of the K bytes.  Absent heads 0.
  bf16x8 bq[NC];
  {
    const int hq = hg * DS_HEADS + hh;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bq[c] = ds_zero8();
      if (hq < G) {
        float x[8];
        q8_rope8<D, ROPE>(qrow + (long)(kvh * G + hq) * D,
                          64 * (c >> 1) + 16 * g + 8 * (c & 1), cs, sn, x);
#pragma unroll
        for (int j = 0; j < 8; ++j) bq[c][j] = ds_bf16bits(x[j] * scale);
      }
    }
  }

  const i32x4 zero16 = i32x4{0, 0, 0, 0};
  const f32x4 zero4 = f32x4{0.f, 0.f, 0.f, 0.f};
  // K (tile t = keys 16t + hh), V (image rows) and the scales of keys
  // 16t + 4g + (0..3) of the tile at k0; only keys < lim are read, the rest
  // are zeros.  A scale vector that starts below lim may reach past it.
  auto load_tile = [&](int k0, int lim, i32x4 (&kf)[4][NKL], i32x4 (&vf)[LPR],
                       f32x4 (&ksf)[4], f32x4 (&vsf)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = k0 + 16 * t + hh;
#pragma unroll
      for (int c = 0; c < NKL; ++c) {
        kf[t][c] = zero16;
        if (key < lim)
          kf[t][c] = *reinterpret_cast<const i32x4*>(
              kbase + (long)key * D + 64 * c + 16 * g);
      }
    }
#pragma unroll
    for (int it = 0; it < LPR; ++it) {
      const int key = k0 + it * RPI + vrow;
      vf[it] = zero16;
      if (key < lim)
        vf[it] = *reinterpret_cast<const i32x4*>(
            vbase + (long)key * D + 16 * vl);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = k0 + 16 * t + 4 * g;
      ksf[t] = zero4;
      vsf[t] = zero4;
      if (key < lim) {
        ksf[t] = *reinterpret_cast<const f32x4*>(ksb + key);
        vsf[t] = *reinterpret_cast<const f32x4*>(vsb + key);
      }
    }
  };

  char* vt = v_lds[wave];
  // transposed read: lane i of a group addresses row i>>2, columns 4(i&3)
  const int trow = 4 * g + (hh >> 2);
  const int tch = (hh & 3) >> 1, tbyte = 8 * (hh & 1);

  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = zero4;
  float m_run = DS_NEG, l_run = 0.f;  // of head hh; l is this lane's share

  i32x4 kr[4][NKL], vr[LPR];
  f32x4 ksr[4], vsr[4];
  int k0 = start + DS_TILE * wave;
  load_tile(k0, k0 < end ? pos : 0, kr, vr, ksr, vsr);
  for (; k0 < end; k0 += DS_TILE * DS_WAVES) {
    // row pos of K and V is the one quantised above (wave-uniform branch)
    if (pos >= k0 && pos < k0 + DS_TILE) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (k0 + 16 * t + hh == pos) {
#pragma unroll
          for (int c = 0; c < NKL; ++c) kr[t][c] = knew_q[c];
        }
#pragma unroll
      for (int it = 0; it < LPR; ++it)
        if (k0 + it * RPI + vrow == pos) vr[it] = vnew_q;
    }
    // one store writes even chunks only, the other odd ones: 4 slots mod 8
    // for 8 lanes, a 2-way bank conflict (docs/KERNELS.md has the arithmetic)
#pragma unroll
    for (int it = 0; it < LPR; ++it) {
      bf16x8 lo, hi;
      q8_cvt16(vr[it], lo, hi);
      const int row = it * RPI + vrow;
      *reinterpret_cast<bf16x8*>(vt + ds_voff<RB>(row, 2 * vl)) = lo;
      *reinterpret_cast<bf16x8*>(vt + ds_voff<RB>(row, 2 * vl + 1)) = hi;
    }

    // next tile's loads go out before this tile's MFMAs
    i32x4 kn[4][NKL], vn[LPR];
    f32x4 ksn[4], vsn[4];
    const int k1 = k0 + DS_TILE * DS_WAVES;
    load_tile(k1, k1 < end ? pos : 0, kn, vn, ksn, vsn);

    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = zero4;
#pragma unroll
      for (int c = 0; c < NKL; ++c) {
        bf16x8 lo, hi;
        q8_cvt16(kr[t][c], lo, hi);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(lo, bq[2 * c], s[t],
                                                       0, 0, 0);
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(hi, bq[2 * c + 1],
                                                       s[t], 0, 0, 0);
      }
    }
    // s[t][r] = q . (int8 row) of key k0 + 16t + 4g + r for head hh; the
    // row scale makes it the score.  Scales of keys >= pos are not taken
    // from memory.
    float tmax = DS_NEG;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kidx = k0 + 16 * t + 4 * g + r;
        const float ks = kidx < pos ? ksr[t][r] : knew_s;
        s[t][r] = kidx <= pos ? s[t][r] * ks : DS_NEG;
        tmax = __builtin_fmaxf(tmax, s[t][r]);
      }
    tmax = __builtin_fmaxf(tmax, ds_shfl_xor(tmax, 16));
    tmax = __builtin_fmaxf(tmax, ds_shfl_xor(tmax, 32));
    const float m_new = __builtin_fmaxf(m_run, tmax);
    const float alpha = ds_exp(m_run - m_new);
    m_run = m_new;
    float psum = 0.f;
    bf16x8 pb[2];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kidx = k0 + 16 * t + 4 * g + r;
        const float p = kidx <= pos ? ds_exp(s[t][r] - m_new) : 0.f;
        const float vs = kidx < pos ? vsr[t][r] : vnew_s;
        psum += p;
        pb[t >> 1][4 * (t & 1) + r] = ds_bf16bits(p * vs);
      }
    l_run = l_run * alpha + psum;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[dt] *= alpha;

    ds_wait_lds();  // this wave's V image is complete
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
      for (int pp = 0; pp < 2; ++pp) {
        const int r0 = 32 * pp + trow;
        const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_bf16x4*)(vt + ds_voff<RB>(r0, 2 * dt + tch) + tbyte));
        const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
            (lds_bf16x4*)(vt + ds_voff<RB>(r0 + 16, 2 * dt + tch) + tbyte));
        const bf16x8 a = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, pb[pp], o[dt],
                                                        0, 0, 0);
      }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
      for (int c = 0; c < NKL; ++c) kr[t][c] = kn[t][c];
      ksr[t] = ksn[t];
      vsr[t] = vsn[t];
    }
#pragma unroll
    for (int it = 0; it < LPR; ++it) vr[it] = vn[it];
  }

  // ---- merge the four wave states in wave order ---------------------------
  l_run += ds_shfl_xor(l_run, 16);
  l_run += ds_shfl_xor(l_run, 32);
  ds_wait_lds();
  float* st = reinterpret_cast<float*>(vt);  // [16][OS] O, then [16][2] m, l
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt)
    *reinterpret_cast<f32x4*>(st + hh * OS + 16 * dt + 4 * g) = o[dt];
  if (g == 0) {
    st[DS_HEADS * OS + 2 * hh] = m_run;
    st[DS_HEADS * OS + 2 * hh + 1] = l_run;
  }
  ds_block_sync();

  if (tid < 2 * D) {  // 16 heads x D/8 chunks of 8
    const int hd = tid / (D / 8), d0 = (tid % (D / 8)) * 8;
    const int hq = hg * DS_HEADS + hd;
    if (hq < G) {
      float mw[DS_WAVES], M = DS_NEG;
#pragma unroll
      for (int w = 0; w < DS_WAVES; ++w) {
        const float* sw = reinterpret_cast<const float*>(v_lds[w]);
        mw[w] = sw[DS_HEADS * OS + 2 * hd];
        M = __builtin_fmaxf(M, mw[w]);
      }
      float acc[8], l = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
#pragma unroll
      for (int w = 0; w < DS_WAVES; ++w) {
        const float* sw = reinterpret_cast<const float*>(v_lds[w]);
        const float f = ds_exp(mw[w] - M);
        l += f * sw[DS_HEADS * OS + 2 * hd + 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += f * sw[hd * OS + d0 + j];
      }
      const long head = (long)b * nh + kvh * G + hq;
      if (nsplit == 1) {  // the chunk is the whole prefix: l > 0
        const float inv = 1.f / l;
        bf16x8 ov;
#pragma unroll
        for (int j = 0; j < 8; ++j) ov[j] = ds_bf16bits(acc[j] * inv);
        *reinterpret_cast<bf16x8*>(ctx + head * D + d0) = ov;
      } else {
        float* wp = ws + (head * nsplit + split) * (D + 2);
        if (d0 == 0) *reinterpret_cast<f32x2*>(wp) = f32x2{M, l};
#pragma unroll
        for (int j = 0; j < 8; j += 2)
          *reinterpret_cast<f32x2*>(wp + 2 + d0 + j) =
              f32x2{acc[j], acc[j + 1]};
      }
    }
  }
}

// bf16 rows [rows, D] -> int8 rows and one fp32 scale per row.  D/16 lanes
// per row, two 16-byte loads and one 16-byte store per lane; 256 threads
// take 4096 / D rows.  Rows past the end are zeros, so the shuffles stay in
// uniform control flow.
template <int D>
__global__ __launch_bounds__(DS_THREADS)
void kv_quantize_int8_kernel(const bf16_t* __restrict__ x,
                             signed char* __restrict__ q,
                             float* __restrict__ sc, long rows) {
  constexpr int LPR = D / 16;
  const long row = (long)blockIdx.x * (DS_THREADS / LPR) + threadIdx.x / LPR;
  const int vl = threadIdx.x % LPR;
  float y[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) y[j] = 0.f;
  if (row < rows) {
    q8_bf16x8_f32(x + row * D + 16 * vl, y);
    q8_bf16x8_f32(x + row * D + 16 * vl + 8, y + 8);
  }
  float amax = q8_amax8(y + 8, q8_amax8(y, 0.f)), scale, inv;
#pragma unroll
  for (int m = 1; m < LPR; m <<= 1)
    amax = __builtin_fmaxf(amax, ds_shfl_xor(amax, m));
  q8_row_scale(amax, scale, inv);
  const i32x4 out = q8_pack16(y, inv);
  if (row < rows) {
    *reinterpret_cast<i32x4*>(q + row * D + 16 * vl) = out;
    if (vl == 0) sc[row] = scale;
  }
}

template <int D>
void q8_launch(const void* qkv, void* kq, float* ksc, void* vq, float* vsc,
               const float* cos_t, const float* sin_t, const void* pos,
               int pos_n, float* ws, void* ctx, int b, int nh, int nkv,
               int cache_len, float scale, int rope, int nsplit,
               hipStream_t s) {
  const int ngrp = (nh / nkv + DS_HEADS - 1) / DS_HEADS;
  const dim3 grid(nsplit, nkv * ngrp, b);
  if (rope)
    hipLaunchKernelGGL((decode_split_q8_kernel<D, true>), grid,
                       dim3(DS_THREADS), 0, s, (const bf16_t*)qkv,
                       (signed char*)kq, ksc, (signed char*)vq, vsc, cos_t,
                       sin_t, (const long*)pos, pos_n, ws, (bf16_t*)ctx, nh,
                       nkv, cache_len, scale);
  else
    hipLaunchKernelGGL((decode_split_q8_kernel<D, false>), grid,
                       dim3(DS_THREADS), 0, s, (const bf16_t*)qkv,
                       (signed char*)kq, ksc, (signed char*)vq, vsc, cos_t,
                       sin_t, (const long*)pos, pos_n, ws, (bf16_t*)ctx, nh,
                       nkv, cache_len, scale);
  if (nsplit > 1) fs_decode_combine(ws, ctx, b, nh, D, nsplit, s);
}

}  // namespace

// d is 64 or 128 and cache_len a multiple of 4; ws is only touched when
// nsplit > 1.  All shape checks are the binding's.
extern "C" void fs_decode_attn_split_q8(
    const void* qkv, void* kq, float* ksc, void* vq, float* vsc,
    const float* cos_t, const float* sin_t, const void* pos, int pos_n,
    float* ws, void* ctx, int b, int nh, int nkv, int d, int cache_len,
    float scale, int rope, int nsplit, hipStream_t s) {
  if (d == 64)
    q8_launch<64>(qkv, kq, ksc, vq, vsc, cos_t, sin_t, pos, pos_n, ws, ctx, b,
                  nh, nkv, cache_len, scale, rope, nsplit, s);
  else
    q8_launch<128>(qkv, kq, ksc, vq, vsc, cos_t, sin_t, pos, pos_n, ws, ctx,
                   b, nh, nkv, cache_len, scale, rope, nsplit, s);
}

// x bf16 [rows, d] -> q int8 [rows, d], sc fp32 [rows]; d is 64 or 128.
extern "C" void fs_kv_quantize_int8(const void* x, void* q, float* sc,
                                    long rows, int d, hipStream_t s) {
  if (rows == 0) return;
  if (d == 64) {
    const dim3 grid((unsigned)((rows + 63) / 64));
    hipLaunchKernelGGL((kv_quantize_int8_kernel<64>), grid, dim3(DS_THREADS),
                       0, s, (const bf16_t*)x, (signed char*)q, sc, rows);
  } else {
    const dim3 grid((unsigned)((rows + 31) / 32));
    hipLaunchKernelGGL((kv_quantize_int8_kernel<128>), grid, dim3(DS_THREADS),
                       0, s, (const bf16_t*)x, (signed char*)q, sc, rows);
  }
}

#pragma clang attribute pop
