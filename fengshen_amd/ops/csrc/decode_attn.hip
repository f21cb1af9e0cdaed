// Split-KV grouped decode attention for MI355X (gfx950), bf16.
//
// One launch per layer inside the captured decode graph, like
// decode_attn_kernel (kernels.hip), with a different work split:
//   qkv     [b, (nh + 2*nkv)*D]  [q | k | v] of this step
//   kc/vc   [b, nkv, L, D]       static caches, row pos_b written here
//   cos/sin [>= L, D] fp32       rope tables
//   pos     int64 [b] or [1]     per-sequence position (device memory)
//   ws      [b, nh, nsplit, D+2] fp32 partials (m, l, O[D]), nsplit > 1 only
//   ctx     [b, nh*D]
// Grid (nsplit, nkv * ceil(G/16), b) x 256 threads, G = nh / nkv.  A block
// owns up to 16 query heads of one KV head and one chunk of the key prefix
// [0, pos_b]; the chunk bounds come from pos_b inside the kernel, so the
// grid depends on shapes only and a captured graph stays valid as pos moves.
// The four waves take the chunk's 64-key tiles round-robin, each with its own
// (m, l, O); there is no block barrier in the key loop, the wave states are
// merged once at the end through LDS in wave order.
//
// Per tile and wave:
//   St[key, head] = K . Qt   mfma 16x16x32, A = 16 keys x 32 d: one 16-byte
//       global load per lane (row = l%16, k = (l/16)*8 + j), no LDS.  B = the
//       group's roped, scaled queries, built once per wave.
//   the accumulator holds 4 keys of head l%16 per 16-key tile: row max and
//       sum are in-lane plus two shuffles (16, 32); m, l and the rescale
//       factor are per-lane scalars.
//   Ot[d, head] = Vt . Pt    B = P packed straight from the two St
//       accumulators of a 32-key pair (k slot 8g + j <-> key 4g + j of the
//       first half, 4g + j - 4 of the second).  A = Vt in the same order,
//       read with ds_read_b64_tr_b16 from a wave-private row-major image of
//       the V tile (16-byte stores, chunk XOR below).
// Rows >= pos_b of the caches are never read: their loads are predicated off
// on the integer key index and give zeros, and row pos_b of K and V comes
// from qkv.  Scores are masked by select, so whatever bits those rows hold
// cannot reach the result.  Exactly one block per (b, KV head) writes row
// pos_b of both caches: head group 0 of the split whose chunk holds pos_b.

#include "common.h"

// Packed fp32 VALU forms are kept out of this file's code.
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

#include "decode_split.h"  // types, tile constants, V image layout, helpers

namespace {

// Elements d0..d0+7 of a head row of qkv, roped at this position in fp32
// (rotate-half convention of decode_attn_kernel), times scale, as bf16.
template <int D, bool ROPE>
__device__ __forceinline__ bf16x8 ds_rope8(const bf16_t* __restrict__ row,
                                           int d0,
                                           const float* __restrict__ cs,
                                           const float* __restrict__ sn,
                                           float scale) {
  const bf16x8 xr = *reinterpret_cast<const bf16x8*>(row + d0);
  float x[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = ds_bf16_f32(xr[j]);
  if (ROPE) {
    const bool lo = d0 < D / 2;
    const bf16x8 yr = *reinterpret_cast<const bf16x8*>(
        row + (lo ? d0 + D / 2 : d0 - D / 2));
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = ds_bf16_f32(yr[j]);
      x[j] = x[j] * cs[d0 + j] + (lo ? -y : y) * sn[d0 + j];
    }
  }
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = ds_bf16bits(x[j] * scale);
  return out;
}

template <int D, bool ROPE>
__global__ __launch_bounds__(DS_THREADS)
void decode_split_kernel(const bf16_t* __restrict__ qkv,
                         bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                         const float* __restrict__ cos_t,
                         const float* __restrict__ sin_t,
                         const long* __restrict__ pos_p, int pos_n,
                         float* __restrict__ ws, bf16_t* __restrict__ ctx,
                         int nh, int nkv, int cache_len, float scale) {
  constexpr int NC = D / 32;         // k steps of St
  constexpr int NDT = D / 16;        // 16-row tiles of Ot
  constexpr int RB = ds_rowb(D);
  constexpr int CH = RB / 16;        // 16-byte chunks per image row
  constexpr int RPI = DS_TILE / CH;  // rows staged per store instruction
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
  const long coff = ((long)b * nkv + kvh) * (long)cache_len * D;
  const bf16_t* kbase = kc + coff;
  const bf16_t* vbase = vc + coff;

  // this split's chunk of [0, pos]: equal parts rounded up to whole tiles
  const int nkeys = pos + 1;
  const int clen = ((nkeys + nsplit - 1) / nsplit + DS_TILE - 1) & ~(DS_TILE - 1);
  const int start = split * clen;
  const int end = start + clen < nkeys ? start + clen : nkeys;

  // the one writer of cache row pos for this (b, KV head)
  if (hg == 0 && pos >= start && pos < end && tid < D / 8) {
    const long roff = coff + (long)pos * D + 8 * tid;
    *reinterpret_cast<bf16x8*>(kc + roff) =
        ds_rope8<D, ROPE>(knew, 8 * tid, cs, sn, 1.f);
    *reinterpret_cast<bf16x8*>(vc + roff) =
        *reinterpret_cast<const bf16x8*>(vnew + 8 * tid);
  }

  // B operand of St: head hh of this group, d = 32c + 8g + j; absent heads 0
  bf16x8 bq[NC];
  {
    const int hq = hg * DS_HEADS + hh;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bq[c] = ds_zero8();
      if (hq < G)
        bq[c] = ds_rope8<D, ROPE>(qrow + (long)(kvh * G + hq) * D,
                                  32 * c + 8 * g, cs, sn, scale);
    }
  }

  const int vrow = lane / CH, vch = lane % CH;
  // K (A fragments, tile t = keys 16t + hh) and V (image chunks) of the tile
  // at k0; only keys < lim are read, the rest are zeros
  auto load_tile = [&](int k0, int lim, bf16x8 (&kf)[4][NC],
                       bf16x8 (&vf)[CH]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int key = k0 + 16 * t + hh;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        kf[t][c] = ds_zero8();
        if (key < lim)
          kf[t][c] = *reinterpret_cast<const bf16x8*>(
              kbase + (long)key * D + 32 * c + 8 * g);
      }
    }
#pragma unroll
    for (int it = 0; it < CH; ++it) {
      const int key = k0 + it * RPI + vrow;
      vf[it] = ds_zero8();
      if (key < lim && vch < D / 8)
        vf[it] = *reinterpret_cast<const bf16x8*>(
            vbase + (long)key * D + 8 * vch);
    }
  };

  char* vt = v_lds[wave];
  // transposed read: lane i of a group addresses row i>>2, columns 4(i&3)
  const int trow = 4 * g + (hh >> 2);
  const int tch = (hh & 3) >> 1, tbyte = 8 * (hh & 1);

  f32x4 o[NDT];
#pragma unroll
  for (int dt = 0; dt < NDT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = DS_NEG, l_run = 0.f;  // of head hh; l is this lane's share

  bf16x8 kr[4][NC], vr[CH];
  int k0 = start + DS_TILE * wave;
  load_tile(k0, k0 < end ? pos : 0, kr, vr);
  for (; k0 < end; k0 += DS_TILE * DS_WAVES) {
    // row pos of K and V comes from qkv (wave-uniform branch)
    if (pos >= k0 && pos < k0 + DS_TILE) {
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (k0 + 16 * t + hh == pos) {
#pragma unroll
          for (int c = 0; c < NC; ++c)
            kr[t][c] = ds_rope8<D, ROPE>(knew, 32 * c + 8 * g, cs, sn, 1.f);
        }
#pragma unroll
      for (int it = 0; it < CH; ++it)
        if (k0 + it * RPI + vrow == pos && vch < D / 8)
          vr[it] = *reinterpret_cast<const bf16x8*>(vnew + 8 * vch);
    }
#pragma unroll
    for (int it = 0; it < CH; ++it)
      *reinterpret_cast<bf16x8*>(vt + ds_voff<RB>(it * RPI + vrow, vch)) =
          vr[it];

    // next tile's loads go out before this tile's MFMAs
    bf16x8 kn[4][NC], vn[CH];
    const int k1 = k0 + DS_TILE * DS_WAVES;
    load_tile(k1, k1 < end ? pos : 0, kn, vn);

    f32x4 s[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      s[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < NC; ++c)
        s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kr[t][c], bq[c], s[t],
                                                       0, 0, 0);
    }
    // s[t][r] = score of key k0 + 16t + 4g + r for head hh
    float tmax = DS_NEG;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kidx = k0 + 16 * t + 4 * g + r;
        s[t][r] = kidx <= pos ? s[t][r] : DS_NEG;
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
        psum += p;
        pb[t >> 1][4 * (t & 1) + r] = ds_bf16bits(p);
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
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int c = 0; c < NC; ++c) kr[t][c] = kn[t][c];
#pragma unroll
    for (int it = 0; it < CH; ++it) vr[it] = vn[it];
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

// Merge the nsplit partials of one (b, head) in split order; grid (nh, b),
// 64 threads, thread t owns d = 2t, 2t + 1.
template <int D>
__global__ __launch_bounds__(64)
void decode_combine_kernel(const float* __restrict__ ws,
                           bf16_t* __restrict__ ctx, int nh, int nsplit) {
  const int t = threadIdx.x;
  const long head = (long)blockIdx.y * nh + blockIdx.x;
  const float* wp = ws + head * nsplit * (D + 2);
  float M = DS_NEG;
  for (int i = 0; i < nsplit; ++i) M = __builtin_fmaxf(M, wp[i * (D + 2)]);
  if (2 * t >= D) return;
  float l = 0.f, a0 = 0.f, a1 = 0.f;
  for (int i = 0; i < nsplit; ++i) {
    const float* p = wp + i * (D + 2);
    const float f = ds_exp(p[0] - M);
    const f32x2 v = *reinterpret_cast<const f32x2*>(p + 2 + 2 * t);
    l += f * p[1];
    a0 += f * v[0];
    a1 += f * v[1];
  }
  const float inv = 1.f / l;
  const unsigned int lo = (unsigned short)ds_bf16bits(a0 * inv);
  const unsigned int hi = (unsigned short)ds_bf16bits(a1 * inv);
  *reinterpret_cast<unsigned int*>(ctx + head * D + 2 * t) = lo | (hi << 16);
}

template <int D>
void ds_launch(const void* qkv, void* kc, void* vc, const float* cos_t,
               const float* sin_t, const void* pos, int pos_n, float* ws,
               void* ctx, int b, int nh, int nkv, int cache_len, float scale,
               int rope, int nsplit, hipStream_t s) {
  const int ngrp = (nh / nkv + DS_HEADS - 1) / DS_HEADS;
  const dim3 grid(nsplit, nkv * ngrp, b);
  if (rope)
    hipLaunchKernelGGL((decode_split_kernel<D, true>), grid, dim3(DS_THREADS),
                       0, s, (const bf16_t*)qkv, (bf16_t*)kc, (bf16_t*)vc,
                       cos_t, sin_t, (const long*)pos, pos_n, ws,
                       (bf16_t*)ctx, nh, nkv, cache_len, scale);
  else
    hipLaunchKernelGGL((decode_split_kernel<D, false>), grid,
                       dim3(DS_THREADS), 0, s, (const bf16_t*)qkv,
                       (bf16_t*)kc, (bf16_t*)vc, cos_t, sin_t,
                       (const long*)pos, pos_n, ws, (bf16_t*)ctx, nh, nkv,
                       cache_len, scale);
  if (nsplit > 1)
    hipLaunchKernelGGL((decode_combine_kernel<D>), dim3(nh, b), dim3(64), 0,
                       s, (const float*)ws, (bf16_t*)ctx, nh, nsplit);
}

}  // namespace

// ws is only touched when nsplit > 1.  All shape checks are the binding's.
extern "C" void fs_decode_attn_split(const void* qkv, void* kc, void* vc,
                                     const float* cos_t, const float* sin_t,
                                     const void* pos, int pos_n, float* ws,
                                     void* ctx, int b, int nh, int nkv, int d,
                                     int cache_len, float scale, int rope,
                                     int nsplit, hipStream_t s) {
  if (d == 64)
    ds_launch<64>(qkv, kc, vc, cos_t, sin_t, pos, pos_n, ws, ctx, b, nh, nkv,
                  cache_len, scale, rope, nsplit, s);
  else if (d == 96)
    ds_launch<96>(qkv, kc, vc, cos_t, sin_t, pos, pos_n, ws, ctx, b, nh, nkv,
                  cache_len, scale, rope, nsplit, s);
  else
    ds_launch<128>(qkv, kc, vc, cos_t, sin_t, pos, pos_n, ws, ctx, b, nh, nkv,
                   cache_len, scale, rope, nsplit, s);
}

// decode_combine_kernel on partials [b, nh, nsplit, d + 2] written by another
// file's split kernel (decode_attn_q8.hip); d is 64, 96 or 128.
extern "C" void fs_decode_combine(const float* ws, void* ctx, int b, int nh,
                                  int d, int nsplit, hipStream_t s) {
  const dim3 grid(nh, b), block(64);
  if (d == 64)
    hipLaunchKernelGGL((decode_combine_kernel<64>), grid, block, 0, s, ws,
                       (bf16_t*)ctx, nh, nsplit);
  else if (d == 96)
    hipLaunchKernelGGL((decode_combine_kernel<96>), grid, block, 0, s, ws,
                       (bf16_t*)ctx, nh, nsplit);
  else
    hipLaunchKernelGGL((decode_combine_kernel<128>), grid, block, 0, s, ws,
                       (bf16_t*)ctx, nh, nsplit);
}

#pragma clang attribute pop
