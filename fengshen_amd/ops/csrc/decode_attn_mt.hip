// Multi-token split-KV grouped decode attention for MI355X (gfx950), bf16.
//
// A verify step of speculative / lookahead decoding: T new tokens per
// sequence attend to the static cache and, causally, to each other, in one
// launch per layer.  decode_split_kernel (decode_attn.hip) with the idle MFMA
// columns filled: its N dimension is 16 query heads of one KV head, of which
// a model with G = nh / nkv heads per KV head uses G.  Here the 16 columns
// are (token, head) pairs, so T tokens read the key prefix once.
//   qkv     [b, T, (nh + 2*nkv)*D]  [q | k | v] of the T tokens of this step;
//                                   token t of sequence b sits at pos_b + t
//   kc/vc   [b, nkv, L, D]          static caches, rows pos_b .. pos_b+T-1
//                                   written here
//   cos/sin [>= L, D] fp32          rope tables
//   pos     int64 [b] or [1]        per-sequence position (device memory),
//                                   clamped into [0, L - T] where it is read
//   ws      [b, T, nh, nsplit, D+2] fp32 partials (m, l, O[D]), nsplit > 1
//   ctx     [b, T, nh*D]
// Grid (nsplit, nkv * ceil(T*G/16), b) x 256 threads.  Column c in [0, T*G)
// of a KV head is token c / G, head c % G of the group; a block owns 16
// consecutive columns (absent ones are zero) and one chunk of the key range
// [0, pos_b + T).  The chunk is ceil((pos_b + T) / nsplit) rounded up to 64,
// computed from pos_b in the kernel: the grid depends on shapes only and a
// captured graph stays valid as pos moves.  With T*G > 16 the column groups
// of a KV head each stream its K/V; all but the first read come from L2, as
// for G > 16 in decode_split_kernel.
//
// What differs from decode_split_kernel:
//   B operand   the query of column c, roped at pos_b + t(c) in fp32, scaled,
//               rounded to bf16; built once per wave.
//   mask        column c sees keys <= pos_b + t(c): the bound is a per-lane
//               scalar next to m and l, and both the score and p are selected
//               on the integer key index.  A tile can hold keys of which a
//               column sees none (keys above pos_b for the column of token
//               0).  Then its m stays DS_NEG, alpha is exp(0) = 1, every p is
//               the select's exact 0, and l and O do not move.  A wave or a
//               split that never sees a key of a column leaves (DS_NEG, 0, 0)
//               for it, which the merges weigh with exp(DS_NEG - M) = 0.
//               Key 0 is visible to every column, so the total l is > 0.
//   new rows    cache loads stay predicated on key < pos_b; rows pos_b ..
//               pos_b+T-1 of K (roped at their own position, rounded to bf16)
//               and V come from qkv.  They may straddle two tiles, two waves
//               and two splits; the patch branch is wave-uniform.  Each of the
//               T cache rows has one writer: column group 0 of the split
//               whose chunk holds that row.  Rows >= pos_b + T are neither
//               read nor written.
// The rest is the sibling's: four waves take the chunk's 64-key tiles
// round-robin with no block barrier in the key loop, K A-fragments come
// straight from global memory, the wave-private V image is read with
// ds_read_b64_tr_b16, the next tile is prefetched before the MFMAs, one LDS
// merge in wave order, no atomics: the same inputs give the same bits.

#include "common.h"

// Packed fp32 VALU forms are kept out of this file's code.
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)

#include "decode_split.h"  // types, tile constants, V image layout, helpers

// decode_combine_kernel of decode_attn.hip on partials [b, nh, nsplit, d + 2]
extern "C" void fs_decode_combine(const float* ws, void* ctx, int b, int nh,
                                  int d, int nsplit, hipStream_t s);

namespace {

// Elements d0..d0+7 of a head row of qkv, roped with the table rows cs/sn in
// fp32 (rotate-half convention of decode_attn_kernel), times scale, as bf16.
template <int D, bool ROPE>
__device__ __forceinline__ bf16x8 mt_rope8(const bf16_t* __restrict__ row,
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
    const f32x4 c0 = *reinterpret_cast<const f32x4*>(cs + d0);
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(cs + d0 + 4);
    const f32x4 s0 = *reinterpret_cast<const f32x4*>(sn + d0);
    const f32x4 s1 = *reinterpret_cast<const f32x4*>(sn + d0 + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float y = ds_bf16_f32(yr[j]);
      const float cj = j < 4 ? c0[j & 3] : c1[j & 3];
      const float sj = j < 4 ? s0[j & 3] : s1[j & 3];
      x[j] = x[j] * cj + (lo ? -y : y) * sj;
    }
  }
  bf16x8 out;
#pragma unroll
  for (int j = 0; j < 8; ++j) out[j] = ds_bf16bits(x[j] * scale);
  return out;
}

template <int D, bool ROPE>
__global__ __launch_bounds__(DS_THREADS)
void decode_split_mt_kernel(const bf16_t* __restrict__ qkv,
                            bf16_t* __restrict__ kc, bf16_t* __restrict__ vc,
                            const float* __restrict__ cos_t,
                            const float* __restrict__ sin_t,
                            const long* __restrict__ pos_p, int pos_n,
                            float* __restrict__ ws, bf16_t* __restrict__ ctx,
                            int T, int nh, int nkv, int cache_len,
                            float scale) {
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
  const int ncol = T * G;
  const int ngrp = (ncol + DS_HEADS - 1) / DS_HEADS;
  const int kvh = blockIdx.y / ngrp, cg = blockIdx.y % ngrp;
  const int b = blockIdx.z;

  // clamped where it is read: a bad value changes keys, never an address
  long praw = pos_p[pos_n == 1 ? 0 : b];
  praw = praw < 0 ? 0 : (praw > cache_len - T ? cache_len - T : praw);
  const int pos = __builtin_amdgcn_readfirstlane((int)praw);

  const long W = (long)(nh + 2 * nkv) * D;
  const bf16_t* qtok = qkv + (long)b * T * W;               // token 0's row
  const bf16_t* knew = qtok + (long)nh * D + kvh * D;       // + t * W
  const bf16_t* vnew = knew + (long)nkv * D;                // + t * W
  const float* cs = cos_t + (long)pos * D;                  // + t * D
  const float* sn = sin_t + (long)pos * D;
  const long coff = ((long)b * nkv + kvh) * (long)cache_len * D;
  const bf16_t* kbase = kc + coff;
  const bf16_t* vbase = vc + coff;

  // this split's chunk of [0, pos + T): equal parts rounded up to whole tiles
  const int nkeys = pos + T;
  const int clen = ((nkeys + nsplit - 1) / nsplit + DS_TILE - 1) & ~(DS_TILE - 1);
  const int start = split * clen;
  const int end = start + clen < nkeys ? start + clen : nkeys;

  // the one writer of cache row pos + tk for this (b, KV head): T rows of
  // D / 8 chunks are at most 256 threads' worth
  if (cg == 0) {
    const int tk = tid / (D / 8), d0 = 8 * (tid % (D / 8));
    const int row = pos + tk;
    if (tk < T && row >= start && row < end) {
      const long roff = coff + (long)row * D + d0;
      *reinterpret_cast<bf16x8*>(kc + roff) = mt_rope8<D, ROPE>(
          knew + tk * W, d0, cs + tk * D, sn + tk * D, 1.f);
      *reinterpret_cast<bf16x8*>(vc + roff) =
          *reinterpret_cast<const bf16x8*>(vnew + tk * W + d0);
    }
  }

  // column hh of this group: token tq, head hq of the KV head's group.  kb is
  // the last key the column sees; absent columns are zero queries and their
  // results are dropped in the merge
  const int col = cg * DS_HEADS + hh;
  int tq = col / G;
  const int hq = col - tq * G;
  tq = tq < T ? tq : T - 1;
  const int kb = pos + tq;

  // B operand of St: column hh, d = 32c + 8g + j
  bf16x8 bq[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    bq[c] = ds_zero8();
    if (col < ncol)
      bq[c] = mt_rope8<D, ROPE>(qtok + tq * W + (long)(kvh * G + hq) * D,
                                32 * c + 8 * g, cs + tq * D, sn + tq * D,
                                scale);
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
  float m_run = DS_NEG, l_run = 0.f;  // of column hh; l is this lane's share

  bf16x8 kr[4][NC], vr[CH];
  int k0 = start + DS_TILE * wave;
  load_tile(k0, k0 < end ? pos : 0, kr, vr);
  for (; k0 < end; k0 += DS_TILE * DS_WAVES) {
    // rows pos .. pos+T-1 of K and V come from qkv (wave-uniform branch)
    if (k0 < pos + T && k0 + DS_TILE > pos) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int tk = k0 + 16 * t + hh - pos;
        if (tk >= 0 && tk < T) {
#pragma unroll
          for (int c = 0; c < NC; ++c)
            kr[t][c] = mt_rope8<D, ROPE>(knew + tk * W, 32 * c + 8 * g,
                                         cs + tk * D, sn + tk * D, 1.f);
        }
      }
#pragma unroll
      for (int it = 0; it < CH; ++it) {
        const int tk = k0 + it * RPI + vrow - pos;
        if (tk >= 0 && tk < T && vch < D / 8)
          vr[it] = *reinterpret_cast<const bf16x8*>(vnew + tk * W + 8 * vch);
      }
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
    // s[t][r] = score of key k0 + 16t + 4g + r for column hh
    float tmax = DS_NEG;
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kidx = k0 + 16 * t + 4 * g + r;
        s[t][r] = kidx <= kb ? s[t][r] : DS_NEG;
        tmax = __builtin_fmaxf(tmax, s[t][r]);
      }
    tmax = __builtin_fmaxf(tmax, ds_shfl_xor(tmax, 16));
    tmax = __builtin_fmaxf(tmax, ds_shfl_xor(tmax, 32));
    // a column that sees no key of this tile: m_new = m_run, alpha = 1
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
        const float p = kidx <= kb ? ds_exp(s[t][r] - m_new) : 0.f;
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

  if (tid < 2 * D) {  // 16 columns x D/8 chunks of 8
    const int hd = tid / (D / 8), d0 = (tid % (D / 8)) * 8;
    const int oc = cg * DS_HEADS + hd;
    if (oc < ncol) {
      // a wave that saw no key of the column holds (DS_NEG, 0, 0): weight
      // exp(DS_NEG - M) = 0, or 1 on zeros when no wave saw one
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
      const int ot = oc / G;
      const long head = ((long)b * T + ot) * nh + kvh * G + (oc - ot * G);
      if (nsplit == 1) {  // the chunk holds key 0, which every column sees
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

template <int D>
void mt_launch(const void* qkv, void* kc, void* vc, const float* cos_t,
               const float* sin_t, const void* pos, int pos_n, float* ws,
               void* ctx, int b, int T, int nh, int nkv, int cache_len,
               float scale, int rope, int nsplit, hipStream_t s) {
  const int ngrp = (T * (nh / nkv) + DS_HEADS - 1) / DS_HEADS;
  const dim3 grid(nsplit, nkv * ngrp, b);
  if (rope)
    hipLaunchKernelGGL((decode_split_mt_kernel<D, true>), grid,
                       dim3(DS_THREADS), 0, s, (const bf16_t*)qkv,
                       (bf16_t*)kc, (bf16_t*)vc, cos_t, sin_t,
                       (const long*)pos, pos_n, ws, (bf16_t*)ctx, T, nh, nkv,
                       cache_len, scale);
  else
    hipLaunchKernelGGL((decode_split_mt_kernel<D, false>), grid,
                       dim3(DS_THREADS), 0, s, (const bf16_t*)qkv,
                       (bf16_t*)kc, (bf16_t*)vc, cos_t, sin_t,
                       (const long*)pos, pos_n, ws, (bf16_t*)ctx, T, nh, nkv,
                       cache_len, scale);
  // partials [b, T, nh, nsplit, D + 2]: the tokens are the combine's batch
  if (nsplit > 1) fs_decode_combine(ws, ctx, b * T, nh, D, nsplit, s);
}

}  // namespace

// tokens in [2, 16], cache_len >= tokens; ws is only touched when nsplit > 1.
// All shape checks are the binding's.
extern "C" void fs_decode_attn_split_mt(const void* qkv, void* kc, void* vc,
                                        const float* cos_t,
                                        const float* sin_t, const void* pos,
                                        int pos_n, float* ws, void* ctx,
                                        int b, int tokens, int nh, int nkv,
                                        int d, int cache_len, float scale,
                                        int rope, int nsplit, hipStream_t s) {
  if (d == 64)
    mt_launch<64>(qkv, kc, vc, cos_t, sin_t, pos, pos_n, ws, ctx, b, tokens,
                  nh, nkv, cache_len, scale, rope, nsplit, s);
  else if (d == 96)
    mt_launch<96>(qkv, kc, vc, cos_t, sin_t, pos, pos_n, ws, ctx, b, tokens,
                  nh, nkv, cache_len, scale, rope, nsplit, s);
  else
    mt_launch<128>(qkv, kc, vc, cos_t, sin_t, pos, pos_n, ws, ctx, b, tokens,
                   nh, nkv, cache_len, scale, rope, nsplit, s);
}

#pragma clang attribute pop
