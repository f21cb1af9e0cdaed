// Flash-style fused attention (fwd + FA2-style bwd) for MI355X (gfx950).
//
// Replaces the reference's flash_attn_cuda import (flash_attention.py:7) with
// a native CDNA4 kernel family: per Q-tile, stream K/V tiles through LDS,
// QK^T and PV on MFMA (v_mfma_f32_16x16x32_bf16), online softmax in fp32
// registers.  No SxS materialization (removes the reference's fused-softmax
// sk<=2048 cap and the 3x HBM round trip of the bmm path).
//
// Generality (round 2): kernels are templated on <int D, bool CAUSAL>:
//   D in {40, 64, 80, 96, 128, 160}  — covers LLaMA/GPT (128/96), BERT (64),
//       SD UNet self/cross attention (40/80/160).  D is padded to DP
//       (multiple of 32) in LDS/fragments; global loads are guarded at
//       8-element granularity (D % 8 == 0), pad lanes carry zeros.
//   CAUSAL=true : dense causal self-attention (sq == sk, sq % 64 == 0) —
//       byte-identical schedule to the round-1 kernel at D=128.
//   CAUSAL=false: bidirectional, supports cross-attention (sq != sk),
//       ragged sk (any length; tail masked), and per-batch key lengths
//       (klens[b], suffix padding masks a la BERT) — key col >= klen
//       contributes nothing to softmax, P, dK, dV.
//
// Structure (guide §B "fused attention prefill"):
//   block = 8 waves; wave w owns 16 q-rows => QBLK = 128; KVBLK = 64.
//   K staged [64][DP] with XOR swizzle (guide §6 G4 / T2: row-major bf16 is
//   a wide ds_read_b128 bank conflict; byte ^= (row&7)<<4 fixes it; LDS row
//   stride is padded to a power of two so the XOR stays a bijection).
//   V staged transposed [DP][64+pad] with kv-index swizzle so PV B-fragments
//   read 16B-contiguous kv runs.  async-STAGE split (T14): next tile's
//   global loads issue during current tile's MFMA.
// Outputs: O [b,h,sq,D] and LSE [b,h,sq] (softmax log-sum-exp, for bwd).

#include "common.h"
#include "flash_blockmap.h"

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

#define FA_QBLK 128          // 8 waves x 16 q rows
#define FA_KVBLK 64
#define FA_WAVES 8
#define FA_VPAD 8
#define FB_T 32              // backward streaming tile

// padded head dim (fragment/LDS layout granularity)
constexpr int fa_dpad(int d) { return (d + 31) / 32 * 32; }
// LDS row stride in BYTES: power of two >= 2*DP so the (row&7)<<4 XOR
// swizzle is a bijection that never crosses rows
constexpr int fa_swb(int dp) {
  int need = 2 * dp, p = 128;
  while (p < need) p <<= 1;
  return p;
}

// XOR swizzle for row-major K/Q/V LDS tiles (16B-granular byte offsets)
__device__ __forceinline__ int kswz(int row, int byte_in_row) {
  return byte_in_row ^ ((row & 7) << 4);
}

// splitmix64 counter hash for attention dropout: fwd and bwd regenerate
// the SAME keep/drop decision per (bh, qrow, kcol) from (seed, index) —
// no mask tensor is ever materialized.
__device__ __forceinline__ unsigned int fa_hash(unsigned long long seed,
                                                unsigned long long idx) {
  unsigned long long z = seed + idx * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (unsigned int)(z >> 32);
}

__device__ __forceinline__ short fa_bf16bits(float f) {
  return (short)__hip_bfloat16_raw(__float2bfloat16(f)).x;
}

// guarded 8-elem global load: zero vector beyond D (D % 8 == 0)
template <int D>
__device__ __forceinline__ bf16x8 fa_load8(const bf16_t* rowp, int d0) {
  if (d0 < D) return *reinterpret_cast<const bf16x8*>(rowp + d0);
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = 0;
  return z;
}

// ===========================================================================
// FORWARD
// ===========================================================================
template <int D, bool CAUSAL>
__global__ __launch_bounds__(FA_WAVES * 64)
void flash_attn_fwd_kernel(const bf16_t* __restrict__ Q,
                           const bf16_t* __restrict__ K,
                           const bf16_t* __restrict__ V,
                           bf16_t* __restrict__ O,
                           float* __restrict__ LSE,
                           const int* __restrict__ klens,
                           int b, int h, int sq, int sk, float scale,
                           unsigned int drop_thresh, float keep_scale,
                           unsigned long long drop_seed) {
  constexpr int DP = fa_dpad(D);
  constexpr int NC = DP / 32;    // MFMA K-chunks
  constexpr int NTO = DP / 16;   // output d-tiles
  constexpr int SWB = fa_swb(DP);

  __shared__ char k_raw[FA_KVBLK * SWB];               // swizzled K rows
  __shared__ short vt_lds[DP][FA_KVBLK + FA_VPAD];     // V transposed
  __shared__ short p_lds[FA_WAVES][16][FA_KVBLK + FA_VPAD];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int qb = blockIdx.x;
  const int head = blockIdx.y;
  const int batch = blockIdx.z;

  const bf16_t* Qp = Q + ((long)batch * h + head) * sq * D;
  const bf16_t* Kp = K + ((long)batch * h + head) * sk * D;
  const bf16_t* Vp = V + ((long)batch * h + head) * sk * D;
  bf16_t* Op = O + ((long)batch * h + head) * sq * D;

  const int klen = CAUSAL ? sk
                          : min(klens ? klens[batch] : sk, sk);

  const int q0 = qb * FA_QBLK + wave * 16;
  // partial blocks: OOB waves compute on clamped rows (must still hit every
  // __syncthreads) and skip their stores
  const bool q_active = q0 < sq;
  const int q0c = q_active ? q0 : (sq > 16 ? sq - 16 : 0);

  // ---- Q tile -> A-fragments (layout LA0: row=l%16, k=(l/16)*8+j;
  // verified on HW by scripts/mfma_probe), pre-scaled -----------------------
  bf16x8 q_frag[NC];
  {
    const int row = lane & 15;
    const int k0 = (lane >> 4) * 8;
    const int qrow = min(q0c + row, sq - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8 raw = fa_load8<D>(Qp + (long)qrow * D, c * 32 + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned short u = (unsigned short)raw[j];
        float f = __uint_as_float(((unsigned int)u) << 16) * scale;
        raw[j] = fa_bf16bits(f);
      }
      q_frag[c] = raw;
    }
  }

  float m_run[4], l_run[4];
  f32x4 o_acc[NTO];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = -INFINITY;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < NTO; ++t) o_acc[t] = f32x4{0, 0, 0, 0};

  int n_kv_tiles;
  if (CAUSAL) {
    const int q_hi = min(qb * FA_QBLK + FA_QBLK, sq) - 1;
    n_kv_tiles = (q_hi / FA_KVBLK) + 1;
  } else {
    n_kv_tiles = (klen + FA_KVBLK - 1) / FA_KVBLK;
    if (n_kv_tiles < 1) n_kv_tiles = 1;  // empty rows still write O=0
  }

  // async-STAGE split (guide T14): global loads for tile t+1 are issued
  // DURING tile t's compute (registers k_reg/v_reg); only the cheap LDS
  // writes sit between the barriers — HBM latency hides under MFMA.
  const int tid = threadIdx.x;
  constexpr int ELEMS = FA_KVBLK * DP;          // elements per tile
  constexpr int SWEEPS = (ELEMS + FA_WAVES * 64 * 8 - 1) / (FA_WAVES * 64 * 8);
  bf16x8 k_reg[SWEEPS], v_reg[SWEEPS];
#pragma unroll
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
    if (i < ELEMS) {
      const int kr = i / DP;
      const int kc = i % DP;
      const long krg = min(kr, sk - 1);
      k_reg[sweep] = fa_load8<D>(Kp + krg * D, kc);
      v_reg[sweep] = fa_load8<D>(Vp + krg * D, kc);
    }
  }

  for (int kt = 0; kt < n_kv_tiles; ++kt) {
    const int k_base = kt * FA_KVBLK;
    __syncthreads();
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
      const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
      if (i < ELEMS) {
        const int kr = i / DP;
        const int kc = i % DP;
        *reinterpret_cast<bf16x8*>(k_raw + kr * SWB + kswz(kr, kc * 2)) =
            k_reg[sweep];
        bf16x8 vv = v_reg[sweep];
        // kv index XOR-swizzled by d bits 3-5 (the transpose scatter would
        // otherwise put 16 lanes of one K-row into ONE bank)
#pragma unroll
        for (int j = 0; j < 8; ++j)
          vt_lds[kc + j][kr ^ ((kc + j) & 0x38)] = vv[j];
      }
    }
    __syncthreads();
    if (kt + 1 < n_kv_tiles) {
      const int nb = (kt + 1) * FA_KVBLK;
#pragma unroll
      for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
        if (i < ELEMS) {
          const int kr = i / DP;
          const int kc = i % DP;
          const long krg = min(nb + kr, sk - 1);
          k_reg[sweep] = fa_load8<D>(Kp + krg * D, kc);
          v_reg[sweep] = fa_load8<D>(Vp + krg * D, kc);
        }
      }
    }

    // ---- S = (sQ) @ K^T : four 16x16 n-tiles ------------------------------
    f32x4 s_acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) s_acc[nt] = f32x4{0, 0, 0, 0};
    {
      const int col = lane & 15;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int krow = nt * 16 + col;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int d0 = c * 32 + (lane >> 4) * 8;
          bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
              k_raw + krow * SWB + kswz(krow, d0 * 2));
          s_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              q_frag[c], bfrag, s_acc[nt], 0, 0, 0);
        }
      }
    }

    // ---- mask + online softmax -------------------------------------------
    const int col = lane & 15;
    float p[4][4];
    float tile_max[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0c + (lane >> 4) * 4 + r;
      float tm = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int kcol = k_base + nt * 16 + col;
        float v = s_acc[nt][r];
        if (CAUSAL ? (kcol > qrow) : (kcol >= klen)) v = -INFINITY;
        p[nt][r] = v;
        tm = fmaxf(tm, v);
      }
      tile_max[r] = tm;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        tile_max[r] = fmaxf(tile_max[r], __shfl_xor(tile_max[r], off, 64));
    }
    float alpha[4], rowsum[4];
    bool need_rescale = false;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float m_new = fmaxf(m_run[r], tile_max[r]);
      alpha[r] = (m_run[r] == -INFINITY) ? 0.f : __expf(m_run[r] - m_new);
      if (m_new != m_run[r]) need_rescale = true;
      m_run[r] = m_new;
      float ps = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        float e = (p[nt][r] == -INFINITY) ? 0.f : __expf(p[nt][r] - m_new);
        p[nt][r] = e;
        ps += e;
      }
      rowsum[r] = ps;
    }
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        rowsum[r] += __shfl_xor(rowsum[r], off, 64);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
      l_run[r] = l_run[r] * alpha[r] + rowsum[r];
    // attention dropout on P (normalizer l uses the UNdropped sum, like
    // eager dropout(softmax(S))); uniform branch, free when p == 0
    if (drop_thresh) {
      const unsigned long long bh_base =
          ((unsigned long long)batch * h + head) * sq;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const unsigned long long qi =
            (bh_base + (unsigned long long)(q0c + (lane >> 4) * 4 + r)) *
            (unsigned long long)sk;
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
          const int kcol = k_base + nt * 16 + col;
          p[nt][r] = (fa_hash(drop_seed, qi + kcol) < drop_thresh)
                         ? 0.f : p[nt][r] * keep_scale;
        }
      }
    }
    // skip the O-wide rescale when no row max moved (defer-max lite, T13)
    if (__any(need_rescale)) {
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o_acc[t][r] *= alpha[r];
      }
    }

    // ---- P -> per-wave LDS, then PV ---------------------------------------
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        p_lds[wave][row][nt * 16 + col] = fa_bf16bits(p[nt][r]);
      }
    }
    __builtin_amdgcn_s_waitcnt(0);  // wave-local LDS visibility

    // A-frags over kv (two K=32 chunks), B-frags from V^T
#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      const int row = lane & 15;
      const int kv0 = kc * 32 + (lane >> 4) * 8;
      bf16x8 pa = *reinterpret_cast<const bf16x8*>(&p_lds[wave][row][kv0]);
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
        const int dcol = t * 16 + (lane & 15);
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &vt_lds[dcol][kv0 ^ (dcol & 0x38)]);
        o_acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pa, bfrag, o_acc[t],
                                                           0, 0, 0);
      }
    }
  }

  // ---- epilogue -----------------------------------------------------------
  if (!q_active) return;  // after the last barrier: safe to exit
  const int col = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + (lane >> 4) * 4 + r;
    if (qrow >= sq) continue;
    const float inv_l = (l_run[r] > 0.f) ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      const int d = t * 16 + col;
      if (d < D) Op[(long)qrow * D + d] = __float2bfloat16(o_acc[t][r] * inv_l);
    }
    if (col == 0 && LSE) {
      LSE[((long)batch * h + head) * sq + qrow] =
          m_run[r] + logf(fmaxf(l_run[r], 1e-30f));
    }
  }
}

// ===========================================================================
// BACKWARD
// ===========================================================================
// FlashAttention-2-style: delta = rowsum(dO*O); then
//   dQ kernel (q-major):   S=(sQ)K^T; P=exp(S-LSE); dP=dO V^T;
//                          dS=P*(dP-delta)*s; dQ += dS K
//   dKdV kernel (kv-major): St=(sK)Q^T; Pt=exp(St-LSE[col]); dPt=V dO^T;
//                          dV += Pt dO; dSt=Pt*(dPt-delta[col])*s; dK += dSt Q
// Same fragment layouts / swizzles as forward.  Streaming tiles are 32-wide
// (FB_T) so LDS stays small -> 3-4 blocks/CU.

template <int D>
__global__ __launch_bounds__(256)
void flash_delta_kernel(const bf16_t* __restrict__ dO,
                        const bf16_t* __restrict__ O,
                        float* __restrict__ delta, long rows) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const long row0 = (long)blockIdx.x * 4 + wid;
  const long stride = (long)gridDim.x * 4;
  for (long row = row0; row < rows; row += stride) {
    const bf16_t* dop = dO + row * D;
    const bf16_t* op = O + row * D;
    float sacc = 0.f;
    for (int i = lane * 2; i < D; i += 128) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        sacc += __bfloat162float(dop[i + j]) * __bfloat162float(op[i + j]);
    }
    sacc = wave_reduce_sum(sacc);
    if (lane == 0) delta[row] = sacc;
  }
}

// Q-major: each block owns 128 q rows (wave -> 16), streams KV in 32-tiles.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(FA_WAVES * 64)
void flash_attn_bwd_dq_kernel(const bf16_t* __restrict__ Q,
                              const bf16_t* __restrict__ K,
                              const bf16_t* __restrict__ V,
                              const bf16_t* __restrict__ dO,
                              const float* __restrict__ LSE,
                              const float* __restrict__ Delta,
                              bf16_t* __restrict__ dQ,
                              const int* __restrict__ klens,
                              int b, int h, int sq, int sk, float scale,
                              unsigned int drop_thresh, float keep_scale,
                              unsigned long long drop_seed) {
  constexpr int DP = fa_dpad(D);
  constexpr int NC = DP / 32;
  constexpr int NTO = DP / 16;
  constexpr int SWB = fa_swb(DP);

  __shared__ char k_raw[FB_T * SWB];                  // K rows, swizzled
  __shared__ char v_raw[FB_T * SWB];                  // V rows, swizzled
  __shared__ short kt_lds[DP][FB_T + FA_VPAD];        // K^T, kv-swizzled
  __shared__ short p_lds[FA_WAVES][16][FB_T + FA_VPAD];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long bh = (long)blockIdx.z * h + blockIdx.y;
  const bf16_t* Qp = Q + bh * sq * D;
  const bf16_t* Kp = K + bh * sk * D;
  const bf16_t* Vp = V + bh * sk * D;
  const bf16_t* dOp = dO + bh * sq * D;
  bf16_t* dQp = dQ + bh * sq * D;
  const float* lse = LSE + bh * sq;
  const float* dlt = Delta + bh * sq;

  const int klen = CAUSAL ? sk
                          : min(klens ? klens[blockIdx.z] : sk, sk);

  const int q0 = blockIdx.x * FA_QBLK + wave * 16;
  const bool q_active = q0 < sq;
  const int q0c = q_active ? q0 : (sq > 16 ? sq - 16 : 0);

  bf16x8 q_frag[NC], do_frag[NC];
  {
    const int row = lane & 15;
    const int k0 = (lane >> 4) * 8;
    const int qrow = min(q0c + row, sq - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8 raw = fa_load8<D>(Qp + (long)qrow * D, c * 32 + k0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned short u = (unsigned short)raw[j];
        float f = __uint_as_float(((unsigned int)u) << 16) * scale;
        raw[j] = fa_bf16bits(f);
      }
      q_frag[c] = raw;
      do_frag[c] = fa_load8<D>(dOp + (long)qrow * D, c * 32 + k0);
    }
  }
  float lse_r[4], dlt_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = min(q0c + (lane >> 4) * 4 + r, sq - 1);
    lse_r[r] = lse[qrow];
    dlt_r[r] = dlt[qrow];
  }

  f32x4 dq_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) dq_acc[t] = f32x4{0, 0, 0, 0};

  int n_kv_tiles;
  if (CAUSAL) {
    const int q_hi = min(blockIdx.x * FA_QBLK + FA_QBLK, sq) - 1;
    n_kv_tiles = (q_hi / FB_T) + 1;
  } else {
    n_kv_tiles = (klen + FB_T - 1) / FB_T;
  }

  // async-STAGE (T14, like the forward): tile t+1 K/V global loads are
  // issued DURING tile t's MFMA so HBM latency hides under compute; only
  // the LDS writes sit between the barriers.
  constexpr int BELEMS = FB_T * DP;
  constexpr int BSWEEPS = (BELEMS + FA_WAVES * 64 * 8 - 1)
                          / (FA_WAVES * 64 * 8);
  bf16x8 kst[BSWEEPS], vst[BSWEEPS];
  {
    const int tid = threadIdx.x;
    const int kt0_base = (CAUSAL ? 0 : 0) * FB_T;
#pragma unroll
    for (int sw = 0; sw < BSWEEPS; ++sw) {
      const int i = tid * 8 + sw * (FA_WAVES * 64 * 8);
      if (i < BELEMS) {
        const int kr = i / DP;
        const int kc = i % DP;
        const long krg = min(kt0_base + kr, sk - 1);
        kst[sw] = fa_load8<D>(Kp + krg * D, kc);
        vst[sw] = fa_load8<D>(Vp + krg * D, kc);
      }
    }
  }
  for (int kt = 0; kt < n_kv_tiles; ++kt) {
    __syncthreads();
    {
      const int tid = threadIdx.x;
#pragma unroll
      for (int sw = 0; sw < BSWEEPS; ++sw) {
        const int i = tid * 8 + sw * (FA_WAVES * 64 * 8);
        if (i < BELEMS) {
          const int kr = i / DP;
          const int kc = i % DP;
          bf16x8 kk = kst[sw];
          *reinterpret_cast<bf16x8*>(
              k_raw + kr * SWB + kswz(kr, kc * 2)) = kk;
          *reinterpret_cast<bf16x8*>(
              v_raw + kr * SWB + kswz(kr, kc * 2)) = vst[sw];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            kt_lds[kc + j][kr ^ ((kc + j) & 0x18)] = kk[j];
        }
      }
    }
    __syncthreads();
    const int k_base = kt * FB_T;
    if (kt + 1 < n_kv_tiles) {
      const int nb = (kt + 1) * FB_T;
      const int tid = threadIdx.x;
#pragma unroll
      for (int sw = 0; sw < BSWEEPS; ++sw) {
        const int i = tid * 8 + sw * (FA_WAVES * 64 * 8);
        if (i < BELEMS) {
          const int kr = i / DP;
          const int kc = i % DP;
          const long krg = min(nb + kr, sk - 1);
          kst[sw] = fa_load8<D>(Kp + krg * D, kc);
          vst[sw] = fa_load8<D>(Vp + krg * D, kc);
        }
      }
    }

    f32x4 s_acc[2], dp_acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      s_acc[nt] = f32x4{0, 0, 0, 0};
      dp_acc[nt] = f32x4{0, 0, 0, 0};
    }
    {
      const int col = lane & 15;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int krow = nt * 16 + col;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int d0 = c * 32 + (lane >> 4) * 8;
          bf16x8 kb = *reinterpret_cast<const bf16x8*>(
              k_raw + krow * SWB + kswz(krow, d0 * 2));
          s_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              q_frag[c], kb, s_acc[nt], 0, 0, 0);
          bf16x8 vb = *reinterpret_cast<const bf16x8*>(
              v_raw + krow * SWB + kswz(krow, d0 * 2));
          dp_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              do_frag[c], vb, dp_acc[nt], 0, 0, 0);
        }
      }
    }

    const int col = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0c + (lane >> 4) * 4 + r;
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int kcol = k_base + nt * 16 + col;
        const bool masked = CAUSAL ? (kcol > qrow) : (kcol >= klen);
        float pv = masked ? 0.f : __expf(s_acc[nt][r] - lse_r[r]);
        float dpv = dp_acc[nt][r];
        if (drop_thresh) {
          const unsigned long long idx =
              (bh * (unsigned long long)sq + qrow) *
                  (unsigned long long)sk + kcol;
          dpv = (fa_hash(drop_seed, idx) < drop_thresh)
                    ? 0.f : dpv * keep_scale;
        }
        float ds = pv * (dpv - dlt_r[r]) * scale;
        p_lds[wave][row][nt * 16 + col] = fa_bf16bits(ds);
      }
    }
    __builtin_amdgcn_s_waitcnt(0);

    {
      const int row = lane & 15;
      const int kv0 = (lane >> 4) * 8;
      bf16x8 pa = *reinterpret_cast<const bf16x8*>(&p_lds[wave][row][kv0]);
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
        const int dcol = t * 16 + (lane & 15);
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &kt_lds[dcol][kv0 ^ (dcol & 0x18)]);
        dq_acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pa, bfrag, dq_acc[t], 0, 0, 0);
      }
    }
  }

  if (!q_active) return;
  const int col = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + (lane >> 4) * 4 + r;
    if (qrow >= sq) continue;
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      const int d = t * 16 + col;
      if (d < D) dQp[(long)qrow * D + d] = __float2bfloat16(dq_acc[t][r]);
    }
  }
}

// KV-major: each block owns 128 kv rows (wave -> 16), streams Q in 32-tiles.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(FA_WAVES * 64)
void flash_attn_bwd_dkv_kernel(const bf16_t* __restrict__ Q,
                               const bf16_t* __restrict__ K,
                               const bf16_t* __restrict__ V,
                               const bf16_t* __restrict__ dO,
                               const float* __restrict__ LSE,
                               const float* __restrict__ Delta,
                               bf16_t* __restrict__ dK,
                               bf16_t* __restrict__ dV,
                               const int* __restrict__ klens,
                               int b, int h, int sq, int sk, float scale,
                               unsigned int drop_thresh, float keep_scale,
                               unsigned long long drop_seed) {
  constexpr int DP = fa_dpad(D);
  constexpr int NC = DP / 32;
  constexpr int NTO = DP / 16;
  constexpr int SWB = fa_swb(DP);

  __shared__ char q_raw[FB_T * SWB];
  __shared__ char do_raw[FB_T * SWB];
  __shared__ short qt_lds[DP][FB_T + FA_VPAD];
  __shared__ short dot_lds[DP][FB_T + FA_VPAD];
  __shared__ short p_lds[FA_WAVES][16][FB_T + FA_VPAD];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const long bh = (long)blockIdx.z * h + blockIdx.y;
  const bf16_t* Qp = Q + bh * sq * D;
  const bf16_t* Kp = K + bh * sk * D;
  const bf16_t* Vp = V + bh * sk * D;
  const bf16_t* dOp = dO + bh * sq * D;
  bf16_t* dKp = dK + bh * sk * D;
  bf16_t* dVp = dV + bh * sk * D;
  const float* lse = LSE + bh * sq;
  const float* dlt = Delta + bh * sq;

  const int klen = CAUSAL ? sk
                          : min(klens ? klens[blockIdx.z] : sk, sk);

  // each block owns FA_WAVES*16 kv rows
  const int kv0_blk = blockIdx.x * (FA_WAVES * 16);
  const int kv0_wave = kv0_blk + wave * 16;
  const bool kv_active = kv0_wave < sk;
  const int kv0c = kv_active ? kv0_wave : (sk > 16 ? sk - 16 : 0);

  bf16x8 k_frag[NC], v_frag[NC];
  {
    const int row = lane & 15;
    const int c0 = (lane >> 4) * 8;
    const int kvrow = min(kv0c + row, sk - 1);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8 raw = fa_load8<D>(Kp + (long)kvrow * D, c * 32 + c0);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        unsigned short u = (unsigned short)raw[j];
        float f = __uint_as_float(((unsigned int)u) << 16) * scale;
        raw[j] = fa_bf16bits(f);
      }
      k_frag[c] = raw;
      v_frag[c] = fa_load8<D>(Vp + (long)kvrow * D, c * 32 + c0);
    }
  }

  f32x4 dv_acc[NTO], dk_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) {
    dv_acc[t] = f32x4{0, 0, 0, 0};
    dk_acc[t] = f32x4{0, 0, 0, 0};
  }

  const int first_qt = CAUSAL ? kv0_blk / FB_T : 0;
  const int n_q_tiles = (sq + FB_T - 1) / FB_T;

  constexpr int BELEMS = FB_T * DP;
  constexpr int BSWEEPS = (BELEMS + FA_WAVES * 64 * 8 - 1)
                          / (FA_WAVES * 64 * 8);
  bf16x8 qst[BSWEEPS], dst[BSWEEPS];
  {
    const int tid = threadIdx.x;
    const int q0_base = first_qt * FB_T;
#pragma unroll
    for (int sw = 0; sw < BSWEEPS; ++sw) {
      const int i = tid * 8 + sw * (FA_WAVES * 64 * 8);
      if (i < BELEMS) {
        const int qr = i / DP;
        const int qc = i % DP;
        const long qrg = min(q0_base + qr, sq - 1);
        qst[sw] = fa_load8<D>(Qp + qrg * D, qc);
        dst[sw] = fa_load8<D>(dOp + qrg * D, qc);
      }
    }
  }
  for (int qt = first_qt; qt < n_q_tiles; ++qt) {
    const int q_base = qt * FB_T;
    __syncthreads();
    {
      const int tid = threadIdx.x;
#pragma unroll
      for (int sw = 0; sw < BSWEEPS; ++sw) {
        const int i = tid * 8 + sw * (FA_WAVES * 64 * 8);
        if (i < BELEMS) {
          const int qr = i / DP;
          const int qc = i % DP;
          bf16x8 qq = qst[sw];
          bf16x8 dd = dst[sw];
          *reinterpret_cast<bf16x8*>(
              q_raw + qr * SWB + kswz(qr, qc * 2)) = qq;
          *reinterpret_cast<bf16x8*>(
              do_raw + qr * SWB + kswz(qr, qc * 2)) = dd;
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            qt_lds[qc + j][qr ^ ((qc + j) & 0x18)] = qq[j];
            dot_lds[qc + j][qr ^ ((qc + j) & 0x18)] = dd[j];
          }
        }
      }
    }
    __syncthreads();
    if (qt + 1 < n_q_tiles) {
      const int nb = (qt + 1) * FB_T;
      const int tid = threadIdx.x;
#pragma unroll
      for (int sw = 0; sw < BSWEEPS; ++sw) {
        const int i = tid * 8 + sw * (FA_WAVES * 64 * 8);
        if (i < BELEMS) {
          const int qr = i / DP;
          const int qc = i % DP;
          const long qrg = min(nb + qr, sq - 1);
          qst[sw] = fa_load8<D>(Qp + qrg * D, qc);
          dst[sw] = fa_load8<D>(dOp + qrg * D, qc);
        }
      }
    }

    f32x4 st_acc[2], dpt_acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      st_acc[nt] = f32x4{0, 0, 0, 0};
      dpt_acc[nt] = f32x4{0, 0, 0, 0};
    }
    {
      const int col = lane & 15;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int qrow = nt * 16 + col;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int d0 = c * 32 + (lane >> 4) * 8;
          bf16x8 qb = *reinterpret_cast<const bf16x8*>(
              q_raw + qrow * SWB + kswz(qrow, d0 * 2));
          st_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              k_frag[c], qb, st_acc[nt], 0, 0, 0);
          bf16x8 db = *reinterpret_cast<const bf16x8*>(
              do_raw + qrow * SWB + kswz(qrow, d0 * 2));
          dpt_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              v_frag[c], db, dpt_acc[nt], 0, 0, 0);
        }
      }
    }

    const int col = lane & 15;
    float pt[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int qcol = q_base + nt * 16 + col;
      const int qcolc = min(qcol, sq - 1);
      const float lse_c = lse[qcolc];
      const float dlt_c = dlt[qcolc];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kvrow = kv0c + (lane >> 4) * 4 + r;
        bool masked = CAUSAL ? (qcol < kvrow)
                             : (kvrow >= klen || qcol >= sq);
        float pv = masked ? 0.f : __expf(st_acc[nt][r] - lse_c);
        float dm = 1.f;
        if (drop_thresh) {
          const unsigned long long idx =
              (bh * (unsigned long long)sq + qcol) *
                  (unsigned long long)sk + kvrow;
          dm = (fa_hash(drop_seed, idx) < drop_thresh) ? 0.f : keep_scale;
        }
        pt[nt][r] = pv * dm;                       // dropped P feeds dV
        dpt_acc[nt][r] = pv * (dm * dpt_acc[nt][r] - dlt_c) * scale;  // dSt
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        p_lds[wave][row][nt * 16 + col] = fa_bf16bits(pt[nt][r]);
    }
    __builtin_amdgcn_s_waitcnt(0);
    {
      const int row = lane & 15;
      const int q0f = (lane >> 4) * 8;
      bf16x8 pa = *reinterpret_cast<const bf16x8*>(&p_lds[wave][row][q0f]);
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
        const int dcol = t * 16 + (lane & 15);
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &dot_lds[dcol][q0f ^ (dcol & 0x18)]);
        dv_acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pa, bfrag, dv_acc[t], 0, 0, 0);
      }
    }

    __builtin_amdgcn_s_waitcnt(0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        p_lds[wave][row][nt * 16 + col] = fa_bf16bits(dpt_acc[nt][r]);
    }
    __builtin_amdgcn_s_waitcnt(0);
    {
      const int row = lane & 15;
      const int q0f = (lane >> 4) * 8;
      bf16x8 pa = *reinterpret_cast<const bf16x8*>(&p_lds[wave][row][q0f]);
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
        const int dcol = t * 16 + (lane & 15);
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            &qt_lds[dcol][q0f ^ (dcol & 0x18)]);
        dk_acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            pa, bfrag, dk_acc[t], 0, 0, 0);
      }
    }
  }

  if (!kv_active) return;
  const int col = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kvrow = kv0_wave + (lane >> 4) * 4 + r;
    if (kvrow >= sk) continue;
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      const int d = t * 16 + col;
      if (d < D) {
        dKp[(long)kvrow * D + d] = __float2bfloat16(dk_acc[t][r]);
        dVp[(long)kvrow * D + d] = __float2bfloat16(dv_acc[t][r]);
      }
    }
  }
}

// ===========================================================================
// launchers
// ===========================================================================
template <int D>
static void launch_fwd(bool causal, const void* q, const void* k,
                       const void* v, void* o, float* lse, const int* klens,
                       int b, int h, int sq, int sk, float scale,
                       unsigned int dth, float ksc, unsigned long long seed,
                       hipStream_t stream) {
  dim3 grid((sq + FA_QBLK - 1) / FA_QBLK, h, b);
  dim3 block(FA_WAVES * 64);
  if (causal)
    hipLaunchKernelGGL((flash_attn_fwd_kernel<D, true>), grid, block, 0,
                       stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (bf16_t*)o, lse, klens, b, h, sq, sk,
                       scale, dth, ksc, seed);
  else
    hipLaunchKernelGGL((flash_attn_fwd_kernel<D, false>), grid, block, 0,
                       stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (bf16_t*)o, lse, klens, b, h, sq, sk,
                       scale, dth, ksc, seed);
}

extern "C" void fs_flash_attn_fwd(const void* q, const void* k, const void* v,
                                  void* o, float* lse, const int* klens,
                                  int b, int h, int sq, int sk, int d,
                                  int causal, float scale, float drop_p,
                                  unsigned long long seed,
                                  hipStream_t stream) {
  const unsigned int dth =
      (drop_p > 0.f) ? (unsigned int)(drop_p * 4294967296.0) : 0u;
  const float ksc = (drop_p > 0.f) ? 1.f / (1.f - drop_p) : 1.f;
#define FWD_CASE(DD) case DD: launch_fwd<DD>(causal, q, k, v, o, lse, klens, \
    b, h, sq, sk, scale, dth, ksc, seed, stream); break;
  switch (d) {
    FWD_CASE(40) FWD_CASE(64) FWD_CASE(80)
    FWD_CASE(96) FWD_CASE(128) FWD_CASE(160)
  }
#undef FWD_CASE
}

template <int D>
static void launch_bwd(bool causal, const void* q, const void* k,
                       const void* v, const void* o, const void* dout,
                       const float* lse, void* dq, void* dk, void* dv,
                       float* delta_ws, const int* klens, int b, int h,
                       int sq, int sk, float scale, unsigned int dth,
                       float ksc, unsigned long long seed,
                       hipStream_t stream) {
  const long rows = (long)b * h * sq;
  {
    long blocks = (rows + 3) / 4;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((flash_delta_kernel<D>), dim3((unsigned)blocks),
                       dim3(256), 0, stream, (const bf16_t*)dout,
                       (const bf16_t*)o, delta_ws, rows);
  }
  dim3 gq((sq + FA_QBLK - 1) / FA_QBLK, h, b);
  dim3 gkv((sk + FA_WAVES * 16 - 1) / (FA_WAVES * 16), h, b);
  dim3 block(FA_WAVES * 64);
  if (causal) {
    hipLaunchKernelGGL((flash_attn_bwd_dq_kernel<D, true>), gq, block, 0,
                       stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (const bf16_t*)dout, lse, delta_ws,
                       (bf16_t*)dq, klens, b, h, sq, sk, scale, dth, ksc,
                       seed);
    hipLaunchKernelGGL((flash_attn_bwd_dkv_kernel<D, true>), gkv, block, 0,
                       stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (const bf16_t*)dout, lse, delta_ws,
                       (bf16_t*)dk, (bf16_t*)dv, klens, b, h, sq, sk, scale,
                       dth, ksc, seed);
  } else {
    hipLaunchKernelGGL((flash_attn_bwd_dq_kernel<D, false>), gq, block, 0,
                       stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (const bf16_t*)dout, lse, delta_ws,
                       (bf16_t*)dq, klens, b, h, sq, sk, scale, dth, ksc,
                       seed);
    hipLaunchKernelGGL((flash_attn_bwd_dkv_kernel<D, false>), gkv, block, 0,
                       stream, (const bf16_t*)q, (const bf16_t*)k,
                       (const bf16_t*)v, (const bf16_t*)dout, lse, delta_ws,
                       (bf16_t*)dk, (bf16_t*)dv, klens, b, h, sq, sk, scale,
                       dth, ksc, seed);
  }
}

extern "C" void fs_flash_attn_bwd(const void* q, const void* k, const void* v,
                                  const void* o, const void* dout,
                                  const float* lse, void* dq, void* dk,
                                  void* dv, float* delta_ws, const int* klens,
                                  int b, int h, int sq, int sk, int d,
                                  int causal, float scale, float drop_p,
                                  unsigned long long seed,
                                  hipStream_t stream) {
  const unsigned int dth =
      (drop_p > 0.f) ? (unsigned int)(drop_p * 4294967296.0) : 0u;
  const float ksc = (drop_p > 0.f) ? 1.f / (1.f - drop_p) : 1.f;
#define BWD_CASE(DD) case DD: launch_bwd<DD>(causal, q, k, v, o, dout, lse, \
    dq, dk, dv, delta_ws, klens, b, h, sq, sk, scale, dth, ksc, seed, \
    stream); break;
  switch (d) {
    BWD_CASE(40) BWD_CASE(64) BWD_CASE(80)
    BWD_CASE(96) BWD_CASE(128) BWD_CASE(160)
  }
#undef BWD_CASE
}

// ===========================================================================
// FORWARD v3 — 8-wave swapped-QK^T schedule (guide §B 8-warp ladder)
// ===========================================================================
// Causal, D=128 (the flagship LLaMA shape).  Differences vs the general
// kernel above:
//   - wave owns 32 q rows (QBLK = 256/block): K/V LDS traffic is amortized
//     over 2x more query rows;
//   - mfma_f32_32x32x16_bf16 with SWAPPED operands (A = K-tile, B = Q):
//     each lane holds a full 32-wide P-row slice for ONE q row in
//     registers, so the row max/sum are 31 in-lane ops + one cross-half
//     shuffle — no 4-round shuffle-reduce trees, and softmax state m/l is
//     a per-lane scalar;
//   - P reaches the PV A-operand in registers (cvt-pack + permlane32_swap);
//   - V is staged row-major once and read column-wise with the transposed
//     LDS read (no second, transposed image);
//   - causal: a wave skips the tiles that lie wholly above its q rows.
// Layouts verified on HW by scripts/mfma32_probe.hip and
// scripts/ds_read_tr_probe.hip.

#define V3_QBLK 256          // 8 waves x 32 q rows
#define V3_KVBLK 64

typedef __attribute__((ext_vector_type(16))) float f32x16;

// Element strides of a logical [b, h, s, D] tensor whose last dim is
// unit-stride.  The v3 kernels address every operand through one of these,
// so they read q/k/v straight out of a packed [b, s, 3*h*D] projection
// output and write O / dQ / dK / dV where the next GEMM wants them.
// Every stride (and base offset) must be a multiple of 8 elements: all
// global accesses are 16-byte vectors.
struct FaStrides {
  long b, h, r;
};

// ---- one LDS image per streamed tile, read by rows AND by columns --------
// A streamed tile (K, V, Q, dO) is staged once, row-major, with 16-byte
// stores.  MFMAs that want its rows read 16-byte chunks (ds_read_b128);
// MFMAs that want its columns (V in P.V, K in dS.K, dO in Pt.dO, Q in dSt.Q)
// use the gfx950 transposed read ds_read_b64_tr_b16: per 16-lane group,
// lane i supplies the address of row i>>2, columns 4*(i&3)..+3 of a 4-row x
// 16-column block and receives column i of it, row q in element q (verified
// on HW by scripts/ds_read_tr_probe.hip).  The read gathers across lanes, so
// EXEC must be all ones: every call sits in wave-uniform control flow, and
// inactive waves compute on clamped rows instead of being masked off.
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((address_space(3))) bf16x4 lds_bf16x4;

// Byte offset of 16-byte chunk `ch` of row `row`.  SWB (row stride in bytes)
// is 256 for D = 128 / 96 and 128 for D = 64.  The chunk XOR keeps the
// staging store, the row read and the transposed read of the 32x32x16
// operands free of bank conflicts (64 banks of 4 B for the reads, 32 for
// the store); it only uses row bits 0..3, so tiles of 16-row multiples
// share one per-lane address.
template <int SWB>
__device__ __forceinline__ int v3_off(int row, int ch) {
  static_assert(SWB == 256 || SWB == 128, "row stride");
  if (SWB == 256)
    return 256 * row + 16 * (ch ^ (((row & 3) << 2) | ((row >> 2) & 3)));
  return 128 * row + 16 * (ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3)));
}

// This lane's address for the transposed read of the 4-row block at row0 of
// the 32 columns starting at col0 (lanes 0-15 and 32-47 take columns
// col0..+15, the others col0+16..+31).
template <int SWB>
__device__ __forceinline__ int v3_tr_addr(int lane, int row0, int col0) {
  const int i = lane & 15;
  const int col = col0 + 16 * ((lane >> 4) & 1) + 4 * (i & 3);
  return v3_off<SWB>(row0 + (i >> 2), col >> 3) + 2 * (col & 7);
}

// B fragment of mfma_f32_32x32x16_bf16 (element j = X[k0 + 8*hi + j][col0 +
// ln]) from a row-major image; a0 / a1 = v3_tr_addr of rows k0 + 8*hi and
// k0 + 8*hi + 4.  The same call yields the A fragment of X^T.
__device__ __forceinline__ bf16x8 v3_tr_frag(const char* a0, const char* a1) {
  const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)a0);
  const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_bf16x4*)a1);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// B fragment for d columns 32*t + ln of the 16 rows at `rows`, from one
// per-lane base tbase = v3_tr_addr(lane, 8*hi, 0): tile t flips chunk bits
// 2..3 (byte bits 6..7) and the second 4-row block flips chunk bit 0, so
// the other addresses are one XOR away and need no registers of their own.
template <int SWB>
__device__ __forceinline__ bf16x8 v3_tr_bfrag(const char* rows, int tbase,
                                              int t) {
  const int a0 = tbase ^ (64 * t);
  return v3_tr_frag(rows + a0, rows + (a0 ^ 16) + 4 * SWB);
}

// Wait for this wave's LDS traffic only (lgkmcnt(0); vmcnt and expcnt left
// at their maxima).  The per-wave exchanges use it instead of a full
// s_waitcnt 0, which would also wait for the next tile's global prefetch.
__device__ __forceinline__ void v3_wait_lds() {
  __builtin_amdgcn_s_waitcnt(0xC07F);
}

// dkv exchange image, [32 rows][32 x 16-bit] with 64-byte rows: byte offset
// of 8-byte unit u of `row`.  The 16 lanes of one ds_write_b64 group store
// the same unit of 16 consecutive rows; the XOR spreads them over all 32
// store banks.  A transposed read takes 4 whole rows (256 contiguous bytes)
// per 32-lane half, conflict-free under any unit permutation.
__device__ __forceinline__ int dkv_xoff(int row, int u) {
  return 64 * row + 8 * (u ^ ((row >> 1) & 7));
}

// ---- per-row key start (KS instantiations) ---------------------------------
// kstart [b, s] int32: query row i sees keys kstart[i] <= j <= i, which is
// right padding (0), left padding by p (p), packed documents (start of the
// row's document) and pad rows (i) in one mask.  The value is clamped into
// [0, row] where it is read, so whatever it holds can change which keys a
// row sees and never an address; every row keeps at least its own key.
__device__ __forceinline__ int v3_kstart_at(const int* ksb, int row) {
  return min(max(ksb[row], 0), row);
}

// Minimum of v over the wave, as a scalar.
__device__ __forceinline__ int v3_wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
  return __builtin_amdgcn_readfirstlane(v);
}

// Smallest key start of the 256 query rows of block `blk`: no row of the
// block sees a key before it, so the key loop starts at that key's tile.
// Every wave computes it for itself (4 loads per lane and one butterfly),
// which needs neither LDS nor a barrier.
__device__ __forceinline__ int v3_block_kstart_min(const int* ksb, int blk,
                                                   int lane, int s) {
  int m = s;
#pragma unroll
  for (int j = 0; j < V3_QBLK / 64; ++j)
    m = min(m, v3_kstart_at(ksb, min(blk * V3_QBLK + 64 * j + lane, s - 1)));
  return v3_wave_min(m);
}

// ---- which (x, head, batch) this block computes ----------------------------
// The v3 kernels launch the grid (x, head, batch) they always had and take
// their coordinates from the XCD-aware map of flash_blockmap.h instead of
// blockIdx: the blocks that share an XCD run whole (batch, head) columns,
// heaviest block first, instead of all the blocks of one x.  heavy_last:
// fwd and dq do more work at large x, dkv at small x (causal); without a
// mask only the L2 sharing is left.  Everything is wave-uniform.
__device__ __forceinline__ FlashBlock v3_block(bool heavy_last) {
  const unsigned int L =
      blockIdx.x + gridDim.x * (blockIdx.y + gridDim.y * blockIdx.z);
  return flash_v3_block_of(L, gridDim.x, gridDim.y, gridDim.z, heavy_last);
}

// ---- grouped-query attention (GQA instantiations) --------------------------
// K/V (and dK/dV) carry h_kv = h / G heads with FaStrides of their own (kvs,
// gkvs); query head j uses KV head j / G.  fwd and dq keep one block per
// query head and only point Kp/Vp at the shared head; dkv runs one block per
// KV head and walks the G query heads of its group into one fp32
// accumulator.  Like kstart, the arguments come last and are not read when
// GQA = false, so the plain instantiations compile to the code they had.
// Causal, no dropout, with or without KS.

// delta[b,h,s] = rowsum(dO * O) over strided rows; same per-row arithmetic
// as flash_delta_kernel.  Grid (x, h, b): blockIdx.y/z pick the head and
// batch, so the [b, h, s] output index needs no division; the 4 waves of a
// block walk the s rows of that head in a grid-stride loop over x.
template <int D>
__global__ __launch_bounds__(256)
void flash_delta_v3_kernel(const bf16_t* __restrict__ dO,
                           const bf16_t* __restrict__ O,
                           float* __restrict__ delta, FaStrides dos,
                           FaStrides os, int h, int s) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const bf16_t* dob = dO + blockIdx.z * dos.b + blockIdx.y * dos.h;
  const bf16_t* ob = O + blockIdx.z * os.b + blockIdx.y * os.h;
  float* dl = delta + ((long)blockIdx.z * h + blockIdx.y) * s;
  for (int row = blockIdx.x * 4 + wid; row < s; row += gridDim.x * 4) {
    const bf16_t* dop = dob + row * dos.r;
    const bf16_t* op = ob + row * os.r;
    float sacc = 0.f;
    for (int i = lane * 2; i < D; i += 128) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
        sacc += __bfloat162float(dop[i + j]) * __bfloat162float(op[i + j]);
    }
    sacc = wave_reduce_sum(sacc);
    if (lane == 0) dl[row] = sacc;
  }
}

template <int D, bool CAUSAL, bool HAS_DROP, bool KS = false,
          bool GQA = false>
__global__ __launch_bounds__(FA_WAVES * 64)
void flash_attn_fwd_v3_kernel(const bf16_t* __restrict__ Q,
                              const bf16_t* __restrict__ K,
                              const bf16_t* __restrict__ V,
                              bf16_t* __restrict__ O,
                              float* __restrict__ LSE,
                              const int* __restrict__ klens,
                              FaStrides qs, FaStrides os,
                              int b, int h, int s, float scale,
                              unsigned int drop_thresh, float keep_scale,
                              unsigned long long drop_seed,
                              const int* __restrict__ kstart,
                              FaStrides kvs, int G) {
  static_assert(!KS || (CAUSAL && !HAS_DROP), "kstart: causal, no dropout");
  static_assert(!GQA || (CAUSAL && !HAS_DROP), "GQA: causal, no dropout");
  constexpr int NC = D / 16;     // MFMA K=16 chunks
  constexpr int NTO = D / 32;    // 32-wide output d-tiles
  constexpr int SWB = fa_swb(D);

  __shared__ __attribute__((aligned(16)))
  char k_raw[2][V3_KVBLK * SWB];                        // swizzled K rows
  __shared__ __attribute__((aligned(16)))
  char v_raw[2][V3_KVBLK * SWB];    // V rows (v3_off), read transposed
  // (double-buffered: tile t+1 stages into buf^1 while buf holds tile t,
  // so the loop needs ONE barrier per tile instead of two.
  // P stays fully in registers via cvt-pack + permlane32_swap — T12;
  // alpha/1-l broadcasts ride lane shuffles: no LDS exchange, no
  // wave-wide lgkmcnt drains in the softmax/PV region)

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;      // lane half
  const int ln = lane & 31;
  const FlashBlock blk = v3_block(true);
  const unsigned int bx = blk.x, by = blk.y, bz = blk.z;
  const long bh = (long)bz * h + by;
  const long qoff = bz * qs.b + by * qs.h;
  const bf16_t* Qp = Q + qoff;
  // GQA: query head j reads KV head j / G through K/V's own strides
  const long kvoff =
      GQA ? bz * kvs.b + (by / G) * kvs.h : qoff;
  const long kv_r = GQA ? kvs.r : qs.r;
  const bf16_t* Kp = K + kvoff;
  const bf16_t* Vp = V + kvoff;
  bf16_t* Op = O + bz * os.b + by * os.h;

  const int klen = CAUSAL ? s : min(klens ? klens[bz] : s, s);

  const int q0w = bx * V3_QBLK + wave * 32;
  const bool q_active = q0w < s;
  const int q0c = q_active ? q0w : s - 32;
  const int my_q = q0c + ln;      // softmax row this lane owns

  // ---- Q -> B-fragments (K=16 chunks), pre-scaled -----------------------
  bf16x8 q_frag[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    bf16x8 raw = *reinterpret_cast<const bf16x8*>(
        Qp + (long)my_q * qs.r + c * 16 + hi * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned short u = (unsigned short)raw[j];
      float f = __uint_as_float(((unsigned int)u) << 16) * scale;
      raw[j] = fa_bf16bits(f);
    }
    q_frag[c] = raw;
  }

  // KS: this lane's key start, the wave's smallest one (a tile that ends
  // before it is invisible to the whole wave) and the block's first tile
  int ks_q = 0, ks_w = 0, kt0 = 0;
  if (KS) {
    const int* ksb = kstart + (long)bz * s;
    ks_q = v3_kstart_at(ksb, my_q);
    ks_w = v3_wave_min(ks_q);
    kt0 = v3_block_kstart_min(ksb, bx, lane, s) / V3_KVBLK;
  }

  // per-lane: row my_q.  KS: a wave runs a tile as soon as one of its rows
  // sees a key in it, so a row can meet tiles in which all of its own keys
  // are masked before it meets a visible one.  A finite start keeps
  // m_new - m_run and p - m_new free of inf - inf there (alpha = 1 on
  // l = 0, then alpha = exp(-1e30 - m) = 0 at the first visible key, the
  // value the -inf guard below gives the plain kernels).
  float m_run = KS ? -1e30f : -INFINITY, l_run = 0.f;
  f32x16 o_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) o_acc[t][r] = 0.f;
  }

  int n_kv_tiles;
  if (CAUSAL) {
    const int q_hi_row = min(bx * V3_QBLK + V3_QBLK, s) - 1;
    n_kv_tiles = (q_hi_row / V3_KVBLK) + 1;
  } else {
    n_kv_tiles = (klen + V3_KVBLK - 1) / V3_KVBLK;
    if (n_kv_tiles < 1) n_kv_tiles = 1;
  }

  // async-STAGE staging registers
  const int tid = threadIdx.x;
  constexpr int ELEMS = V3_KVBLK * D;
  constexpr int SWEEPS = (ELEMS + FA_WAVES * 64 * 8 - 1) / (FA_WAVES * 64 * 8);
  bf16x8 k_reg[SWEEPS], v_reg[SWEEPS];
#pragma unroll
  for (int sweep = 0; sweep < SWEEPS; ++sweep) {
    const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
    if (i < ELEMS) {
      const long kr = KS ? min(kt0 * V3_KVBLK + i / D, s - 1)
                         : min(i / D, s - 1);
      const int kc = i % D;
      k_reg[sweep] = *reinterpret_cast<const bf16x8*>(Kp + kr * kv_r + kc);
      v_reg[sweep] = *reinterpret_cast<const bf16x8*>(Vp + kr * kv_r + kc);
    }
  }

  // stage the first tile into buffer 0
  {
#pragma unroll
    for (int sweep = 0; sweep < SWEEPS; ++sweep) {
      const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
      if (i < ELEMS) {
        const int kr = i / D;
        const int kc = i % D;
        *reinterpret_cast<bf16x8*>(
            k_raw[0] + kr * SWB + kswz(kr, kc * 2)) = k_reg[sweep];
        *reinterpret_cast<bf16x8*>(
            v_raw[0] + v3_off<SWB>(kr, kc >> 3)) = v_reg[sweep];
      }
    }
  }
  // transposed-read base: V rows 8*hi.., d columns ln (v3_tr_bfrag); kv
  // chunk c2 adds 16 rows, which leaves the swizzle term unchanged
  const int v_tr = v3_tr_addr<SWB>(lane, 8 * hi, 0);
  // causal: a wave whose last q row lies above a tile sees only masked
  // entries there (P = 0 exactly, m/l unchanged) and skips the compute
  // part; staging and the barrier stay unconditional.  The test is on the
  // wave's first lane so the branch is scalar and EXEC stays full.
  const int q_last_w = __builtin_amdgcn_readfirstlane(q0c) + 31;

  int cur = 0;
  for (int kt = KS ? kt0 : 0; kt < n_kv_tiles; ++kt) {
    const int k_base = kt * V3_KVBLK;
    __syncthreads();  // publishes buf[cur]; everyone done with buf[cur^1]
    if (kt + 1 < n_kv_tiles) {
      const int nb = (kt + 1) * V3_KVBLK;
#pragma unroll
      for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
        if (i < ELEMS) {
          const long kr = min((long)(nb + i / D), (long)s - 1);
          const int kc = i % D;
          k_reg[sweep] = *reinterpret_cast<const bf16x8*>(Kp + kr * kv_r + kc);
          v_reg[sweep] = *reinterpret_cast<const bf16x8*>(Vp + kr * kv_r + kc);
        }
      }
    }

    if ((!CAUSAL || k_base <= q_last_w) &&
        (!KS || k_base + V3_KVBLK > ks_w)) {
      // ---- S^T = K_tile @ (sQ)^T : two 32x32 kv-tiles ---------------------
      f32x16 st[2];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[nt][r] = 0.f;
      }
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int krow = nt * 32 + ln;
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          bf16x8 a = *reinterpret_cast<const bf16x8*>(
              k_raw[cur] + krow * SWB + kswz(krow, (c * 16 + hi * 8) * 2));
          st[nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, q_frag[c],
                                                           st[nt], 0, 0, 0);
        }
      }
      // lane now holds S^T[kv][q = my row]: kv = k_base + nt*32 + crow(r,hi)
      // with crow(r,hi) = (r&3) + 8*(r>>2) + 4*hi

      // ---- causal mask + in-register online softmax ----------------------
      float p[32];
      float tmax = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kcol = k_base + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
          float v = st[nt][r];
          if (CAUSAL ? (kcol > my_q || (KS && kcol < ks_q)) : (kcol >= klen))
            v = -INFINITY;
          p[nt * 16 + r] = v;
          tmax = fmaxf(tmax, v);
        }
      }
      tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));  // combine lane halves
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = (m_run == -INFINITY) ? 0.f : __expf(m_run - m_new);
      const bool rescale = (m_new != m_run);
      m_run = m_new;
      float rs = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        float e = (p[i] == -INFINITY) ? 0.f : __expf(p[i] - m_new);
        p[i] = e;
        rs += e;
      }
      rs += __shfl_xor(rs, 32, 64);
      l_run = l_run * alpha + rs;

      // attention dropout on P (normalizer keeps the undropped sum)
      if (HAS_DROP && drop_thresh) {
        const unsigned long long qi =
            (bh * (unsigned long long)s + my_q) * (unsigned long long)s;
#pragma unroll
        for (int nt = 0; nt < 2; ++nt) {
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int kcol =
                k_base + nt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            float& pv = p[nt * 16 + r];
            pv = (fa_hash(drop_seed, qi + kcol) < drop_thresh)
                     ? 0.f : pv * keep_scale;
          }
        }
      }

      // rescale: alpha for o-row crow(r,hi) fetched by lane shuffle
      // (alpha is per-q-row, identical in lanes l and l+32)
      if (__any(rescale)) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float al = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
#pragma unroll
          for (int t = 0; t < NTO; ++t) o_acc[t][r] *= al;
        }
      }

      // ---- P -> A-fragments in registers (T12) ----------------------------
      // Lane layout: p holds, for its own q row, kv octs G = 4*nt + g with
      // 4-runs at kv = 8G + 4*hi + j.  A-frag for PV chunk c2 needs kv
      // 16c2 + 8*hi' + j: word pair k from oct 2c2 (hi=0 half) and oct
      // 2c2+1 (hi=1 half).  One permlane32_swap per word yields BOTH
      // halves' targets: out0 = words 0/1, out1 = words 2/3, uniformly.
      unsigned int pw[8][2];  // [oct][word]: packed bf16 pairs of own run
#pragma unroll
      for (int G = 0; G < 8; ++G) {
        const int base = (G >> 2) * 16 + (G & 3) * 4;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const unsigned int lo =
              (unsigned short)fa_bf16bits(p[base + 2 * k]);
          const unsigned int hi_b =
              (unsigned short)fa_bf16bits(p[base + 2 * k + 1]);
          pw[G][k] = (hi_b << 16) | lo;
        }
      }

      // ---- PV: O[q][d] += P[q][kv] @ V[kv][d] -----------------------------
#pragma unroll
      for (int c2 = 0; c2 < 4; ++c2) {  // kv chunks of 16
        unsigned int paw[4];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          auto pr = __builtin_amdgcn_permlane32_swap(
              (int)pw[2 * c2][k], (int)pw[2 * c2 + 1][k], false, false);
          paw[k] = (unsigned int)pr[0];
          paw[k + 2] = (unsigned int)pr[1];
        }
        bf16x8 pa;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          pa[2 * k] = (short)(paw[k] & 0xFFFF);
          pa[2 * k + 1] = (short)(paw[k] >> 16);
        }
#pragma unroll
        for (int t = 0; t < NTO; ++t) {   // d cols, 32 each
          const char* vrow = v_raw[cur] + c2 * 16 * SWB;
          bf16x8 vb = v3_tr_bfrag<SWB>(vrow, v_tr, t);
          o_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, vb, o_acc[t],
                                                             0, 0, 0);
        }
      }
    }  // tile visible to this wave

    // stage tile kt+1 into the spare buffer (loop-top barrier publishes)
    if (kt + 1 < n_kv_tiles) {
      const int nxt = cur ^ 1;
#pragma unroll
      for (int sweep = 0; sweep < SWEEPS; ++sweep) {
        const int i = tid * 8 + sweep * (FA_WAVES * 64 * 8);
        if (i < ELEMS) {
          const int kr = i / D;
          const int kc = i % D;
          *reinterpret_cast<bf16x8*>(
              k_raw[nxt] + kr * SWB + kswz(kr, kc * 2)) = k_reg[sweep];
          *reinterpret_cast<bf16x8*>(
              v_raw[nxt] + v3_off<SWB>(kr, kc >> 3)) = v_reg[sweep];
        }
      }
      cur = nxt;
    }
  }

  // ---- epilogue ---------------------------------------------------------
  if (!q_active) return;
  const float my_inv_l = (l_run > 0.f) ? 1.f / l_run : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qrow = q0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
    const float inv_l =
        __shfl(my_inv_l, (r & 3) + 8 * (r >> 2) + 4 * hi, 64);
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      Op[(long)qrow * os.r + t * 32 + ln] =
          __float2bfloat16(o_acc[t][r] * inv_l);
    }
  }
  if (hi == 0 && LSE) {
    LSE[bh * s + q0w + ln] = m_run + logf(fmaxf(l_run, 1e-30f));
  }
}

// qs3 / os3: (batch, head, row) element strides of q|k|v and of o.
extern "C" void fs_flash_attn_fwd_v3_strided(
    const void* q, const void* k, const void* v, void* o, float* lse,
    const int* klens, const long* qs3, const long* os3, int b, int h, int s,
    int d, int causal, float scale, float drop_p, unsigned long long seed,
    hipStream_t stream) {
  const FaStrides qs{qs3[0], qs3[1], qs3[2]};
  const FaStrides os{os3[0], os3[1], os3[2]};
  dim3 grid((s + V3_QBLK - 1) / V3_QBLK, h, b);
  dim3 block(FA_WAVES * 64);
  const unsigned int dth =
      (drop_p > 0.f) ? (unsigned int)(drop_p * 4294967296.0) : 0u;
  const float ksc = (drop_p > 0.f) ? 1.f / (1.f - drop_p) : 1.f;
#define V3F(DD, CC, DR) hipLaunchKernelGGL( \
    (flash_attn_fwd_v3_kernel<DD, CC, DR>), \
    grid, block, 0, stream, (const bf16_t*)q, (const bf16_t*)k, \
    (const bf16_t*)v, (bf16_t*)o, lse, klens, qs, os, b, h, s, scale, dth, \
    ksc, seed, (const int*)nullptr, FaStrides{}, 1)
  if (dth) {
    if (d == 128 && causal) V3F(128, true, true);
    else if (d == 128) V3F(128, false, true);
    else if (d == 96 && causal) V3F(96, true, true);
    else if (d == 96) V3F(96, false, true);
    else if (d == 64 && causal) V3F(64, true, true);
    else V3F(64, false, true);
  } else {
    if (d == 128 && causal) V3F(128, true, false);
    else if (d == 128) V3F(128, false, false);
    else if (d == 96 && causal) V3F(96, true, false);
    else if (d == 96) V3F(96, false, false);
    else if (d == 64 && causal) V3F(64, true, false);
    else V3F(64, false, false);
  }
#undef V3F
}

// Causal forward with a per-row key start (kstart [b, s] int32, see
// v3_kstart_at); no dropout, no klens.
extern "C" void fs_flash_attn_fwd_v3_kstart(
    const void* q, const void* k, const void* v, void* o, float* lse,
    const int* kstart, const long* qs3, const long* os3, int b, int h, int s,
    int d, float scale, hipStream_t stream) {
  const FaStrides qs{qs3[0], qs3[1], qs3[2]};
  const FaStrides os{os3[0], os3[1], os3[2]};
  dim3 grid((s + V3_QBLK - 1) / V3_QBLK, h, b);
  dim3 block(FA_WAVES * 64);
#define V3K(DD) hipLaunchKernelGGL( \
    (flash_attn_fwd_v3_kernel<DD, true, false, true>), \
    grid, block, 0, stream, (const bf16_t*)q, (const bf16_t*)k, \
    (const bf16_t*)v, (bf16_t*)o, lse, (const int*)nullptr, qs, os, b, h, s, \
    scale, 0u, 1.f, 0ull, kstart, FaStrides{}, 1)
  if (d == 128) V3K(128);
  else if (d == 96) V3K(96);
  else V3K(64);
#undef V3K
}

// Grouped-query causal forward: q/o have h heads, k/v h_kv = h / G heads
// with strides kvs3 of their own; query head j reads KV head j / G.
// kstart may be null.  No dropout, no klens.
extern "C" void fs_flash_attn_fwd_v3_gqa(
    const void* q, const void* k, const void* v, void* o, float* lse,
    const int* kstart, const long* qs3, const long* kvs3, const long* os3,
    int b, int h, int h_kv, int s, int d, float scale, hipStream_t stream) {
  const FaStrides qs{qs3[0], qs3[1], qs3[2]};
  const FaStrides kvs{kvs3[0], kvs3[1], kvs3[2]};
  const FaStrides os{os3[0], os3[1], os3[2]};
  dim3 grid((s + V3_QBLK - 1) / V3_QBLK, h, b);
  dim3 block(FA_WAVES * 64);
#define V3G(DD, KK) hipLaunchKernelGGL( \
    (flash_attn_fwd_v3_kernel<DD, true, false, KK, true>), \
    grid, block, 0, stream, (const bf16_t*)q, (const bf16_t*)k, \
    (const bf16_t*)v, (bf16_t*)o, lse, (const int*)nullptr, qs, os, b, h, s, \
    scale, 0u, 1.f, 0ull, kstart, kvs, h / h_kv)
  if (kstart) {
    if (d == 128) V3G(128, true);
    else if (d == 96) V3G(96, true);
    else V3G(64, true);
  } else {
    if (d == 128) V3G(128, false);
    else if (d == 96) V3G(96, false);
    else V3G(64, false);
  }
#undef V3G
}

extern "C" void fs_flash_attn_fwd_v3(const void* q, const void* k,
                                     const void* v, void* o, float* lse,
                                     const int* klens, int b, int h, int s,
                                     int d, int causal, float scale,
                                     float drop_p, unsigned long long seed,
                                     hipStream_t stream) {
  const long c3[3] = {(long)h * s * d, (long)s * d, (long)d};
  fs_flash_attn_fwd_v3_strided(q, k, v, o, lse, klens, c3, c3, b, h, s, d,
                               causal, scale, drop_p, seed, stream);
}

// ===========================================================================
// BACKWARD v3 — swapped 32x32 schedule (causal, D=128)
// ===========================================================================
// Same design move as forward v3: orient every S-like MFMA so the softmax
// row variable (q for dq, q-column for dkv) is lane-local — lse/delta
// become per-lane scalar loads, masks are per-register compares, and the
// only cross-lane traffic is the compact P/dS LDS exchange.

#define B3_FB 32  // streamed tile width

// q-major: wave owns 32 q rows (block 256), streams KV in 32-tiles.
template <int D, bool CAUSAL, bool HAS_DROP, bool KS = false,
          bool GQA = false>
__global__ __launch_bounds__(FA_WAVES * 64)
void flash_attn_bwd_dq_v3_kernel(const bf16_t* __restrict__ Q,
                                 const bf16_t* __restrict__ K,
                                 const bf16_t* __restrict__ V,
                                 const bf16_t* __restrict__ dO,
                                 const float* __restrict__ LSE,
                                 const float* __restrict__ Delta,
                                 bf16_t* __restrict__ dQ,
                                 const int* __restrict__ klens,
                                 FaStrides qs, FaStrides dos, FaStrides gs,
                                 int b, int h, int s, float scale,
                                 unsigned int drop_thresh, float keep_scale,
                                 unsigned long long drop_seed,
                                 const int* __restrict__ kstart,
                                 FaStrides kvs, int G) {
  static_assert(!KS || (CAUSAL && !HAS_DROP), "kstart: causal, no dropout");
  static_assert(!GQA || (CAUSAL && !HAS_DROP), "GQA: causal, no dropout");
  constexpr int NC = D / 16;
  constexpr int NTO = D / 32;
  constexpr int SWB = fa_swb(D);

  // double-buffered row images (v3_off): tile t+1 stages into buf^1 while
  // buf holds tile t, so the loop needs one barrier per tile.  K is read by
  // rows for S^T and transposed for dS.K; V by rows only.
  __shared__ __attribute__((aligned(16))) char k_raw[2][B3_FB * SWB];
  __shared__ __attribute__((aligned(16))) char v_raw[2][B3_FB * SWB];
  __shared__ short p_x[FA_WAVES][32][B3_FB + FA_VPAD];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int ln = lane & 31;
  const FlashBlock blk = v3_block(true);
  const unsigned int bx = blk.x, by = blk.y, bz = blk.z;
  const long bh = (long)bz * h + by;
  const long qoff = bz * qs.b + by * qs.h;
  const bf16_t* Qp = Q + qoff;
  // GQA: query head j reads KV head j / G through K/V's own strides
  const long kvoff =
      GQA ? bz * kvs.b + (by / G) * kvs.h : qoff;
  const long kv_r = GQA ? kvs.r : qs.r;
  const bf16_t* Kp = K + kvoff;
  const bf16_t* Vp = V + kvoff;
  const bf16_t* dOp = dO + bz * dos.b + by * dos.h;
  bf16_t* dQp = dQ + bz * gs.b + by * gs.h;
  const float* lse = LSE + bh * s;
  const float* dlt = Delta + bh * s;

  const int klen = CAUSAL ? s : min(klens ? klens[bz] : s, s);
  const int q0w = bx * V3_QBLK + wave * 32;
  const bool q_active = q0w < s;
  const int q0c = q_active ? q0w : s - 32;
  const int my_q = q0c + ln;

  // Q (pre-scaled) and dO rows in registers (B-fragments)
  bf16x8 q_frag[NC], do_frag[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    bf16x8 raw = *reinterpret_cast<const bf16x8*>(
        Qp + (long)my_q * qs.r + c * 16 + hi * 8);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned short u = (unsigned short)raw[j];
      raw[j] = fa_bf16bits(
          __uint_as_float(((unsigned int)u) << 16) * scale);
    }
    q_frag[c] = raw;
    do_frag[c] = *reinterpret_cast<const bf16x8*>(
        dOp + (long)my_q * dos.r + c * 16 + hi * 8);
  }
  const float lse_r = lse[my_q];
  const float dlt_r = dlt[my_q];
  // KS: as in the forward kernel, in 32-key tiles
  int ks_q = 0, ks_w = 0, kt0 = 0;
  if (KS) {
    const int* ksb = kstart + (long)bz * s;
    ks_q = v3_kstart_at(ksb, my_q);
    ks_w = v3_wave_min(ks_q);
    kt0 = v3_block_kstart_min(ksb, bx, lane, s) / B3_FB;
  }

  f32x16 dq_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) dq_acc[t][r] = 0.f;
  }

  int n_kv_tiles;
  if (CAUSAL) {
    const int q_hi_row = min(bx * V3_QBLK + V3_QBLK, s) - 1;
    n_kv_tiles = (q_hi_row / B3_FB) + 1;
  } else {
    n_kv_tiles = (klen + B3_FB - 1) / B3_FB;
  }

  // staging: one 16-byte chunk of K and of V per thread (B3_FB * D / 8
  // <= 512 chunks), prefetched into registers under the MFMAs
  const int st_i = threadIdx.x * 8;
  const bool st_on = st_i < B3_FB * D;
  const int st_r = st_on ? st_i / D : 0;
  const int st_c = st_on ? st_i % D : 0;
  const int st_off = v3_off<SWB>(st_r, st_c >> 3);
  bf16x8 k_reg, v_reg;
  {
    const long krg = KS ? min(kt0 * B3_FB + st_r, s - 1) : min(st_r, s - 1);
    k_reg = *reinterpret_cast<const bf16x8*>(Kp + krg * kv_r + st_c);
    v_reg = *reinterpret_cast<const bf16x8*>(Vp + krg * kv_r + st_c);
  }
  if (st_on) {
    *reinterpret_cast<bf16x8*>(k_raw[0] + st_off) = k_reg;
    *reinterpret_cast<bf16x8*>(v_raw[0] + st_off) = v_reg;
  }
  // transposed-read base (v3_tr_bfrag) and row-read base: chunk 2c + hi of
  // row ln is the base with byte bits 5.. flipped by c
  const int k_tr = v3_tr_addr<SWB>(lane, 8 * hi, 0);
  const int kv_row = v3_off<SWB>(ln, hi);
  // causal: tiles wholly right of the wave's last q row give dS = 0 exactly;
  // the wave skips their compute part (scalar branch, EXEC stays full)
  const int q_last_w = __builtin_amdgcn_readfirstlane(q0c) + 31;

  int cur = 0;
  for (int kt = KS ? kt0 : 0; kt < n_kv_tiles; ++kt) {
    const int k_base = kt * B3_FB;
    __syncthreads();  // publishes buf[cur]; everyone done with buf[cur^1]
    if (kt + 1 < n_kv_tiles) {
      const long krg = min(k_base + B3_FB + st_r, s - 1);
      k_reg = *reinterpret_cast<const bf16x8*>(Kp + krg * kv_r + st_c);
      v_reg = *reinterpret_cast<const bf16x8*>(Vp + krg * kv_r + st_c);
    }

    if ((!CAUSAL || k_base <= q_last_w) && (!KS || k_base + B3_FB > ks_w)) {
      // S^T = K (sQ)^T and dP^T = V dO^T : one 32x32 kv-tile each
      f32x16 st, dpt;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        st[r] = 0.f;
        dpt[r] = 0.f;
      }
      {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int roff = kv_row ^ (32 * c);
          bf16x8 ka = *reinterpret_cast<const bf16x8*>(k_raw[cur] + roff);
          st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, q_frag[c], st,
                                                       0, 0, 0);
          bf16x8 va = *reinterpret_cast<const bf16x8*>(v_raw[cur] + roff);
          dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(va, do_frag[c], dpt,
                                                        0, 0, 0);
        }
      }
      // lane holds, for its OWN q row: kv = k_base + crow(r,hi)

      // dS = P * (dP - delta) * scale, in-register; exchange by q row
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        short pk[4] __attribute__((aligned(8)));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = g * 4 + j;
          const int kcol = k_base + (r & 3) + 8 * (r >> 2) + 4 * hi;
          const bool masked = CAUSAL ? (kcol > my_q || (KS && kcol < ks_q))
                                     : (kcol >= klen);
          float pv = masked ? 0.f : __expf(st[r] - lse_r);
          float dpv = dpt[r];
          if (HAS_DROP && drop_thresh) {
            const unsigned long long idx =
                (bh * (unsigned long long)s + my_q) *
                    (unsigned long long)s + kcol;
            dpv = (fa_hash(drop_seed, idx) < drop_thresh)
                      ? 0.f : dpv * keep_scale;
          }
          pk[j] = fa_bf16bits(pv * (dpv - dlt_r) * scale);
        }
        *reinterpret_cast<long*>(&p_x[wave][ln][8 * g + 4 * hi]) =
            *reinterpret_cast<const long*>(pk);
      }
      v3_wait_lds();

      // dQ += dS @ K : A = dS [32q x 16kv], B = K read transposed
#pragma unroll
      for (int c2 = 0; c2 < 2; ++c2) {
        bf16x8 pa = *reinterpret_cast<const bf16x8*>(
            &p_x[wave][ln][c2 * 16 + hi * 8]);
        const char* krows = k_raw[cur] + c2 * 16 * SWB;
#pragma unroll
        for (int t = 0; t < NTO; ++t) {
          bf16x8 kb = v3_tr_bfrag<SWB>(krows, k_tr, t);
          dq_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(pa, kb,
                                                              dq_acc[t],
                                                              0, 0, 0);
        }
      }
    }  // tile visible to this wave

    // stage tile kt+1 into the spare buffer (loop-top barrier publishes)
    if (kt + 1 < n_kv_tiles) {
      cur ^= 1;
      if (st_on) {
        *reinterpret_cast<bf16x8*>(k_raw[cur] + st_off) = k_reg;
        *reinterpret_cast<bf16x8*>(v_raw[cur] + st_off) = v_reg;
      }
    }
  }

  if (!q_active) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qrow = q0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
    for (int t = 0; t < NTO; ++t)
      dQp[(long)qrow * gs.r + t * 32 + ln] = __float2bfloat16(dq_acc[t][r]);
  }
}

// KV-major: wave owns 32 kv rows (block 256), streams Q/dO in 32-tiles.
// The wave's own K and V rows stay in registers for the whole loop (64
// VGPRs next to the 128 of dK/dV), which puts the kernel at the 256-VGPR
// cap: a few loop-invariant values live in scratch.
// The softmax scale folds into the exp (st*scale - lse) so K stays raw.
// KS: the query loop of a block ends at the last row that still sees one of
// its keys.  qend [b, s/64] int32 holds, per 64-key tile, the last row i
// with kstart[i] <= the tile's last key (kstart is non-decreasing, so the
// wrapper finds it with a searchsorted); the block takes the largest of
// its four tiles' entries, clamped into [the block's first row, s - 1].
template <int D, bool CAUSAL, bool HAS_DROP, bool KS = false,
          bool GQA = false>
__global__ __launch_bounds__(FA_WAVES * 64)
void flash_attn_bwd_dkv_v3_kernel(const bf16_t* __restrict__ Q,
                                  const bf16_t* __restrict__ K,
                                  const bf16_t* __restrict__ V,
                                  const bf16_t* __restrict__ dO,
                                  const float* __restrict__ LSE,
                                  const float* __restrict__ Delta,
                                  bf16_t* __restrict__ dK,
                                  bf16_t* __restrict__ dV,
                                  const int* __restrict__ klens,
                                  FaStrides qs, FaStrides dos, FaStrides gs,
                                  int b, int h, int s, float scale,
                                  unsigned int drop_thresh, float keep_scale,
                                  unsigned long long drop_seed,
                                  const int* __restrict__ kstart,
                                  const int* __restrict__ qend,
                                  FaStrides kvs, FaStrides gkvs, int G) {
  static_assert(!KS || (CAUSAL && !HAS_DROP), "kstart: causal, no dropout");
  static_assert(!GQA || (CAUSAL && !HAS_DROP), "GQA: causal, no dropout");
  constexpr int NC = D / 16;
  constexpr int NTO = D / 32;
  constexpr int SWB = fa_swb(D);

  // row images (v3_off): Q and dO are read by rows for St / dPt and
  // transposed for dSt.Q / Pt.dO.  Single-buffered, two barriers per tile:
  // this kernel sits at the 256-VGPR cap, and the registers a prefetched
  // tile needs turn into scratch traffic that costs more than the overlap
  // gains (docs/KERNELS.md, negative results)
  __shared__ __attribute__((aligned(16))) char q_raw[B3_FB * SWB];
  __shared__ __attribute__((aligned(16))) char do_raw[B3_FB * SWB];
  // per-wave exchange of Pt / dSt, held as [q column][kv row] with 64-byte
  // rows: a lane stores its q column's kv runs 8g + 4*hi .. +3 as 8-byte
  // units (unit XOR dkv_xoff: conflict-free stores) and the A operand
  // [kv row][q] comes back through the transposed read
  __shared__ __attribute__((aligned(16))) char p_x[FA_WAVES][32 * 64];
  __shared__ __attribute__((aligned(16))) char ds_x[FA_WAVES][32 * 64];

  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int hi = lane >> 5;
  const int ln = lane & 31;
  // the block's work falls with x: a causal kv block meets the query tiles
  // from its own rows on
  const FlashBlock blk = v3_block(false);
  const unsigned int bx = blk.x, by = blk.y, bz = blk.z;
  // GQA: by is the KV head; the block walks the G query heads
  // qh0 .. qh0 + G - 1 that share it (h stays the number of query heads)
  const unsigned int qh0 = GQA ? by * G : by;
  const long bh = (long)bz * h + qh0;
  const long qoff = bz * qs.b + qh0 * qs.h;
  const bf16_t* Qp = Q + qoff;
  const long kvoff = GQA ? bz * kvs.b + by * kvs.h : qoff;
  const long kv_r = GQA ? kvs.r : qs.r;
  const bf16_t* Kp = K + kvoff;
  const bf16_t* Vp = V + kvoff;
  const bf16_t* dOp = dO + bz * dos.b + qh0 * dos.h;
  const long goff = GQA ? bz * gkvs.b + by * gkvs.h
                        : bz * gs.b + by * gs.h;
  const long g_r = GQA ? gkvs.r : gs.r;
  bf16_t* dKp = dK + goff;
  bf16_t* dVp = dV + goff;
  const float* lse = LSE + bh * s;
  const float* dlt = Delta + bh * s;

  const int klen = CAUSAL ? s : min(klens ? klens[bz] : s, s);
  const int kv0_blk = bx * V3_QBLK;
  const int kv0w = kv0_blk + wave * 32;
  const bool kv_active = kv0w < s;
  const int kv0c = kv_active ? kv0w : s - 32;
  const int my_kv = kv0c + ln;

  // dv/dk in the 32x32 layout: NTO d-tiles x 16 f32 each
  f32x16 dv_acc[NTO], dk_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      dv_acc[t][r] = 0.f;
      dk_acc[t][r] = 0.f;
    }
  }

  const int first_qt = CAUSAL ? kv0_blk / B3_FB : 0;
  int n_q_tiles = s / B3_FB;
  const int* ksb = nullptr;
  if (KS) {
    ksb = kstart + (long)bz * s;
    const int nt = s / V3_KVBLK;
    const int* qe = qend + (long)bz * nt;
    int e = 0;
#pragma unroll
    for (int j = 0; j < V3_QBLK / V3_KVBLK; ++j)
      e = max(e, qe[min(kv0_blk / V3_KVBLK + j, nt - 1)]);
    n_q_tiles = min(max(e, kv0_blk), s - 1) / B3_FB + 1;
  }

  // staging: one 16-byte chunk of Q and of dO per thread (B3_FB * D / 8
  // <= 512 chunks)
  const int st_i = threadIdx.x * 8;
  const bool st_on = st_i < B3_FB * D;
  const int st_r = st_on ? st_i / D : 0;
  const int st_c = st_on ? st_i % D : 0;
  const int st_off = v3_off<SWB>(st_r, st_c >> 3);
  // transposed-read base (v3_tr_bfrag) and row-read base: chunk 2c + hi of
  // row ln is the base with byte bits 5.. flipped by c
  const int qd_tr = v3_tr_addr<SWB>(lane, 8 * hi, 0);
  const int qd_row = v3_off<SWB>(ln, hi);
  // exchange image: rows q 8*hi (+4) + (i>>2), kv columns = this lane's ln
  int x_tr[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    const int i = lane & 15;
    const int row = 8 * hi + 4 * e + (i >> 2);
    x_tr[e] = dkv_xoff(row, 4 * ((lane >> 4) & 1) + (i & 3));
  }
  // the wave's own K and V rows as A fragments, loaded once: they do not
  // change from tile to tile.  (The compiler used to hoist these loads out
  // of the loop by itself; anything that keeps it from doing so, such as a
  // branch around them, leaves 16 loads of 32 B per row in every tile of
  // every wave and makes the kernel L2-bound, 1.5x slower.)
  bf16x8 k_frag[NC], v_frag[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    k_frag[c] = *reinterpret_cast<const bf16x8*>(
        Kp + (long)my_kv * kv_r + c * 16 + hi * 8);
    v_frag[c] = *reinterpret_cast<const bf16x8*>(
        Vp + (long)my_kv * kv_r + c * 16 + hi * 8);
  }

  // GQA: one pass over the query tiles per query head of the group, all
  // into the same fp32 dk_acc / dv_acc (one rounding at the end, one owner
  // per dK/dV row).  kstart / qend are per batch row, so the bounds hold
  // for every member.  The group loop is folded into the tile loop (its
  // last tile rewinds qt and steps the per-head bases), so the plain
  // instantiations keep the single loop, and the code, they had before.
  int gm = 0;
  for (int qt = first_qt; qt < n_q_tiles; ++qt) {
    const int q_base = qt * B3_FB;
    __syncthreads();
    {
      const long qrg = q_base + st_r;
      const bf16x8 qq =
          *reinterpret_cast<const bf16x8*>(Qp + qrg * qs.r + st_c);
      const bf16x8 dd =
          *reinterpret_cast<const bf16x8*>(dOp + qrg * dos.r + st_c);
      if (st_on) {
        *reinterpret_cast<bf16x8*>(q_raw + st_off) = qq;
        *reinterpret_cast<bf16x8*>(do_raw + st_off) = dd;
      }
    }
    const int qcol = q_base + ln;
    const float lse_c = lse[qcol];
    const float dlt_c = dlt[qcol];
    int ks_c = 0;
    if (KS) ks_c = v3_kstart_at(ksb, qcol);
    __syncthreads();

    // St = K Q^T (raw K; scale folded into the exp below)
    f32x16 st, dpt;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8 qb = *reinterpret_cast<const bf16x8*>(
          q_raw + (qd_row ^ (32 * c)));
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_frag[c], qb, st, 0, 0,
                                                   0);
    }
    // dPt = V dO^T
#pragma unroll
    for (int r = 0; r < 16; ++r) dpt[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      bf16x8 db = *reinterpret_cast<const bf16x8*>(
          do_raw + (qd_row ^ (32 * c)));
      dpt = __builtin_amdgcn_mfma_f32_32x32x16_bf16(v_frag[c], db, dpt, 0, 0,
                                                    0);
    }

    // Pt AND dSt by kv row, one exchange pass: st/dpt registers die
    // here (keeping them through the dV MFMAs spilled 128 B/lane)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      short pk[4] __attribute__((aligned(8)));
      short dk4[4] __attribute__((aligned(8)));
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = g * 4 + j;
        const int kvrow = kv0c + (r & 3) + 8 * (r >> 2) + 4 * hi;
        const bool masked = CAUSAL ? (qcol < kvrow || (KS && kvrow < ks_c))
                                   : (kvrow >= klen);
        float pv = masked ? 0.f : __expf(st[r] * scale - lse_c);
        float dm = 1.f;
        if (HAS_DROP && drop_thresh) {
          const unsigned long long idx =
              (bh * (unsigned long long)s + qcol) *
                  (unsigned long long)s + kvrow;
          dm = (fa_hash(drop_seed, idx) < drop_thresh) ? 0.f : keep_scale;
        }
        pk[j] = fa_bf16bits(pv * dm);  // dropped P -> dV
        dk4[j] = fa_bf16bits(pv * (dm * dpt[r] - dlt_c) * scale);  // -> dK
      }
      const int xo = dkv_xoff(ln, 2 * g + hi);
      *reinterpret_cast<long*>(p_x[wave] + xo) =
          *reinterpret_cast<const long*>(pk);
      *reinterpret_cast<long*>(ds_x[wave] + xo) =
          *reinterpret_cast<const long*>(dk4);
    }
    v3_wait_lds();

    // dV += Pt dO : A = Pt [32kv x 16q-chunk], B = dO, both transposed
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      bf16x8 pa = v3_tr_frag(p_x[wave] + c2 * 16 * 64 + x_tr[0],
                             p_x[wave] + c2 * 16 * 64 + x_tr[1]);
      const char* drows = do_raw + c2 * 16 * SWB;
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
        bf16x8 bfrag = v3_tr_bfrag<SWB>(drows, qd_tr, t);
        dv_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            pa, bfrag, dv_acc[t], 0, 0, 0);
      }
    }

    // dK += dSt Q (dSt already exchanged above)
#pragma unroll
    for (int c2 = 0; c2 < 2; ++c2) {
      bf16x8 pa = v3_tr_frag(ds_x[wave] + c2 * 16 * 64 + x_tr[0],
                             ds_x[wave] + c2 * 16 * 64 + x_tr[1]);
      const char* qrows = q_raw + c2 * 16 * SWB;
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
        bf16x8 bfrag = v3_tr_bfrag<SWB>(qrows, qd_tr, t);
        dk_acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            pa, bfrag, dk_acc[t], 0, 0, 0);
      }
    }
    if (GQA && qt + 1 == n_q_tiles && ++gm < G) {
      // next query head of the group
      qt = first_qt - 1;
      Qp += qs.h;
      dOp += dos.h;
      lse += s;
      dlt += s;
    }
  }

  if (!kv_active) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int kvrow = kv0w + (r & 3) + 8 * (r >> 2) + 4 * hi;
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      dKp[(long)kvrow * g_r + t * 32 + ln] = __float2bfloat16(dk_acc[t][r]);
      dVp[(long)kvrow * g_r + t * 32 + ln] = __float2bfloat16(dv_acc[t][r]);
    }
  }
}

template <int D, bool CAUSAL, bool HAS_DROP, bool KS = false>
static void launch_bwd_v3(const void* q, const void* k, const void* v,
                          const void* o, const void* dout, const float* lse,
                          void* dq, void* dk, void* dv, float* delta_ws,
                          const int* klens, FaStrides qs, FaStrides os,
                          FaStrides dos, FaStrides gs, int b, int h, int s,
                          float scale, unsigned int dth, float ksc,
                          unsigned long long seed, hipStream_t stream,
                          const int* kstart = nullptr,
                          const int* qend = nullptr) {
  {
    // at most 16 x-blocks per (batch, head): plenty of blocks to fill the
    // chip while each wave still streams several rows
    int bx = (s + 31) / 32;
    if (bx > 16) bx = 16;
    hipLaunchKernelGGL((flash_delta_v3_kernel<D>), dim3(bx, h, b), dim3(256),
                       0, stream, (const bf16_t*)dout, (const bf16_t*)o,
                       delta_ws, dos, os, h, s);
  }
  dim3 grid((s + V3_QBLK - 1) / V3_QBLK, h, b);
  dim3 block(FA_WAVES * 64);
  hipLaunchKernelGGL((flash_attn_bwd_dq_v3_kernel<D, CAUSAL, HAS_DROP, KS>),
                     grid, block, 0, stream, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout,
                     lse, delta_ws, (bf16_t*)dq, klens, qs, dos, gs, b, h, s,
                     scale, dth, ksc, seed, kstart, FaStrides{}, 1);
  hipLaunchKernelGGL((flash_attn_bwd_dkv_v3_kernel<D, CAUSAL, HAS_DROP, KS>),
                     grid, block, 0, stream, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout,
                     lse, delta_ws, (bf16_t*)dk, (bf16_t*)dv, klens, qs, dos,
                     gs, b, h, s, scale, dth, ksc, seed, kstart, qend,
                     FaStrides{}, FaStrides{}, 1);
}

// Grouped-query backward: delta and dq run per query head (grid y = h), dkv
// per KV head (grid y = h_kv) with the group loop inside the block.
template <int D, bool KS>
static void launch_bwd_v3_gqa(const void* q, const void* k, const void* v,
                              const void* o, const void* dout,
                              const float* lse, void* dq, void* dk, void* dv,
                              float* delta_ws, FaStrides qs, FaStrides kvs,
                              FaStrides os, FaStrides dos, FaStrides gs,
                              FaStrides gkvs, int b, int h, int h_kv, int s,
                              float scale, hipStream_t stream,
                              const int* kstart, const int* qend) {
  int bx = (s + 31) / 32;
  if (bx > 16) bx = 16;
  hipLaunchKernelGGL((flash_delta_v3_kernel<D>), dim3(bx, h, b), dim3(256),
                     0, stream, (const bf16_t*)dout, (const bf16_t*)o,
                     delta_ws, dos, os, h, s);
  const int G = h / h_kv;
  const int nx = (s + V3_QBLK - 1) / V3_QBLK;
  dim3 block(FA_WAVES * 64);
  hipLaunchKernelGGL(
      (flash_attn_bwd_dq_v3_kernel<D, true, false, KS, true>), dim3(nx, h, b),
      block, 0, stream, (const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v,
      (const bf16_t*)dout, lse, delta_ws, (bf16_t*)dq, (const int*)nullptr,
      qs, dos, gs, b, h, s, scale, 0u, 1.f, 0ull, kstart, kvs, G);
  hipLaunchKernelGGL(
      (flash_attn_bwd_dkv_v3_kernel<D, true, false, KS, true>),
      dim3(nx, h_kv, b), block, 0, stream, (const bf16_t*)q, (const bf16_t*)k,
      (const bf16_t*)v, (const bf16_t*)dout, lse, delta_ws, (bf16_t*)dk,
      (bf16_t*)dv, (const int*)nullptr, qs, dos, gs, b, h, s, scale, 0u, 1.f,
      0ull, kstart, qend, kvs, gkvs, G);
}

// qs3: q|k|v, os3: o, dos3: dout, gs3: dq|dk|dv (batch, head, row) strides.
extern "C" void fs_flash_attn_bwd_v3_strided(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, void* dq, void* dk, void* dv,
    float* delta_ws, const int* klens, const long* qs3, const long* os3,
    const long* dos3, const long* gs3, int b, int h, int s, int d,
    int causal, float scale, float drop_p, unsigned long long seed,
    hipStream_t stream) {
  const FaStrides qs{qs3[0], qs3[1], qs3[2]};
  const FaStrides os{os3[0], os3[1], os3[2]};
  const FaStrides dos{dos3[0], dos3[1], dos3[2]};
  const FaStrides gs{gs3[0], gs3[1], gs3[2]};
  const unsigned int dth =
      (drop_p > 0.f) ? (unsigned int)(drop_p * 4294967296.0) : 0u;
  const float ksc = (drop_p > 0.f) ? 1.f / (1.f - drop_p) : 1.f;
#define BWD3(DD, CC, DR) launch_bwd_v3<DD, CC, DR>( \
      q, k, v, o, dout, lse, dq, dk, dv, delta_ws, klens, qs, os, dos, gs, \
      b, h, s, scale, dth, ksc, seed, stream)
  if (dth) {
    if (d == 128 && causal) BWD3(128, true, true);
    else if (d == 128) BWD3(128, false, true);
    else if (d == 96 && causal) BWD3(96, true, true);
    else if (d == 96) BWD3(96, false, true);
    else if (d == 64 && causal) BWD3(64, true, true);
    else BWD3(64, false, true);
  } else {
    if (d == 128 && causal) BWD3(128, true, false);
    else if (d == 128) BWD3(128, false, false);
    else if (d == 96 && causal) BWD3(96, true, false);
    else if (d == 96) BWD3(96, false, false);
    else if (d == 64 && causal) BWD3(64, true, false);
    else BWD3(64, false, false);
  }
#undef BWD3
}

// Causal backward with a per-row key start; qend [b, s/64] int32 is the
// query-loop bound of dkv (see flash_attn_bwd_dkv_v3_kernel).  delta does
// not depend on the mask, so flash_delta_v3_kernel serves both.
extern "C" void fs_flash_attn_bwd_v3_kstart(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, void* dq, void* dk, void* dv,
    float* delta_ws, const int* kstart, const int* qend, const long* qs3,
    const long* os3, const long* dos3, const long* gs3, int b, int h, int s,
    int d, float scale, hipStream_t stream) {
  const FaStrides qs{qs3[0], qs3[1], qs3[2]};
  const FaStrides os{os3[0], os3[1], os3[2]};
  const FaStrides dos{dos3[0], dos3[1], dos3[2]};
  const FaStrides gs{gs3[0], gs3[1], gs3[2]};
#define BWD3K(DD) launch_bwd_v3<DD, true, false, true>( \
      q, k, v, o, dout, lse, dq, dk, dv, delta_ws, nullptr, qs, os, dos, gs, \
      b, h, s, scale, 0u, 1.f, 0ull, stream, kstart, qend)
  if (d == 128) BWD3K(128);
  else if (d == 96) BWD3K(96);
  else BWD3K(64);
#undef BWD3K
}

// kvs3: k|v, gkvs3: dk|dv strides; kstart / qend both null or both set.
extern "C" void fs_flash_attn_bwd_v3_gqa(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, void* dq, void* dk, void* dv,
    float* delta_ws, const int* kstart, const int* qend, const long* qs3,
    const long* kvs3, const long* os3, const long* dos3, const long* gs3,
    const long* gkvs3, int b, int h, int h_kv, int s, int d, float scale,
    hipStream_t stream) {
  const FaStrides qs{qs3[0], qs3[1], qs3[2]};
  const FaStrides kvs{kvs3[0], kvs3[1], kvs3[2]};
  const FaStrides os{os3[0], os3[1], os3[2]};
  const FaStrides dos{dos3[0], dos3[1], dos3[2]};
  const FaStrides gs{gs3[0], gs3[1], gs3[2]};
  const FaStrides gkvs{gkvs3[0], gkvs3[1], gkvs3[2]};
#define BWD3G(DD, KK) launch_bwd_v3_gqa<DD, KK>( \
      q, k, v, o, dout, lse, dq, dk, dv, delta_ws, qs, kvs, os, dos, gs, \
      gkvs, b, h, h_kv, s, scale, stream, kstart, qend)
  if (kstart) {
    if (d == 128) BWD3G(128, true);
    else if (d == 96) BWD3G(96, true);
    else BWD3G(64, true);
  } else {
    if (d == 128) BWD3G(128, false);
    else if (d == 96) BWD3G(96, false);
    else BWD3G(64, false);
  }
#undef BWD3G
}

extern "C" void fs_flash_attn_bwd_v3(const void* q, const void* k,
                                     const void* v, const void* o,
                                     const void* dout, const float* lse,
                                     void* dq, void* dk, void* dv,
                                     float* delta_ws, const int* klens,
                                     int b, int h, int s, int d, int causal,
                                     float scale, float drop_p,
                                     unsigned long long seed,
                                     hipStream_t stream) {
  const long c3[3] = {(long)h * s * d, (long)s * d, (long)d};
  fs_flash_attn_bwd_v3_strided(q, k, v, o, dout, lse, dq, dk, dv, delta_ws,
                               klens, c3, c3, c3, c3, b, h, s, d, causal,
                               scale, drop_p, seed, stream);
}
