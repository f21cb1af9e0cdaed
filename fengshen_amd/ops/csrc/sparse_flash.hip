// Block-sparse flash attention (fwd + FA2-style bwd) for MI355X (gfx950).
//
// Same building blocks as the general kernels in flash_attn.hip: a wave owns
// 16 query rows, S and PV run on v_mfma_f32_16x16x32_bf16, K rows are staged
// XOR-swizzled, V / K^T / Q^T / dO^T transposed with the kv-index swizzle,
// and P reaches the second GEMM through a per-wave LDS tile.  What is new is
// that a block does not sweep the key axis: it walks a tile list.
//
// Metadata (built on the host by ops/sparse_flash.py, one set per
// (layout, seq_len)); LH = h, or 1 when all heads share one layout:
//   row lists  row_ptr[LH * nqt + 1], row_idx[nnz], row_mask[nnz]
//       for (head, 128-row query tile): the 64-key tiles with at least one
//       active 16x16 sub-block.  Mask bit 4*w + n: the 16 rows of wave w see
//       the n-th group of 16 keys of that tile.
//   col lists  col_ptr[LH * nkt + 1], col_idx[nnz], col_mask[nnz]
//       the transpose: for (head, 64-key tile) the query tiles that see it,
//       same bits.
// Forward and dQ walk the row lists, dK/dV the column lists, so every output
// row is owned by exactly one wave: no atomics, bit-reproducible gradients.
//
// Masking is by select: an inactive sub-block, a causal position
// (kcol > qrow), a masked key (key_mask[b, kcol] == 0) and a column >= s all
// give P = 0 without evaluating exp on a masked score.  A query row that
// sees no key gets O = 0, LSE = 0 and contributes nothing to any gradient.

#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int SF_QBLK = 128;   // 8 waves x 16 q rows
constexpr int SF_KVBLK = 64;   // key tile of the lists
constexpr int SF_WAVES = 8;
constexpr int SF_PAD = 8;
constexpr int SF_T = 32;       // backward streaming tile
constexpr int SF_KV_WAVES = 4; // dK/dV block: 4 waves x 16 keys = one key tile
// "not visible" score: finite, so the softmax state never holds an inf
// (the extension is built with -ffast-math)
constexpr float SF_NEG = -1e30f;

constexpr int sf_dpad(int d) { return (d + 31) / 32 * 32; }
constexpr int sf_swb(int dp) {
  int need = 2 * dp, p = 128;
  while (p < need) p <<= 1;
  return p;
}

__device__ __forceinline__ int sf_swz(int row, int byte_in_row) {
  return byte_in_row ^ ((row & 7) << 4);
}

__device__ __forceinline__ short sf_bf16bits(float f) {
  return (short)__hip_bfloat16_raw(__float2bfloat16(f)).x;
}

template <int D>
__device__ __forceinline__ bf16x8 sf_load8(const bf16_t* rowp, int d0) {
  if (d0 < D) return *reinterpret_cast<const bf16x8*>(rowp + d0);
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = 0;
  return z;
}

__device__ __forceinline__ bf16x8 sf_scale8(bf16x8 raw, float scale) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned short u = (unsigned short)raw[j];
    float f = __uint_as_float(((unsigned int)u) << 16) * scale;
    raw[j] = sf_bf16bits(f);
  }
  return raw;
}

// First step t in [t, t_end) whose sub-mask is non-zero, else t_end.  A
// list entry is SUB consecutive steps; step t covers entry t / SUB and
// sub-range t % SUB, selected by sub0 << (shift * (t % SUB)).  All operands
// are block-uniform, so every wave takes the same path.
template <int SUB>
__device__ __forceinline__ int sf_next_step(const int* __restrict__ masks,
                                            int t, int t_end,
                                            unsigned int sub0, int shift) {
  while (t < t_end) {
    const unsigned int m = (unsigned int)masks[t / SUB];
    if (m & (sub0 << (shift * (t % SUB)))) break;
    ++t;
  }
  return t;
}

// ===========================================================================
// FORWARD: block = one (batch, head, 128-row query tile), walks its row list
// ===========================================================================
template <int D, bool CAUSAL>
__global__ __launch_bounds__(SF_WAVES * 64)
void sparse_flash_fwd_kernel(const bf16_t* __restrict__ Q,
                             const bf16_t* __restrict__ K,
                             const bf16_t* __restrict__ V,
                             bf16_t* __restrict__ O,
                             float* __restrict__ LSE,
                             const int* __restrict__ row_ptr,
                             const int* __restrict__ row_idx,
                             const int* __restrict__ row_mask,
                             const unsigned char* __restrict__ kmask,
                             int h, int s, int list_heads, float scale) {
  constexpr int DP = sf_dpad(D);
  constexpr int NC = DP / 32;
  constexpr int NTO = DP / 16;
  constexpr int SWB = sf_swb(DP);
  constexpr int NT = SF_WAVES * 64;

  __shared__ char k_raw[SF_KVBLK * SWB];
  __shared__ short vt_lds[DP][SF_KVBLK + SF_PAD];
  __shared__ short p_lds[SF_WAVES][16][SF_KVBLK + SF_PAD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int qb = blockIdx.x;
  const int head = blockIdx.y;
  const int batch = blockIdx.z;
  const long bh = (long)batch * h + head;

  const bf16_t* Qp = Q + bh * s * D;
  const bf16_t* Kp = K + bh * s * D;
  const bf16_t* Vp = V + bh * s * D;
  bf16_t* Op = O + bh * s * D;
  const unsigned char* km = kmask ? kmask + (long)batch * s : nullptr;

  const int lh = (list_heads == 1) ? 0 : head;
  const int lbase = lh * (int)gridDim.x + qb;
  const int beg = row_ptr[lbase];
  const int end = row_ptr[lbase + 1];

  const int q0 = qb * SF_QBLK + wave * 16;
  const bool q_active = q0 < s;           // s % 16 == 0: all 16 rows or none
  const int q0c = q_active ? q0 : s - 16;

  bf16x8 q_frag[NC];
  {
    const int qrow = q0c + (lane & 15);
    const int k0 = (lane >> 4) * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      q_frag[c] = sf_scale8(sf_load8<D>(Qp + (long)qrow * D, c * 32 + k0),
                            scale);
  }

  float m_run[4], l_run[4];
  f32x4 o_acc[NTO];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m_run[r] = SF_NEG;
    l_run[r] = 0.f;
  }
#pragma unroll
  for (int t = 0; t < NTO; ++t) o_acc[t] = f32x4{0, 0, 0, 0};

  constexpr int ELEMS = SF_KVBLK * DP;
  constexpr int SWEEPS = (ELEMS + NT * 8 - 1) / (NT * 8);
  bf16x8 k_reg[SWEEPS], v_reg[SWEEPS];

  auto prefetch = [&](int kt) {
    const int k_base = kt * SF_KVBLK;
#pragma unroll
    for (int sw = 0; sw < SWEEPS; ++sw) {
      const int i = tid * 8 + sw * (NT * 8);
      if (i < ELEMS) {
        const int kr = i / DP;
        const int kc = i % DP;
        const long krg = min(k_base + kr, s - 1);
        k_reg[sw] = sf_load8<D>(Kp + krg * D, kc);
        v_reg[sw] = sf_load8<D>(Vp + krg * D, kc);
      }
    }
  };

  int cur = sf_next_step<1>(row_mask, beg, end, 0xffffffffu, 0);
  if (cur < end) prefetch(row_idx[cur]);

  while (cur < end) {
    const int k_base = row_idx[cur] * SF_KVBLK;
    const unsigned int mask = (unsigned int)row_mask[cur];
    __syncthreads();
#pragma unroll
    for (int sw = 0; sw < SWEEPS; ++sw) {
      const int i = tid * 8 + sw * (NT * 8);
      if (i < ELEMS) {
        const int kr = i / DP;
        const int kc = i % DP;
        *reinterpret_cast<bf16x8*>(k_raw + kr * SWB + sf_swz(kr, kc * 2)) =
            k_reg[sw];
        bf16x8 vv = v_reg[sw];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          vt_lds[kc + j][kr ^ ((kc + j) & 0x38)] = vv[j];
      }
    }
    __syncthreads();
    const int nxt = sf_next_step<1>(row_mask, cur + 1, end, 0xffffffffu, 0);
    if (nxt < end) prefetch(row_idx[nxt]);
    cur = nxt;

    // the wave's four sub-block bits; wave-uniform
    const unsigned int wbits = q_active ? ((mask >> (4 * wave)) & 0xfu) : 0u;
    if (wbits == 0u) continue;

    f32x4 s_acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) s_acc[nt] = f32x4{0, 0, 0, 0};
    const int col = lane & 15;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      if (!(wbits & (1u << nt))) continue;
      const int krow = nt * 16 + col;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int d0 = c * 32 + (lane >> 4) * 8;
        bf16x8 bfrag = *reinterpret_cast<const bf16x8*>(
            k_raw + krow * SWB + sf_swz(krow, d0 * 2));
        s_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            q_frag[c], bfrag, s_acc[nt], 0, 0, 0);
      }
    }

    // per-column visibility (sub-block bit, range, key mask)
    bool colvis[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int kcol = k_base + nt * 16 + col;
      bool vis = (wbits & (1u << nt)) && kcol < s;
      if (vis && km) vis = km[kcol] != 0;
      colvis[nt] = vis;
    }

    float p[4][4];
    float tile_max[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0c + (lane >> 4) * 4 + r;
      float tm = SF_NEG;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const int kcol = k_base + nt * 16 + col;
        bool vis = colvis[nt];
        if (CAUSAL) vis = vis && (kcol <= qrow);
        const float v = vis ? s_acc[nt][r] : SF_NEG;
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
      alpha[r] = (m_run[r] == SF_NEG) ? 0.f : __expf(m_run[r] - m_new);
      if (m_new != m_run[r]) need_rescale = true;
      m_run[r] = m_new;
      float ps = 0.f;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        const float e =
            (p[nt][r] == SF_NEG) ? 0.f : __expf(p[nt][r] - m_new);
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
    for (int r = 0; r < 4; ++r) l_run[r] = l_run[r] * alpha[r] + rowsum[r];
    if (__any(need_rescale)) {
#pragma unroll
      for (int t = 0; t < NTO; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) o_acc[t][r] *= alpha[r];
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        p_lds[wave][row][nt * 16 + col] = sf_bf16bits(p[nt][r]);
    }
    __builtin_amdgcn_s_waitcnt(0);  // wave-local LDS visibility

#pragma unroll
    for (int kc = 0; kc < 2; ++kc) {
      if (!(wbits & (3u << (2 * kc)))) continue;  // both sub-blocks are P = 0
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

  if (!q_active) return;
  const int col = lane & 15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0 + (lane >> 4) * 4 + r;
    const bool seen = l_run[r] > 0.f;
    const float inv_l = seen ? 1.f / l_run[r] : 0.f;
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      const int d = t * 16 + col;
      if (d < D) Op[(long)qrow * D + d] = __float2bfloat16(o_acc[t][r] * inv_l);
    }
    if (col == 0)
      LSE[bh * s + qrow] = seen ? m_run[r] + logf(l_run[r]) : 0.f;
  }
}

// ===========================================================================
// BACKWARD
// ===========================================================================
template <int D>
__global__ __launch_bounds__(256)
void sparse_flash_delta_kernel(const bf16_t* __restrict__ dO,
                               const bf16_t* __restrict__ O,
                               float* __restrict__ delta, long rows) {
  const int lane = threadIdx.x & 63;
  const int wid = threadIdx.x >> 6;
  const long stride = (long)gridDim.x * 4;
  for (long row = (long)blockIdx.x * 4 + wid; row < rows; row += stride) {
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

// dQ, q-major over the row lists.  A 64-key list entry is streamed as two
// 32-key halves; a half in which no wave has a bit is not staged at all.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(SF_WAVES * 64)
void sparse_flash_bwd_dq_kernel(const bf16_t* __restrict__ Q,
                                const bf16_t* __restrict__ K,
                                const bf16_t* __restrict__ V,
                                const bf16_t* __restrict__ dO,
                                const float* __restrict__ LSE,
                                const float* __restrict__ Delta,
                                bf16_t* __restrict__ dQ,
                                const int* __restrict__ row_ptr,
                                const int* __restrict__ row_idx,
                                const int* __restrict__ row_mask,
                                const unsigned char* __restrict__ kmask,
                                int h, int s, int list_heads, float scale) {
  constexpr int DP = sf_dpad(D);
  constexpr int NC = DP / 32;
  constexpr int NTO = DP / 16;
  constexpr int SWB = sf_swb(DP);
  constexpr int NT = SF_WAVES * 64;

  __shared__ char k_raw[SF_T * SWB];
  __shared__ char v_raw[SF_T * SWB];
  __shared__ short kt_lds[DP][SF_T + SF_PAD];
  __shared__ short p_lds[SF_WAVES][16][SF_T + SF_PAD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int head = blockIdx.y;
  const int batch = blockIdx.z;
  const long bh = (long)batch * h + head;
  const bf16_t* Qp = Q + bh * s * D;
  const bf16_t* Kp = K + bh * s * D;
  const bf16_t* Vp = V + bh * s * D;
  const bf16_t* dOp = dO + bh * s * D;
  bf16_t* dQp = dQ + bh * s * D;
  const float* lse = LSE + bh * s;
  const float* dlt = Delta + bh * s;
  const unsigned char* km = kmask ? kmask + (long)batch * s : nullptr;

  const int lh = (list_heads == 1) ? 0 : head;
  const int lbase = lh * (int)gridDim.x + blockIdx.x;
  const int beg = row_ptr[lbase];
  const int end = row_ptr[lbase + 1];

  const int q0 = blockIdx.x * SF_QBLK + wave * 16;
  const bool q_active = q0 < s;
  const int q0c = q_active ? q0 : s - 16;

  bf16x8 q_frag[NC], do_frag[NC];
  {
    const int qrow = q0c + (lane & 15);
    const int k0 = (lane >> 4) * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      q_frag[c] = sf_scale8(sf_load8<D>(Qp + (long)qrow * D, c * 32 + k0),
                            scale);
      do_frag[c] = sf_load8<D>(dOp + (long)qrow * D, c * 32 + k0);
    }
  }
  float lse_r[4], dlt_r[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int qrow = q0c + (lane >> 4) * 4 + r;
    lse_r[r] = lse[qrow];
    dlt_r[r] = dlt[qrow];
  }

  f32x4 dq_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) dq_acc[t] = f32x4{0, 0, 0, 0};

  constexpr int BELEMS = SF_T * DP;
  constexpr int BSWEEPS = (BELEMS + NT * 8 - 1) / (NT * 8);
  bf16x8 kst[BSWEEPS], vst[BSWEEPS];

  // step t: entry t/2, key half t%2 (bits n = 2*half, 2*half+1 of each wave)
  auto prefetch = [&](int t) {
    const int k_base = row_idx[t >> 1] * SF_KVBLK + (t & 1) * SF_T;
#pragma unroll
    for (int sw = 0; sw < BSWEEPS; ++sw) {
      const int i = tid * 8 + sw * (NT * 8);
      if (i < BELEMS) {
        const int kr = i / DP;
        const int kc = i % DP;
        const long krg = min(k_base + kr, s - 1);
        kst[sw] = sf_load8<D>(Kp + krg * D, kc);
        vst[sw] = sf_load8<D>(Vp + krg * D, kc);
      }
    }
  };

  const int t_end = end * 2;
  int cur = sf_next_step<2>(row_mask, beg * 2, t_end, 0x33333333u, 2);
  if (cur < t_end) prefetch(cur);

  while (cur < t_end) {
    const int half = cur & 1;
    const int k_base = row_idx[cur >> 1] * SF_KVBLK + half * SF_T;
    const unsigned int mask = (unsigned int)row_mask[cur >> 1];
    __syncthreads();
#pragma unroll
    for (int sw = 0; sw < BSWEEPS; ++sw) {
      const int i = tid * 8 + sw * (NT * 8);
      if (i < BELEMS) {
        const int kr = i / DP;
        const int kc = i % DP;
        bf16x8 kk = kst[sw];
        *reinterpret_cast<bf16x8*>(k_raw + kr * SWB + sf_swz(kr, kc * 2)) = kk;
        *reinterpret_cast<bf16x8*>(v_raw + kr * SWB + sf_swz(kr, kc * 2)) =
            vst[sw];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          kt_lds[kc + j][kr ^ ((kc + j) & 0x18)] = kk[j];
      }
    }
    __syncthreads();
    const int nxt = sf_next_step<2>(row_mask, cur + 1, t_end, 0x33333333u, 2);
    if (nxt < t_end) prefetch(nxt);
    cur = nxt;

    const unsigned int wbits =
        q_active ? ((mask >> (4 * wave + 2 * half)) & 0x3u) : 0u;
    if (wbits == 0u) continue;

    f32x4 s_acc[2], dp_acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      s_acc[nt] = f32x4{0, 0, 0, 0};
      dp_acc[nt] = f32x4{0, 0, 0, 0};
    }
    const int col = lane & 15;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      if (!(wbits & (1u << nt))) continue;
      const int krow = nt * 16 + col;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int d0 = c * 32 + (lane >> 4) * 8;
        bf16x8 kb = *reinterpret_cast<const bf16x8*>(
            k_raw + krow * SWB + sf_swz(krow, d0 * 2));
        s_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            q_frag[c], kb, s_acc[nt], 0, 0, 0);
        bf16x8 vb = *reinterpret_cast<const bf16x8*>(
            v_raw + krow * SWB + sf_swz(krow, d0 * 2));
        dp_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            do_frag[c], vb, dp_acc[nt], 0, 0, 0);
      }
    }

    bool colvis[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int kcol = k_base + nt * 16 + col;
      bool vis = (wbits & (1u << nt)) && kcol < s;
      if (vis && km) vis = km[kcol] != 0;
      colvis[nt] = vis;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int qrow = q0c + (lane >> 4) * 4 + r;
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) {
        const int kcol = k_base + nt * 16 + col;
        bool vis = colvis[nt];
        if (CAUSAL) vis = vis && (kcol <= qrow);
        const float pv = vis ? __expf(s_acc[nt][r] - lse_r[r]) : 0.f;
        const float ds = pv * (dp_acc[nt][r] - dlt_r[r]) * scale;
        p_lds[wave][row][nt * 16 + col] = sf_bf16bits(ds);
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
#pragma unroll
    for (int t = 0; t < NTO; ++t) {
      const int d = t * 16 + col;
      if (d < D) dQp[(long)qrow * D + d] = __float2bfloat16(dq_acc[t][r]);
    }
  }
}

// dK/dV, kv-major over the column lists.  Block = one 64-key tile, wave n
// owns key group n (16 keys).  A 128-row list entry is streamed as four
// 32-row chunks; chunk c holds the rows of query waves 2c and 2c+1, so wave
// n's sub-block nt of the chunk is mask bit 4*(2c+nt) + n.
template <int D, bool CAUSAL>
__global__ __launch_bounds__(SF_KV_WAVES * 64)
void sparse_flash_bwd_dkv_kernel(const bf16_t* __restrict__ Q,
                                 const bf16_t* __restrict__ K,
                                 const bf16_t* __restrict__ V,
                                 const bf16_t* __restrict__ dO,
                                 const float* __restrict__ LSE,
                                 const float* __restrict__ Delta,
                                 bf16_t* __restrict__ dK,
                                 bf16_t* __restrict__ dV,
                                 const int* __restrict__ col_ptr,
                                 const int* __restrict__ col_idx,
                                 const int* __restrict__ col_mask,
                                 const unsigned char* __restrict__ kmask,
                                 int h, int s, int list_heads, float scale) {
  constexpr int DP = sf_dpad(D);
  constexpr int NC = DP / 32;
  constexpr int NTO = DP / 16;
  constexpr int SWB = sf_swb(DP);
  constexpr int NT = SF_KV_WAVES * 64;

  __shared__ char q_raw[SF_T * SWB];
  __shared__ char do_raw[SF_T * SWB];
  __shared__ short qt_lds[DP][SF_T + SF_PAD];
  __shared__ short dot_lds[DP][SF_T + SF_PAD];
  __shared__ short p_lds[SF_KV_WAVES][16][SF_T + SF_PAD];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int head = blockIdx.y;
  const int batch = blockIdx.z;
  const long bh = (long)batch * h + head;
  const bf16_t* Qp = Q + bh * s * D;
  const bf16_t* Kp = K + bh * s * D;
  const bf16_t* Vp = V + bh * s * D;
  const bf16_t* dOp = dO + bh * s * D;
  bf16_t* dKp = dK + bh * s * D;
  bf16_t* dVp = dV + bh * s * D;
  const float* lse = LSE + bh * s;
  const float* dlt = Delta + bh * s;

  const int lh = (list_heads == 1) ? 0 : head;
  const int lbase = lh * (int)gridDim.x + blockIdx.x;
  const int beg = col_ptr[lbase];
  const int end = col_ptr[lbase + 1];

  const int kv0 = blockIdx.x * SF_KVBLK + wave * 16;
  const bool kv_active = kv0 < s;
  const int kv0c = kv_active ? kv0 : s - 16;

  bf16x8 k_frag[NC], v_frag[NC];
  {
    const int kvrow = kv0c + (lane & 15);
    const int c0 = (lane >> 4) * 8;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      k_frag[c] = sf_scale8(sf_load8<D>(Kp + (long)kvrow * D, c * 32 + c0),
                            scale);
      v_frag[c] = sf_load8<D>(Vp + (long)kvrow * D, c * 32 + c0);
    }
  }
  // key mask of the four key rows this lane accumulates
  bool rowkeep[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int kvrow = kv0c + (lane >> 4) * 4 + r;
    rowkeep[r] = kmask ? kmask[(long)batch * s + kvrow] != 0 : true;
  }

  f32x4 dv_acc[NTO], dk_acc[NTO];
#pragma unroll
  for (int t = 0; t < NTO; ++t) {
    dv_acc[t] = f32x4{0, 0, 0, 0};
    dk_acc[t] = f32x4{0, 0, 0, 0};
  }

  constexpr int BELEMS = SF_T * DP;
  constexpr int BSWEEPS = (BELEMS + NT * 8 - 1) / (NT * 8);
  bf16x8 qst[BSWEEPS], dst[BSWEEPS];

  auto prefetch = [&](int t) {
    const int q_base = col_idx[t >> 2] * SF_QBLK + (t & 3) * SF_T;
#pragma unroll
    for (int sw = 0; sw < BSWEEPS; ++sw) {
      const int i = tid * 8 + sw * (NT * 8);
      if (i < BELEMS) {
        const int qr = i / DP;
        const int qc = i % DP;
        const long qrg = min(q_base + qr, s - 1);
        qst[sw] = sf_load8<D>(Qp + qrg * D, qc);
        dst[sw] = sf_load8<D>(dOp + qrg * D, qc);
      }
    }
  };

  const int t_end = end * 4;
  int cur = sf_next_step<4>(col_mask, beg * 4, t_end, 0xffu, 8);
  if (cur < t_end) prefetch(cur);

  while (cur < t_end) {
    const int chunk = cur & 3;
    const int q_base = col_idx[cur >> 2] * SF_QBLK + chunk * SF_T;
    const unsigned int mask = (unsigned int)col_mask[cur >> 2];
    __syncthreads();
#pragma unroll
    for (int sw = 0; sw < BSWEEPS; ++sw) {
      const int i = tid * 8 + sw * (NT * 8);
      if (i < BELEMS) {
        const int qr = i / DP;
        const int qc = i % DP;
        bf16x8 qq = qst[sw];
        bf16x8 dd = dst[sw];
        *reinterpret_cast<bf16x8*>(q_raw + qr * SWB + sf_swz(qr, qc * 2)) = qq;
        *reinterpret_cast<bf16x8*>(do_raw + qr * SWB + sf_swz(qr, qc * 2)) =
            dd;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          qt_lds[qc + j][qr ^ ((qc + j) & 0x18)] = qq[j];
          dot_lds[qc + j][qr ^ ((qc + j) & 0x18)] = dd[j];
        }
      }
    }
    __syncthreads();
    const int nxt = sf_next_step<4>(col_mask, cur + 1, t_end, 0xffu, 8);
    if (nxt < t_end) prefetch(nxt);
    cur = nxt;

    // bit nt: the wave's keys are seen by query wave 2*chunk + nt
    const unsigned int wbits =
        kv_active ? (((mask >> (8 * chunk + wave)) & 1u) |
                     (((mask >> (8 * chunk + 4 + wave)) & 1u) << 1))
                  : 0u;
    if (wbits == 0u) continue;

    f32x4 st_acc[2], dpt_acc[2];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      st_acc[nt] = f32x4{0, 0, 0, 0};
      dpt_acc[nt] = f32x4{0, 0, 0, 0};
    }
    const int col = lane & 15;
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      if (!(wbits & (1u << nt))) continue;
      const int qrow = nt * 16 + col;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int d0 = c * 32 + (lane >> 4) * 8;
        bf16x8 qb = *reinterpret_cast<const bf16x8*>(
            q_raw + qrow * SWB + sf_swz(qrow, d0 * 2));
        st_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            k_frag[c], qb, st_acc[nt], 0, 0, 0);
        bf16x8 db = *reinterpret_cast<const bf16x8*>(
            do_raw + qrow * SWB + sf_swz(qrow, d0 * 2));
        dpt_acc[nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            v_frag[c], db, dpt_acc[nt], 0, 0, 0);
      }
    }

    float pt[2][4];
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      const int qcol = q_base + nt * 16 + col;
      const int qcolc = min(qcol, s - 1);
      const float lse_c = lse[qcolc];
      const float dlt_c = dlt[qcolc];
      const bool colvis = (wbits & (1u << nt)) && qcol < s;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int kvrow = kv0c + (lane >> 4) * 4 + r;
        bool vis = colvis && rowkeep[r];
        if (CAUSAL) vis = vis && (kvrow <= qcol);
        const float pv = vis ? __expf(st_acc[nt][r] - lse_c) : 0.f;
        pt[nt][r] = pv;
        dpt_acc[nt][r] = pv * (dpt_acc[nt][r] - dlt_c) * scale;  // dS^T
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = (lane >> 4) * 4 + r;
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        p_lds[wave][row][nt * 16 + col] = sf_bf16bits(pt[nt][r]);
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
        p_lds[wave][row][nt * 16 + col] = sf_bf16bits(dpt_acc[nt][r]);
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
    const int kvrow = kv0 + (lane >> 4) * 4 + r;
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
template <int D, bool CAUSAL>
void launch_fwd(const void* q, const void* k, const void* v, void* o,
                float* lse, const int* rp, const int* ri, const int* rm,
                const unsigned char* kmask, int b, int h, int s,
                int list_heads, float scale, hipStream_t stream) {
  dim3 grid((s + SF_QBLK - 1) / SF_QBLK, h, b);
  hipLaunchKernelGGL((sparse_flash_fwd_kernel<D, CAUSAL>), grid,
                     dim3(SF_WAVES * 64), 0, stream, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)o, lse, rp,
                     ri, rm, kmask, h, s, list_heads, scale);
}

template <int D, bool CAUSAL>
void launch_bwd(const void* q, const void* k, const void* v, const void* o,
                const void* dout, const float* lse, void* dq, void* dk,
                void* dv, float* delta, const int* rp, const int* ri,
                const int* rm, const int* cp, const int* ci, const int* cm,
                const unsigned char* kmask, int b, int h, int s,
                int list_heads, float scale, hipStream_t stream) {
  const long rows = (long)b * h * s;
  long blocks = (rows + 3) / 4;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL((sparse_flash_delta_kernel<D>), dim3((unsigned)blocks),
                     dim3(256), 0, stream, (const bf16_t*)dout,
                     (const bf16_t*)o, delta, rows);
  dim3 gq((s + SF_QBLK - 1) / SF_QBLK, h, b);
  dim3 gkv((s + SF_KVBLK - 1) / SF_KVBLK, h, b);
  hipLaunchKernelGGL((sparse_flash_bwd_dq_kernel<D, CAUSAL>), gq,
                     dim3(SF_WAVES * 64), 0, stream, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout,
                     lse, delta, (bf16_t*)dq, rp, ri, rm, kmask, h, s,
                     list_heads, scale);
  hipLaunchKernelGGL((sparse_flash_bwd_dkv_kernel<D, CAUSAL>), gkv,
                     dim3(SF_KV_WAVES * 64), 0, stream, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, (const bf16_t*)dout,
                     lse, delta, (bf16_t*)dk, (bf16_t*)dv, cp, ci, cm, kmask,
                     h, s, list_heads, scale);
}

}  // namespace

extern "C" void fs_sparse_flash_fwd(const void* q, const void* k,
                                    const void* v, void* o, float* lse,
                                    const int* rp, const int* ri,
                                    const int* rm,
                                    const unsigned char* kmask, int b, int h,
                                    int s, int d, int list_heads, int causal,
                                    float scale, hipStream_t stream) {
#define SF_FWD(DD)                                                          \
  case DD:                                                                  \
    if (causal)                                                             \
      launch_fwd<DD, true>(q, k, v, o, lse, rp, ri, rm, kmask, b, h, s,     \
                           list_heads, scale, stream);                      \
    else                                                                    \
      launch_fwd<DD, false>(q, k, v, o, lse, rp, ri, rm, kmask, b, h, s,    \
                            list_heads, scale, stream);                     \
    break;
  switch (d) { SF_FWD(64) SF_FWD(96) SF_FWD(128) }
#undef SF_FWD
}

extern "C" void fs_sparse_flash_bwd(
    const void* q, const void* k, const void* v, const void* o,
    const void* dout, const float* lse, void* dq, void* dk, void* dv,
    float* delta, const int* rp, const int* ri, const int* rm, const int* cp,
    const int* ci, const int* cm, const unsigned char* kmask, int b, int h,
    int s, int d, int list_heads, int causal, float scale,
    hipStream_t stream) {
#define SF_BWD(DD)                                                          \
  case DD:                                                                  \
    if (causal)                                                             \
      launch_bwd<DD, true>(q, k, v, o, dout, lse, dq, dk, dv, delta, rp,    \
                           ri, rm, cp, ci, cm, kmask, b, h, s, list_heads,  \
                           scale, stream);                                  \
    else                                                                    \
      launch_bwd<DD, false>(q, k, v, o, dout, lse, dq, dk, dv, delta, rp,   \
                            ri, rm, cp, ci, cm, kmask, b, h, s, list_heads, \
                            scale, stream);                                 \
    break;
  switch (d) { SF_BWD(64) SF_BWD(96) SF_BWD(128) }
#undef SF_BWD
}
