// Host interface of the flash v3 kernels (flash_attn.hip): one argument
// struct and two launchers for every variant -- plain, dropout, klens, per-row
// key start (kstart), grouped-query K/V.  bindings.cpp fills the struct from
// checked tensors; the launchers pick the kernel instantiation from it.
#pragma once

#include <hip/hip_runtime.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct FlashV3Args {
  // Operands: logical [b, h, s, d] bf16 (k, v, dk, dv: [b, h_kv, s, d]),
  // lse and delta_ws contiguous fp32 [b, h, s].  Forward writes o and lse;
  // backward reads them with dout and writes dq, dk, dv (delta_ws is its
  // scratch).  Forward leaves the backward-only pointers null.
  const void *q, *k, *v;
  void* o;
  const void* dout;
  float* lse;
  void *dq, *dk, *dv;
  float* delta_ws;
  // Masks, each may be null: klens int32 [b] (bidirectional only), kstart
  // int32 [b, s] (causal only, no dropout), qend int32 [b, s/64] (backward
  // with kstart).
  const int *klens, *kstart, *qend;
  // (batch, head, row) element strides, last dim unit-stride: qs of q (and
  // of k, v when h_kv == h), kvs of k and v, os of o, dos of dout, gs of dq
  // (and of dk, dv when h_kv == h), gkvs of dk and dv.  kvs and gkvs are
  // read only when h_kv != h.
  long qs[3], kvs[3], os[3], dos[3], gs[3], gkvs[3];
  int b, h, h_kv, s, d;  // d in {64, 96, 128}, s % 64 == 0, h % h_kv == 0
  int causal;            // h_kv != h or kstart: causal only, no dropout
  float scale, drop_p;
  unsigned long long seed;
} FlashV3Args;

void fs_flash_v3_fwd(const FlashV3Args* a, hipStream_t stream);
void fs_flash_v3_bwd(const FlashV3Args* a, hipStream_t stream);

#ifdef __cplusplus
}
#endif
