"""Flash attention wrapper: fused HIP forward + fused FA2-style backward.

csrc/flash_attn.hip (no SxS materialization, LSE saved).  Round-2
generality (ref flash_attention.py:174 call semantics):
- causal self-attention (LLaMA/GPT): sq == sk, sq % 64 == 0;
- bidirectional with optional per-batch key lengths (BERT suffix padding
  masks become klens int32 [b]);
- cross-attention (sq != sk, ragged sk) for the SD UNet;
- head_dim in {40, 64, 80, 96, 128, 160} (BERT 64, GPT2-3.5B 96,
  LLaMA 128, SD 40/80/160);
- causal with a per-row key start (``kstart`` int32 [b, s]: row i sees
  keys kstart[i] <= j <= i) for padded and packed batches: right padding
  (0), left padding by p (p), packed documents (start of the row's
  document); a pad row sees only itself (kstart[i] = i).  v3 shapes only,
  no dropout;
- grouped-query attention: k/v with h_kv heads, h % h_kv == 0, query head
  j uses KV head j // (h / h_kv) (HF ``repeat_kv`` order).  Native in the
  causal v3 kernels without dropout, with or without ``kstart``; K/V are
  never expanded and dK/dV come back with h_kv heads.
"""
from __future__ import annotations

import os
from typing import Optional

import torch

from fengshen_amd.ops import get_ext

_FLASH_DIMS = (40, 64, 80, 96, 128, 160)


def _v3_eligible(ext, q, k, causal, klens, dropout_p):
    """v3 (swapped-QK^T 32x32 schedule, ~1.8x): self-attention at
    d in {64, 128} with s % 64 == 0; causal or klens-masked bidirectional.
    Dropout routes to the general kernels by default: a same-box A/B on
    the BERT step (b128 s512 d64 p=0.1) measured them identical (177.2
    vs 177.5/178.8 samples/s — the step is no longer attention-bound),
    so the simpler routing stands; FENGSHEN_FLASH_V3_DROP=1 flips
    dropout onto v3 at d 64/96 for experiments."""
    if not (hasattr(ext, "flash_attn_fwd_v3")
            and q.shape[-1] in (64, 96, 128)
            and q.shape[-2] == k.shape[-2]
            and q.shape[-2] % 64 == 0 and q.shape[-2] >= 64):
        return False
    if dropout_p > 0:
        return os.environ.get("FENGSHEN_FLASH_V3_DROP") == "1" \
            and q.shape[-1] in (64, 96)
    return True


def gqa_flash_enabled() -> bool:
    """FENGSHEN_GQA_FLASH=0 expands K/V to the query heads in front of
    every attention path instead of using the grouped-query kernels."""
    return os.environ.get("FENGSHEN_GQA_FLASH", "1") != "0"


def gqa_flash_supported(q: torch.Tensor, k: torch.Tensor, causal: bool,
                        dropout_p: float) -> bool:
    """Calls the grouped-query kernels cover: bf16 on the GPU, causal
    self-attention at v3 shapes, no dropout (a mask must reduce to kstart —
    the caller's check)."""
    return (gqa_flash_enabled() and causal and q.is_cuda
            and q.shape[1] % k.shape[1] == 0
            and kstart_supported(q.shape[-1], q.shape[-2], k.shape[-2],
                                 q.dtype, dropout_p))


def expand_kv(x: torch.Tensor, num_heads: int) -> torch.Tensor:
    """[b, h_kv, s, d] -> [b, h, s, d], query head j <- KV head j // G.
    Autograd sums the group's gradients."""
    b, h_kv, s, d = x.shape
    if h_kv == num_heads:
        return x
    if num_heads % h_kv:
        raise ValueError(f"{num_heads} query heads are not a multiple of "
                         f"{h_kv} KV heads")
    g = num_heads // h_kv
    return x[:, :, None].expand(b, h_kv, g, s, d).reshape(b, num_heads, s, d)


def varlen_flash_enabled() -> bool:
    """FENGSHEN_VARLEN_FLASH=0 keeps causal attention under a mask on the
    bmm + masked-softmax path."""
    return os.environ.get("FENGSHEN_VARLEN_FLASH", "1") != "0"


def kstart_supported(head_dim: int, sq: int, sk: int, dtype,
                     dropout_p: float) -> bool:
    """Shapes the kstart kernels cover."""
    return (dtype == torch.bfloat16 and head_dim in (64, 96, 128)
            and sq == sk and sq % 64 == 0 and sq >= 64 and dropout_p == 0)


def kstart_qend(kstart: torch.Tensor) -> torch.Tensor:
    """Query-loop bound of the dkv kernel: int32 [b, s/64], entry t = the
    last row i with kstart[i] <= 64*t + 63 (the last key of 64-key tile t).
    kstart must be non-decreasing along s, so this is a searchsorted; it
    runs on kstart's device with no host sync."""
    b, s = kstart.shape
    last_key = torch.arange(63, s, 64, device=kstart.device,
                            dtype=kstart.dtype)
    pos = torch.searchsorted(kstart, last_key.unsqueeze(0).expand(b, -1)
                             .contiguous(), right=True)
    return (pos - 1).to(torch.int32)


def kstart_to_mask(kstart: torch.Tensor) -> torch.Tensor:
    """The dense [b, 1, s, s] bool mask (True = masked) kstart stands for."""
    s = kstart.shape[1]
    ar = torch.arange(s, device=kstart.device)
    i, j = ar.view(1, s, 1), ar.view(1, 1, s)
    return ((j > i) | (j < kstart.unsqueeze(2))).unsqueeze(1)


def kstart_from_eod(tokens: torch.Tensor, eod_token: int) -> torch.Tensor:
    """int32 [b, s] key start of a packed batch: a document ends with its
    EOD token and the next one starts behind it, as with
    get_ltor_masks_and_position_ids(reset_attention_mask=True) — whose
    [b, 1, s, s] mask is kstart_to_mask of this and is never built here."""
    b, s = tokens.shape
    ar = torch.arange(s, device=tokens.device)
    # start of the document that follows an EOD at j is j + 1; a row's
    # start is the latest one at or before it
    starts = torch.where(tokens == eod_token, ar + 1, torch.zeros_like(ar))
    starts = torch.cat([starts.new_zeros(b, 1), starts[:, :-1]], dim=1)
    return torch.cummax(starts, dim=1).values.to(torch.int32)


def mask_to_kstart(mask: torch.Tensor, s: int) -> Optional[torch.Tensor]:
    """Convert a True=masked mask of causal self-attention over s tokens
    into a per-row key start (int32 [b, s]), or None if it is not one:
    - [b, s] or [b, 1, 1, s] key-pad mask whose kept keys form one
      contiguous run per batch row (left, right or no padding).  Real rows
      start at the run's first key; pad rows see only themselves.
    - [b, 1, s, s] mask that is exactly "j > i or j < kstart[i]" with a
      non-decreasing kstart (packed documents).
    The candidate is verified by rebuilding the mask from it."""
    if mask.dtype != torch.bool:
        mask = mask != 0
    ar = torch.arange(s, device=mask.device)
    if mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == s \
            and mask.shape[3] == s and s > 1:
        keep = ~mask[:, 0]
        ks = keep.to(torch.int8).argmax(dim=2)        # first kept key
        cand = ((ar.view(1, 1, s) > ar.view(1, s, 1))
                | (ar.view(1, 1, s) < ks.unsqueeze(2)))
        if not torch.equal(cand, mask[:, 0]):
            return None
        if not bool((ks[:, 1:] >= ks[:, :-1]).all()):
            return None
        return ks.to(torch.int32).contiguous()
    if mask.dim() == 4:
        if mask.shape[1] != 1 or mask.shape[2] != 1 or mask.shape[3] != s:
            return None
        m2 = mask[:, 0, 0, :]
    elif mask.dim() == 2 and mask.shape[1] == s:
        m2 = mask
    else:
        return None
    keep = ~m2
    n = keep.sum(dim=1)
    first = keep.to(torch.int8).argmax(dim=1)
    run = (ar.unsqueeze(0) >= first.unsqueeze(1)) \
        & (ar.unsqueeze(0) < (first + n).unsqueeze(1))
    if not torch.equal(run, keep):
        return None  # holes between the keys
    ks = torch.where(keep, first.unsqueeze(1), ar.unsqueeze(0))
    return ks.to(torch.int32).contiguous()


def model_kstart(mask: Optional[torch.Tensor], x: torch.Tensor
                 ) -> Optional[torch.Tensor]:
    """For a model's forward: convert its causal ``mask`` once for all
    layers (mask_to_kstart compares on the device and reads the verdict
    back) when the hidden states x [b, s, h] can reach the kstart kernels
    at all; the layers still check head dim and dropout for themselves and
    keep the mask for what the kernels do not cover."""
    if mask is None or not varlen_flash_enabled():
        return None
    s = x.shape[1]
    if not (x.is_cuda and x.dtype == torch.bfloat16 and s % 64 == 0
            and s >= 64 and mask.shape[-1] == s):
        return None
    return mask_to_kstart(mask, s)


class _FlashAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, causal, klens, dropout_p, seed,
                kstart=None):
        ext = get_ext()
        ctx.kstart = kstart
        if kstart is not None:
            # no quiet fall-back: the binding raises on anything the
            # kstart kernels do not cover
            o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, causal, klens,
                                           dropout_p, seed, kstart=kstart)
            ctx.qend = kstart_qend(kstart)
        elif k.shape[1] != q.shape[1] \
                or _v3_eligible(ext, q, k, causal, klens, dropout_p):
            # grouped-query K/V exist in the v3 kernels only; the binding
            # raises on what they do not cover
            o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, causal, klens,
                                           dropout_p, seed)
        else:
            o, lse = ext.flash_attn_fwd(q, k, v, scale, causal, klens,
                                        dropout_p, seed)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.scale = scale
        ctx.causal = causal
        ctx.klens = klens
        ctx.dropout_p = dropout_p
        ctx.seed = seed
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        ext = get_ext()
        if ctx.kstart is not None:
            dq, dk, dv = ext.flash_attn_bwd_v3(
                q, k, v, o, do.contiguous(), lse, ctx.scale, ctx.causal,
                ctx.klens, ctx.dropout_p, ctx.seed, kstart=ctx.kstart,
                qend=ctx.qend)
        elif k.shape[1] != q.shape[1] \
                or _v3_eligible(ext, q, k, ctx.causal, ctx.klens,
                                ctx.dropout_p):
            dq, dk, dv = ext.flash_attn_bwd_v3(
                q, k, v, o, do.contiguous(), lse, ctx.scale, ctx.causal,
                ctx.klens, ctx.dropout_p, ctx.seed)
        else:
            dq, dk, dv = ext.flash_attn_bwd(
                q, k, v, o, do.contiguous(), lse, ctx.scale, ctx.causal,
                ctx.klens, ctx.dropout_p, ctx.seed)
        return dq, dk, dv, None, None, None, None, None, None


def _split_qkv(qkv, num_heads, num_kv_heads):
    """[b, s, (np + 2*nkv)*hn] packed buffer, laid out [q | k | v] -> q as a
    [b, np, s, hn] view and k, v as [b, nkv, s, hn] views."""
    hn = qkv.shape[-1] // (num_heads + 2 * num_kv_heads)
    wq, wkv = num_heads * hn, num_kv_heads * hn
    q = qkv.narrow(2, 0, wq).unflatten(2, (num_heads, hn)).transpose(1, 2)
    k, v = (qkv.narrow(2, wq + i * wkv, wkv).unflatten(2, (num_kv_heads, hn))
            .transpose(1, 2) for i in range(2))
    return q, k, v


def _rope_packed(qkv, num_heads, num_kv_heads, cos, sin, offset, bwd):
    """Rotate the q and k heads of a packed buffer in place."""
    if num_kv_heads == num_heads:
        q, k, _ = _split_qkv(qkv, num_heads, num_kv_heads)
        get_ext().rope_inplace(q, k, cos, sin, offset, bwd)
        return
    # q and k are adjacent and share the head stride: one
    # [b, np + nkv, s, hn] view, one launch
    n = num_heads + num_kv_heads
    hn = qkv.shape[-1] // (n + num_kv_heads)
    qk = qkv.narrow(2, 0, n * hn).unflatten(2, (n, hn)).transpose(1, 2)
    get_ext().rope_inplace_one(qk, cos, sin, offset, bwd)


class _RopePackedInplace(torch.autograd.Function):
    """Rotates the q and k heads of a packed [b, s, (np + 2*nkv)*hn] buffer in
    place and returns it marked dirty, so autograd sees the overwrite (no
    linear backward needs its own output, so overwriting the projection
    output is sound).  A function of its own because autograd allows an
    in-place update of a view input (a biased linear's output is one) only
    in a Function with a single output."""

    @staticmethod
    def forward(ctx, qkv, num_heads, cos, sin, offset, num_kv_heads=None):
        num_kv_heads = num_kv_heads or num_heads
        _rope_packed(qkv, num_heads, num_kv_heads, cos, sin, offset, False)
        ctx.mark_dirty(qkv)
        ctx.save_for_backward(cos, sin)
        ctx.num_heads = num_heads
        ctx.num_kv_heads = num_kv_heads
        ctx.offset = offset
        return qkv

    @staticmethod
    def backward(ctx, grad):
        cos, sin = ctx.saved_tensors
        # rotation is orthogonal: un-rotate the q/k thirds.  Done in place:
        # packed_self_attention never lets the rotated buffer escape, so
        # its only consumer is _PackedFlash, whose backward allocates this
        # gradient fresh and keeps no reference to it.
        if grad.stride(-1) != 1 or any(st % 8 for st in grad.stride()[:-1]) \
                or grad.storage_offset() % 8:
            grad = grad.contiguous()
        _rope_packed(grad, ctx.num_heads, ctx.num_kv_heads, cos, sin,
                     ctx.offset, True)
        return grad, None, None, None, None, None


class _PackedFlash(torch.autograd.Function):
    """v3 flash attention straight on the packed QKV buffer: the strided
    kernels read the three parts where the GEMM left them and write O as
    [b, s, np*hn]; backward writes dq/dk/dv into the parts of one packed
    gradient.  No layout copies, no ``cat``.  With num_kv_heads < num_heads
    the k and v parts are nkv*hn wide (grouped-query kernels)."""

    @staticmethod
    def forward(ctx, qkv, num_heads, scale, causal, klens, kstart=None,
                num_kv_heads=None):
        b, s, w = qkv.shape
        nkv = num_kv_heads or num_heads
        q, k, v = _split_qkv(qkv, num_heads, nkv)
        o = torch.empty(b, s, w // (num_heads + 2 * nkv) * num_heads,
                        dtype=qkv.dtype, device=qkv.device)
        ov = o.unflatten(2, (num_heads, -1)).transpose(1, 2)
        if kstart is not None:
            lse = get_ext().flash_attn_fwd_v3_strided(
                q, k, v, ov, scale, causal, klens, kstart=kstart)
            ctx.qend = kstart_qend(kstart)
        else:
            lse = get_ext().flash_attn_fwd_v3_strided(q, k, v, ov, scale,
                                                      causal, klens)
        ctx.kstart = kstart
        ctx.save_for_backward(qkv, o, lse)
        ctx.num_heads = num_heads
        ctx.num_kv_heads = nkv
        ctx.scale = scale
        ctx.causal = causal
        ctx.klens = klens
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        np_ = ctx.num_heads
        q, k, v = _split_qkv(qkv, np_, ctx.num_kv_heads)
        # dO is read where it lies as long as its last dim is contiguous
        if do.stride(-1) != 1 or any(st % 8 for st in do.stride()[:-1]) \
                or do.storage_offset() % 8:
            do = do.contiguous()
        grad = torch.empty(qkv.shape, dtype=qkv.dtype, device=qkv.device)
        dq, dk, dv = _split_qkv(grad, np_, ctx.num_kv_heads)
        kw = {}
        if ctx.kstart is not None:
            kw = {"kstart": ctx.kstart, "qend": ctx.qend}
        get_ext().flash_attn_bwd_v3_strided(
            q, k, v, o.unflatten(2, (np_, -1)).transpose(1, 2),
            do.unflatten(2, (np_, -1)).transpose(1, 2), lse, dq, dk, dv,
            ctx.scale, ctx.causal, ctx.klens, **kw)
        return grad, None, None, None, None, None, None


def packed_attn_eligible(qkv, head_dim: int, causal: bool, mask,
                         dropout_p: float, num_heads: Optional[int] = None,
                         num_kv_heads: Optional[int] = None) -> bool:
    """True when self-attention can run on the packed [b, s, (np+2*nkv)*hn]
    projection output in place: v3 shapes (d in {64, 96, 128}, s % 64 == 0),
    bf16, no dropout.  Grouped-query layouts (num_kv_heads != num_heads)
    are causal only and off under FENGSHEN_GQA_FLASH=0.  A mask must still reduce to klens (bidirectional)
    or to kstart (causal) — checked by the caller; under causal a mask is
    refused outright when FENGSHEN_VARLEN_FLASH=0.  FENGSHEN_PACKED_ATTN=0
    forces the chunk/transpose/contiguous path."""
    if os.environ.get("FENGSHEN_PACKED_ATTN", "1") == "0":
        return False
    if qkv.dtype != torch.bfloat16 or qkv.dim() != 3 or dropout_p > 0:
        return False
    if num_kv_heads is not None and num_kv_heads != num_heads \
            and not (causal and gqa_flash_enabled()):
        return False
    s = qkv.shape[1]
    if head_dim not in (64, 96, 128) or s % 64 != 0 or s < 64:
        return False
    if causal and mask is not None and not varlen_flash_enabled():
        return False
    return (qkv.stride(2) == 1 and qkv.stride(0) % 8 == 0
            and qkv.stride(1) % 8 == 0 and qkv.storage_offset() % 8 == 0)


def packed_self_attention(qkv: torch.Tensor, num_heads: int,
                          cos: Optional[torch.Tensor],
                          sin: Optional[torch.Tensor], offset: int,
                          scale: float, causal: bool = True,
                          klens: Optional[torch.Tensor] = None,
                          kstart: Optional[torch.Tensor] = None,
                          num_kv_heads: Optional[int] = None
                          ) -> torch.Tensor:
    """qkv [b, s, (np + 2*nkv)*hn] bf16 (nkv = num_kv_heads, default np),
    partition-local layout [q | k | v], last dim unit-stride.  Rotates q/k IN PLACE when cos/sin are given (pass None
    for no rotary) and returns the context as [b, s, np*hn], ready for the
    output projection.  Callers must not reuse ``qkv`` afterwards.
    ``kstart`` (int32 [b, s], causal only): per-row key start."""
    if cos is not None:
        qkv = _RopePackedInplace.apply(qkv, num_heads, cos, sin, offset,
                                       num_kv_heads)
    return _PackedFlash.apply(qkv, num_heads, float(scale), causal, klens,
                              kstart, num_kv_heads)


def _draw_seed(device) -> int:
    """Per-call dropout seed: CPU torch RNG (deterministic under
    torch.manual_seed) mixed with the TP rank so TP-local heads get
    decorrelated masks (eager path forks the mpu RNG tracker for the
    same reason)."""
    base = int(torch.randint(0, 2 ** 62, (1,)).item())
    try:
        from fengshen_amd.parallel import groups as pg
        base += pg.get_tensor_model_parallel_rank() * 0x9E3779B9
    except Exception:
        pass
    return base


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                    scale: float, causal: bool = True,
                    klens: Optional[torch.Tensor] = None,
                    dropout_p: float = 0.0,
                    kstart: Optional[torch.Tensor] = None) -> torch.Tensor:
    """q [b,h,sq,d], k/v [b,h_kv,sk,d] bf16 contiguous; h_kv < h (grouped
    queries) needs causal v3 shapes without dropout and returns dk/dv with
    h_kv heads — anything else raises.  dropout_p > 0
    applies attention dropout with an in-kernel counter hash (no mask
    tensor); the normalizer uses the undropped row sum, matching eager
    dropout(softmax(S)) @ V.  kstart (int32 [b, s], non-decreasing along
    s): causal attention where row i sees keys kstart[i] <= j <= i; v3
    shapes, no dropout — anything else raises."""
    seed = _draw_seed(q.device) if dropout_p > 0 else 0
    return _FlashAttention.apply(q.contiguous(), k.contiguous(),
                                 v.contiguous(), scale, causal, klens,
                                 float(dropout_p), seed, kstart)


def mask_to_klens(mask: torch.Tensor, sk: int) -> Optional[torch.Tensor]:
    """Convert a True=masked pad mask into per-batch key lengths when it is
    a pure suffix-padding pattern ([b,1,1,sk] or [b,sk]); else None."""
    if mask.dtype != torch.bool:
        mask = mask != 0
    if mask.dim() == 4:
        if mask.shape[2] != 1 or mask.shape[1] != 1 or mask.shape[3] != sk:
            return None
        m2 = mask[:, 0, 0, :]
    elif mask.dim() == 2 and mask.shape[1] == sk:
        m2 = mask
    else:
        return None
    klens = (~m2).sum(dim=1, dtype=torch.int32)
    ar = torch.arange(sk, device=mask.device, dtype=torch.int32)
    if not torch.equal(m2, ar.unsqueeze(0) >= klens.unsqueeze(1)):
        return None  # not suffix padding
    return klens.contiguous()


def flash_attn_supported(q, k, v, causal, mask, dropout_p) -> bool:
    if q.dtype != torch.bfloat16:
        return False
    if q.shape[-1] not in _FLASH_DIMS:
        return False
    sq, sk = q.shape[-2], k.shape[-2]
    if causal:
        return mask is None and sq == sk and sq % 64 == 0
    # bidirectional: sq tiles at 16; sk arbitrary; mask must convert to
    # suffix-pad klens (checked by the caller via mask_to_klens)
    return sq % 16 == 0 and sq >= 16
