"""Block-sparse self-attention (DeepSpeed sparse-attention equivalent).

Behavioral parity: reference models/megatron/layers/utils.py:187-296
(configure_sparse_attention) — the reference builds DeepSpeed/Triton
SparseSelfAttention with one of five sparsity configs (fixed, variable,
local sliding-window, bigbird, bslongformer).  Here the layouts are
reproduced exactly as [num_heads, nb, nb] block masks.

Two paths sit behind SparseSelfAttention:

- kernel path: bf16 on the GPU, head dim 64/96/128, block 16/32/64/128.
  The layout becomes tile lists (ops/sparse_flash.py) and the block-sparse
  flash kernels in csrc/sparse_flash.hip walk them: forward and backward
  touch only active tiles, nothing of size s x s exists, gradients are
  bit-reproducible.  A query row that sees no key (all its keys masked)
  returns 0 there.
- eager blockwise path: everything else (fp32, CPU, other head dims,
  block 8), and any input when FENGSHEN_SPARSE_FLASH=0.  For every query
  block only its active key blocks are gathered and attended, so memory is
  O(s * active_blocks * block) instead of O(s^2).
"""
from __future__ import annotations

import math
import os
from typing import List, Optional

import torch
import torch.nn as nn

__all__ = [
    "FixedSparsityConfig",
    "VariableSparsityConfig",
    "LocalSlidingWindowSparsityConfig",
    "BigBirdSparsityConfig",
    "BSLongformerSparsityConfig",
    "SparseSelfAttention",
    "configure_sparse_attention",
]


class SparsityConfig:
    """Base: builds a [num_heads, nb, nb] bool layout (True = attend)."""

    def __init__(self, num_heads: int, block: int = 16,
                 different_layout_per_head: bool = False,
                 attention: str = "unidirectional"):
        self.num_heads = num_heads
        self.block = block
        self.different_layout_per_head = different_layout_per_head
        self.attention = attention

    # -- helpers -------------------------------------------------------
    def _empty(self, nb: int) -> torch.Tensor:
        h = self.num_heads if self.different_layout_per_head else 1
        return torch.zeros(h, nb, nb, dtype=torch.bool)

    def _finalize(self, layout: torch.Tensor) -> torch.Tensor:
        nb = layout.shape[-1]
        if self.attention == "unidirectional":
            causal = torch.tril(torch.ones(nb, nb, dtype=torch.bool))
            layout = layout & causal
        if layout.shape[0] == 1 and self.num_heads > 1:
            layout = layout.expand(self.num_heads, nb, nb).contiguous()
        return layout

    def num_blocks(self, seq_len: int) -> int:
        if seq_len % self.block != 0:
            raise ValueError(
                f"seq_len {seq_len} not divisible by block {self.block}")
        return seq_len // self.block

    def make_layout(self, seq_len: int) -> torch.Tensor:
        raise NotImplementedError


class FixedSparsityConfig(SparsityConfig):
    """Local blocks + periodic global columns (ref utils.py:199-216)."""

    def __init__(self, num_heads, block=16, different_layout_per_head=False,
                 num_local_blocks: int = 4, num_global_blocks: int = 1,
                 num_different_global_patterns: int = 1,
                 attention="unidirectional",
                 horizontal_global_attention: bool = False):
        super().__init__(num_heads, block, different_layout_per_head,
                         attention)
        self.num_local_blocks = num_local_blocks
        self.num_global_blocks = num_global_blocks
        self.num_different_global_patterns = num_different_global_patterns
        self.horizontal_global_attention = horizontal_global_attention

    def make_layout(self, seq_len: int) -> torch.Tensor:
        nb = self.num_blocks(seq_len)
        layout = self._empty(nb)
        nh = layout.shape[0]
        L = self.num_local_blocks
        for h in range(nh):
            # local windows: blocks grouped in chunks of L attend within chunk
            for qb in range(nb):
                start = (qb // L) * L
                layout[h, qb, start:qb + 1] = True
            # global: last `num_global_blocks` of each local window attend /
            # are attended everywhere (pattern offset varies per head)
            pat = h % self.num_different_global_patterns
            for w_end in range(L, nb + 1, L):
                g0 = w_end - (pat + 1) * self.num_global_blocks
                g1 = g0 + self.num_global_blocks
                g0 = max(g0, w_end - L)
                layout[h, w_end - 1:, g0:g1] = True  # later rows see globals
                if self.horizontal_global_attention:
                    layout[h, g0:g1, :] = True
        return self._finalize(layout)


class VariableSparsityConfig(SparsityConfig):
    """Custom local window sizes + explicit global blocks + random blocks
    (ref utils.py:217-237)."""

    def __init__(self, num_heads, block=16, different_layout_per_head=False,
                 num_random_blocks: int = 0,
                 local_window_blocks: Optional[List[int]] = None,
                 global_block_indices: Optional[List[int]] = None,
                 global_block_end_indices: Optional[List[int]] = None,
                 attention="unidirectional",
                 horizontal_global_attention: bool = False):
        super().__init__(num_heads, block, different_layout_per_head,
                         attention)
        self.num_random_blocks = num_random_blocks
        self.local_window_blocks = local_window_blocks or [4]
        self.global_block_indices = global_block_indices or [0]
        self.global_block_end_indices = global_block_end_indices
        self.horizontal_global_attention = horizontal_global_attention

    def make_layout(self, seq_len: int) -> torch.Tensor:
        nb = self.num_blocks(seq_len)
        layout = self._empty(nb)
        nh = layout.shape[0]
        # local windows: consecutive groups sized by local_window_blocks
        # (last size repeats)
        sizes = list(self.local_window_blocks)
        start = 0
        while start < nb:
            w = sizes.pop(0) if sizes else self.local_window_blocks[-1]
            end = min(start + w, nb)
            layout[:, start:end, start:end] = True
            start = end
        # globals
        if self.global_block_end_indices:
            spans = zip(self.global_block_indices,
                        self.global_block_end_indices)
        else:
            spans = [(i, i + 1) for i in self.global_block_indices]
        for g0, g1 in spans:
            layout[:, :, g0:g1] = True
            if self.horizontal_global_attention:
                layout[:, g0:g1, :] = True
        # random blocks (seeded per head for determinism)
        if self.num_random_blocks:
            g = torch.Generator().manual_seed(1234)
            for h in range(nh):
                for qb in range(nb):
                    cols = torch.randint(0, nb, (self.num_random_blocks,),
                                         generator=g)
                    layout[h, qb, cols] = True
        return self._finalize(layout)


class LocalSlidingWindowSparsityConfig(SparsityConfig):
    """Pure sliding window of num_sliding_window_blocks
    (ref utils.py:238-252)."""

    def __init__(self, num_heads, block=16,
                 num_sliding_window_blocks: int = 4,
                 attention="unidirectional"):
        super().__init__(num_heads, block, False, attention)
        self.num_sliding_window_blocks = num_sliding_window_blocks

    def make_layout(self, seq_len: int) -> torch.Tensor:
        nb = self.num_blocks(seq_len)
        layout = self._empty(nb)
        w = self.num_sliding_window_blocks
        for qb in range(nb):
            lo = max(0, qb - w // 2) if self.attention == "bidirectional" \
                else max(0, qb - w + 1)
            hi = min(nb, qb + (w + 1) // 2) \
                if self.attention == "bidirectional" else qb + 1
            layout[:, qb, lo:hi] = True
        return self._finalize(layout)


class BigBirdSparsityConfig(SparsityConfig):
    """random + sliding window + global (ref utils.py:253-266)."""

    def __init__(self, num_heads, block=16, different_layout_per_head=False,
                 num_random_blocks: int = 1,
                 num_sliding_window_blocks: int = 3,
                 num_global_blocks: int = 1, attention="unidirectional"):
        super().__init__(num_heads, block, different_layout_per_head,
                         attention)
        self.num_random_blocks = num_random_blocks
        self.num_sliding_window_blocks = num_sliding_window_blocks
        self.num_global_blocks = num_global_blocks

    def make_layout(self, seq_len: int) -> torch.Tensor:
        nb = self.num_blocks(seq_len)
        layout = self._empty(nb)
        nh = layout.shape[0]
        w = self.num_sliding_window_blocks
        for qb in range(nb):
            layout[:, qb, max(0, qb - w + 1):qb + 1] = True
        g = self.num_global_blocks
        layout[:, :, :g] = True   # everyone sees the first g blocks
        layout[:, :g, :] = True   # first g blocks see everything (pre-causal)
        gen = torch.Generator().manual_seed(1234)
        for h in range(nh):
            for qb in range(nb):
                cols = torch.randint(0, max(qb, 1), (self.num_random_blocks,),
                                     generator=gen)
                layout[h, qb, cols] = True
        return self._finalize(layout)


class BSLongformerSparsityConfig(SparsityConfig):
    """sliding window + explicit global block spans (ref utils.py:267-283)."""

    def __init__(self, num_heads, block=16, different_layout_per_head=False,
                 num_sliding_window_blocks: int = 3,
                 global_block_indices: Optional[List[int]] = None,
                 global_block_end_indices: Optional[List[int]] = None,
                 attention="unidirectional"):
        super().__init__(num_heads, block, different_layout_per_head,
                         attention)
        self.num_sliding_window_blocks = num_sliding_window_blocks
        self.global_block_indices = global_block_indices or [0]
        self.global_block_end_indices = global_block_end_indices

    def make_layout(self, seq_len: int) -> torch.Tensor:
        nb = self.num_blocks(seq_len)
        layout = self._empty(nb)
        w = self.num_sliding_window_blocks
        for qb in range(nb):
            layout[:, qb, max(0, qb - w + 1):qb + 1] = True
        if self.global_block_end_indices:
            spans = zip(self.global_block_indices,
                        self.global_block_end_indices)
        else:
            spans = [(i, i + 1) for i in self.global_block_indices]
        for g0, g1 in spans:
            layout[:, :, g0:g1] = True
            layout[:, g0:g1, :] = True
        return self._finalize(layout)


class SparseSelfAttention(nn.Module):
    """Blockwise attention under a SparsityConfig layout.

    Input q/k/v: [b, np, s, hn] (same convention as ops.functional
    .attention).  For each query block only the union of active key
    blocks across heads is gathered; inactive (head, block) pairs are
    masked with -inf before the softmax, intra-diagonal-block causality
    is enforced by index comparison.  Layouts are cached per seq_len.

    bf16 GPU inputs with a supported head dim and block run the
    block-sparse flash kernels instead (see the module docstring); their
    tile lists are cached per (seq_len, device) next to the layouts.
    """

    def __init__(self, sparsity_config: SparsityConfig,
                 max_seq_length: int = 2048, attn_mask_mode: str = "add"):
        super().__init__()
        self.config = sparsity_config
        self.max_seq_length = max_seq_length
        self.attn_mask_mode = attn_mask_mode
        self._layouts = {}
        self._tile_lists = {}

    def layout(self, seq_len: int, device) -> torch.Tensor:
        key = (seq_len, str(device))
        if key not in self._layouts:
            self._layouts[key] = self.config.make_layout(seq_len).to(device)
        return self._layouts[key]

    def tile_lists(self, seq_len: int, device):
        """Tile lists of the layout for the block-sparse flash kernels."""
        key = (seq_len, str(device))
        if key not in self._tile_lists:
            from fengshen_amd.ops.sparse_flash import build_tile_lists
            lists = build_tile_lists(self.config.make_layout(seq_len),
                                     self.config.block, seq_len)
            self._tile_lists[key] = lists.to(device)
        return self._tile_lists[key]

    def uses_kernel(self, q: torch.Tensor) -> bool:
        """True if forward(q, ...) takes the block-sparse flash kernels."""
        if not q.is_cuda or q.dtype != torch.bfloat16:
            return False
        if os.environ.get("FENGSHEN_SPARSE_FLASH") == "0":
            return False
        from fengshen_amd.ops import sparse_flash as sf
        from fengshen_amd.ops import use_hip
        return (q.shape[-1] in sf.SPARSE_FLASH_DIMS
                and self.config.block in sf.SPARSE_FLASH_BLOCKS
                and use_hip(q) and sf.sparse_flash_available())

    def density(self, seq_len: int) -> float:
        lay = self.config.make_layout(seq_len)
        return lay.float().mean().item()

    def forward(self, q, k, v, attention_mask=None,
                scale: Optional[float] = None):
        b, np_, s, hn = q.shape
        B = self.config.block
        nb = s // B
        scale = scale if scale is not None else 1.0 / math.sqrt(hn)
        causal = self.config.attention == "unidirectional"
        if self.uses_kernel(q):
            from fengshen_amd.ops.sparse_flash import block_sparse_attention
            self.config.num_blocks(s)  # s % block == 0
            return block_sparse_attention(
                q, k, v, self.tile_lists(s, q.device), scale, causal,
                key_mask=attention_mask)
        layout = self.layout(s, q.device)  # [np, nb, nb]

        kb = k.view(b, np_, nb, B, hn)
        vb = v.view(b, np_, nb, B, hn)
        out = torch.empty_like(q)
        neg = torch.finfo(torch.float32).min
        for qb in range(nb):
            active = layout[:, qb]                       # [np, nb]
            cols = active.any(dim=0).nonzero(as_tuple=True)[0]  # [nk]
            if cols.numel() == 0:
                out[:, :, qb * B:(qb + 1) * B] = 0
                continue
            kg = kb[:, :, cols].reshape(b, np_, -1, hn)  # [b,np,nk*B,hn]
            vg = vb[:, :, cols].reshape(b, np_, -1, hn)
            qq = q[:, :, qb * B:(qb + 1) * B]            # [b,np,B,hn]
            scores = (qq.float() @ kg.float().transpose(-1, -2)) * scale
            # per-head block mask
            hmask = active[:, cols]                      # [np, nk]
            scores = scores.view(b, np_, B, cols.numel(), B)
            scores = scores.masked_fill(
                ~hmask[None, :, None, :, None], neg)
            if causal:
                qpos = qb * B + torch.arange(B, device=q.device)
                kpos = (cols[:, None] * B
                        + torch.arange(B, device=q.device)[None, :])
                cmask = kpos[None, :, :] > qpos[:, None, None]  # [B,nk,B]
                scores = scores.masked_fill(
                    cmask[None, None, :, :, :], neg)
            if attention_mask is not None:
                # [b, s] padding mask, 1 = keep
                km = attention_mask[:, cols.reshape(-1, 1) * B
                                    + torch.arange(B, device=q.device)]
                scores = scores.masked_fill(
                    (km == 0)[:, None, None, :, :], neg)
            scores = scores.view(b, np_, B, -1)
            probs = torch.softmax(scores, dim=-1).to(v.dtype)
            out[:, :, qb * B:(qb + 1) * B] = probs @ vg
        return out


def configure_sparse_attention(config, attention_type: str,
                               num_attention_heads: int):
    """reference models/megatron/layers/utils.py:187-296 — same attention
    types and sparsity_config dict keys."""
    sc = getattr(config, "sparsity_config", None) or {}
    block = sc.get("block", 16)
    dlph = sc.get("different_layout_per_head", False)
    if attention_type == "sparse_fixed":
        cfg = FixedSparsityConfig(
            num_heads=num_attention_heads, block=block,
            different_layout_per_head=dlph,
            num_local_blocks=sc.get("num_local_blocks", 4),
            num_global_blocks=sc.get("num_global_blocks", 1),
            num_different_global_patterns=sc.get(
                "num_different_global_patterns", 1),
            attention="unidirectional", horizontal_global_attention=False)
    elif attention_type == "sparse_variable":
        cfg = VariableSparsityConfig(
            num_heads=num_attention_heads, block=block,
            different_layout_per_head=dlph,
            num_random_blocks=sc.get("num_random_blocks", 0),
            local_window_blocks=sc.get("local_window_blocks", [4]),
            global_block_indices=sc.get("global_block_indices", [0]),
            global_block_end_indices=sc.get("global_block_end_indices"),
            attention="unidirectional", horizontal_global_attention=False)
    elif attention_type == "local":
        nlb = sc.get("num_local_blocks",
                     sc.get("num_sliding_window_blocks", 4))
        cfg = LocalSlidingWindowSparsityConfig(
            num_heads=num_attention_heads, block=block,
            num_sliding_window_blocks=nlb, attention="unidirectional")
    elif attention_type == "bigbird":
        cfg = BigBirdSparsityConfig(
            num_heads=num_attention_heads, block=block,
            different_layout_per_head=dlph,
            num_random_blocks=sc.get("num_random_blocks", 1),
            num_sliding_window_blocks=sc.get("num_sliding_window_blocks", 3),
            num_global_blocks=sc.get("num_global_blocks", 1),
            attention="unidirectional")
    elif attention_type == "bslongformer":
        cfg = BSLongformerSparsityConfig(
            num_heads=num_attention_heads, block=block,
            different_layout_per_head=dlph,
            num_sliding_window_blocks=sc.get("num_sliding_window_blocks", 3),
            global_block_indices=sc.get("global_block_indices", [0]),
            global_block_end_indices=sc.get("global_block_end_indices"),
            attention="unidirectional")
    else:
        raise ValueError(f"Attention type {attention_type} not recognized")
    max_len = getattr(config, "max_position_embeddings", 2048)
    return SparseSelfAttention(cfg, max_seq_length=max_len)
