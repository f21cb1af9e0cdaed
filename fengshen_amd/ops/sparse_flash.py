"""Block-sparse flash attention: tile lists + autograd wrapper.

csrc/sparse_flash.hip walks tile lists instead of the key axis.  This
module turns a [h, nb, nb] block layout into those lists (pure torch, no
GPU or extension needed) and wraps the two bindings in an autograd
Function.

List format (all int32, CSR).  The kernels work on 128-row query tiles
(8 waves x 16 rows) and 64-key tiles (4 groups of 16 keys); a layout of
block 16/32/64/128 is first expanded to 16-granular form, so one layout
bit becomes one or more 16x16 sub-blocks.

- row lists: for list head ``lh`` and query tile ``qt``, entries
  ``row_ptr[lh * nqt + qt] .. row_ptr[lh * nqt + qt + 1]`` of ``row_idx``
  (key tile index, ascending) and ``row_mask``.  Mask bit ``4 * w + n``:
  rows ``qt * 128 + 16 * w ..+15`` see keys ``kt * 64 + 16 * n ..+15``.
- col lists: the transpose.  For ``lh`` and key tile ``kt`` the query
  tiles that see it, with the same masks.
- ``list_heads`` is ``h``, or 1 when every head has the same layout (the
  lists are then stored once).
"""
from __future__ import annotations

from typing import Optional

import torch

from fengshen_amd.ops import get_ext

__all__ = ["TileLists", "build_tile_lists", "tile_lists_to_mask",
           "block_sparse_attention", "sparse_flash_available",
           "SPARSE_FLASH_DIMS", "SPARSE_FLASH_BLOCKS"]

Q_TILE = 128
K_TILE = 64
SUB = 16
SPARSE_FLASH_DIMS = (64, 96, 128)
SPARSE_FLASH_BLOCKS = (16, 32, 64, 128)


class TileLists:
    """Row and column tile lists of one (layout, seq_len)."""

    _FIELDS = ("row_ptr", "row_idx", "row_mask",
               "col_ptr", "col_idx", "col_mask")

    def __init__(self, row_ptr, row_idx, row_mask, col_ptr, col_idx,
                 col_mask, seq_len: int, num_heads: int, list_heads: int):
        self.row_ptr, self.row_idx, self.row_mask = row_ptr, row_idx, row_mask
        self.col_ptr, self.col_idx, self.col_mask = col_ptr, col_idx, col_mask
        self.seq_len = seq_len
        self.num_heads = num_heads
        self.list_heads = list_heads

    @property
    def num_q_tiles(self) -> int:
        return -(-self.seq_len // Q_TILE)

    @property
    def num_k_tiles(self) -> int:
        return -(-self.seq_len // K_TILE)

    @property
    def device(self):
        return self.row_ptr.device

    def to(self, device) -> "TileLists":
        return TileLists(*(getattr(self, f).to(device) for f in self._FIELDS),
                         self.seq_len, self.num_heads, self.list_heads)

    def validate(self) -> None:
        """CSR structure and tile-index range of both lists (host pass;
        run once when the lists are built, never per call)."""
        for ptr, idx, mask, n_lists, n_idx, name in (
                (self.row_ptr, self.row_idx, self.row_mask,
                 self.num_q_tiles, self.num_k_tiles, "row"),
                (self.col_ptr, self.col_idx, self.col_mask,
                 self.num_k_tiles, self.num_q_tiles, "col")):
            for t in (ptr, idx, mask):
                if t.dtype != torch.int32 or t.dim() != 1:
                    raise ValueError(f"{name} lists must be 1-D int32")
            if ptr.numel() != self.list_heads * n_lists + 1:
                raise ValueError(f"{name}_ptr has {ptr.numel()} entries, "
                                 f"expected {self.list_heads * n_lists + 1}")
            if idx.numel() != mask.numel():
                raise ValueError(f"{name}_idx / {name}_mask length mismatch")
            p = ptr.cpu()
            if p[0].item() != 0 or p[-1].item() != idx.numel() \
                    or (p[1:] < p[:-1]).any().item():
                raise ValueError(f"{name}_ptr is not a CSR pointer array")
            if idx.numel() and (idx.min().item() < 0
                                or idx.max().item() >= n_idx):
                raise ValueError(f"{name}_idx out of range [0, {n_idx})")


def _csr(mask3: torch.Tensor):
    """[L, n_outer, n_inner] int64 masks -> (ptr, idx, mask) over the
    non-zero entries, inner index ascending."""
    nz = mask3 != 0
    counts = nz.sum(dim=-1).reshape(-1)
    ptr = torch.zeros(counts.numel() + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(counts, 0)
    where = nz.nonzero(as_tuple=False)  # row-major: (l, outer, inner) sorted
    idx = where[:, 2]
    vals = mask3[nz]
    # bit 31 may be set: reinterpret the low 32 bits as int32
    vals = torch.where(vals >= 2 ** 31, vals - 2 ** 32, vals)
    return (ptr.to(torch.int32), idx.to(torch.int32).contiguous(),
            vals.to(torch.int32).contiguous())


def build_tile_lists(layout: torch.Tensor, block: int,
                     seq_len: int) -> TileLists:
    """layout: bool [h, nb, nb] (True = attend), nb * block == seq_len."""
    if block not in SPARSE_FLASH_BLOCKS:
        raise ValueError(f"block must be one of {SPARSE_FLASH_BLOCKS}, "
                         f"got {block}")
    if layout.dim() != 3 or layout.shape[1] != layout.shape[2]:
        raise ValueError("layout must be [h, nb, nb]")
    h, nb, _ = layout.shape
    if nb * block != seq_len:
        raise ValueError(f"layout of {nb} blocks of {block} does not cover "
                         f"seq_len {seq_len}")
    layout = layout.detach().to("cpu", torch.bool)
    list_heads = h
    if h > 1 and bool((layout == layout[:1]).all()):
        layout = layout[:1]
        list_heads = 1

    rep = block // SUB
    fine = layout.repeat_interleave(rep, 1).repeat_interleave(rep, 2)
    n16 = seq_len // SUB
    nqt = -(-seq_len // Q_TILE)
    nkt = -(-seq_len // K_TILE)
    wq, nk = Q_TILE // SUB, K_TILE // SUB           # 8 waves, 4 key groups
    padded = torch.zeros(list_heads, nqt * wq, nkt * nk, dtype=torch.int64)
    padded[:, :n16, :n16] = fine
    tiles = padded.view(list_heads, nqt, wq, nkt, nk)
    weight = (1 << (nk * torch.arange(wq)[:, None]
                    + torch.arange(nk)[None, :])).to(torch.int64)
    masks = (tiles * weight[None, None, :, None, :]).sum(dim=(2, 4))

    row = _csr(masks)                                # [lh, nqt, nkt]
    col = _csr(masks.transpose(1, 2).contiguous())   # [lh, nkt, nqt]
    lists = TileLists(*row, *col, seq_len, h, list_heads)
    lists.validate()
    return lists


def tile_lists_to_mask(lists: TileLists, seq_len: int) -> torch.Tensor:
    """Inverse of build_tile_lists: the dense bool [h, s, s] visibility the
    row lists describe (layout only: no causal triangle, no key mask).
    Deliberately a plain walk over the entries, independent of the
    builder's tensor arithmetic."""
    s = seq_len
    nqt = -(-s // Q_TILE)
    row_ptr = lists.row_ptr.cpu().tolist()
    row_idx = lists.row_idx.cpu().tolist()
    row_mask = lists.row_mask.cpu().tolist()
    out = torch.zeros(lists.list_heads, s, s, dtype=torch.bool)
    for lh in range(lists.list_heads):
        for qt in range(nqt):
            base = lh * nqt + qt
            for e in range(row_ptr[base], row_ptr[base + 1]):
                kt = row_idx[e]
                bits = row_mask[e] & 0xFFFFFFFF
                for w in range(Q_TILE // SUB):
                    for n in range(K_TILE // SUB):
                        if not (bits >> (4 * w + n)) & 1:
                            continue
                        r0 = qt * Q_TILE + w * SUB
                        c0 = kt * K_TILE + n * SUB
                        if r0 >= s or c0 >= s:
                            raise ValueError(
                                f"list entry ({lh}, {qt}, {kt}) has a bit "
                                f"beyond seq_len {s}")
                        out[lh, r0:r0 + SUB, c0:c0 + SUB] = True
    if lists.list_heads == 1 and lists.num_heads > 1:
        out = out.expand(lists.num_heads, s, s).contiguous()
    return out


def sparse_flash_available() -> bool:
    ext = get_ext()
    return ext is not None and hasattr(ext, "sparse_flash_fwd") \
        and hasattr(ext, "sparse_flash_bwd")


class _BlockSparseFlash(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, lists, scale, causal, key_mask):
        ext = get_ext()
        o, lse = ext.sparse_flash_fwd(
            q, k, v, lists.row_ptr, lists.row_idx, lists.row_mask, key_mask,
            scale, causal, False)
        ctx.save_for_backward(q, k, v, o, lse)
        ctx.lists = lists
        ctx.scale = scale
        ctx.causal = causal
        ctx.key_mask = key_mask
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        ls = ctx.lists
        dq, dk, dv = get_ext().sparse_flash_bwd(
            q, k, v, o, do.contiguous(), lse, ls.row_ptr, ls.row_idx,
            ls.row_mask, ls.col_ptr, ls.col_idx, ls.col_mask, ctx.key_mask,
            ctx.scale, ctx.causal, False)
        return dq, dk, dv, None, None, None, None


def block_sparse_attention(q, k, v, lists: TileLists, scale: float,
                           causal: bool,
                           key_mask: Optional[torch.Tensor] = None):
    """q/k/v: bf16 [b, h, s, d] on the GPU, d in {64, 96, 128}.  ``lists``
    must live on the same device (``lists.to(q.device)``).  ``causal``
    additionally hides kcol > qrow.  ``key_mask``: [b, s], non-zero = keep.
    A query row that sees no key returns 0 and gets / gives no gradient."""
    if not sparse_flash_available():
        raise RuntimeError(
            "block_sparse_attention needs the HIP extension with the "
            "sparse_flash entry points; run `python -m fengshen_amd.ops.build`")
    if lists.seq_len != q.shape[-2] or lists.num_heads != q.shape[1]:
        raise ValueError(
            f"tile lists are for h={lists.num_heads}, s={lists.seq_len}; "
            f"got q {tuple(q.shape)}")
    if key_mask is not None:
        key_mask = (key_mask != 0).to(torch.uint8).contiguous()
    return _BlockSparseFlash.apply(q.contiguous(), k.contiguous(),
                                   v.contiguous(), lists, float(scale),
                                   bool(causal), key_mask)
