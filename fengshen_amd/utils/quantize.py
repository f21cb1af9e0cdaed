"""Weight-only int8 and int4 quantization for inference.

Behavioral parity: reference examples/ziya_inference (bitsandbytes
Linear8bitLt conversion, hf_quantizatin_inference.py:9-10; llama.cpp q4/q5
path) — MI355X equivalent: W8A16 per-channel symmetric quantization
(W8Linear) and W4A16 symmetric quantization with a bf16 scale per group of
128 input features (W4Linear).  Activations are never quantised; decode is a
weight stream, so int8 halves the HBM traffic of bf16 and int4 halves it
again.
"""
from __future__ import annotations

import torch
import torch.nn as nn


class W8Linear(nn.Module):
    """int8 weight + per-output-channel fp scale; bf16 activations.

    Up to 16 rows of bf16 activations on the GPU stay in int8 in HBM:
    ops.functional.decode_linear_route picks w8_gemv or, for 2..16 rows,
    decode_gemm (FENGSHEN_DECODE_GEMM = auto | 0 | 1).  Everything else
    dequantises the weight and calls F.linear."""

    def __init__(self, weight: torch.Tensor, bias=None):
        super().__init__()
        w = weight.detach().float()
        scale = w.abs().amax(dim=1, keepdim=True) / 127.0
        scale = scale.clamp(min=1e-8)
        qw = torch.round(w / scale).clamp(-127, 127).to(torch.int8)
        self.register_buffer("qweight", qw)
        self.register_buffer("scale", scale.to(torch.float32))
        self.bias = None
        if bias is not None:
            self.register_buffer("bias_buf", bias.detach().clone())
            self.bias = True
        self.out_features, self.in_features = weight.shape

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from fengshen_amd.ops import use_hip, get_ext
        from fengshen_amd.ops.functional import (
            decode_gemm_mode, decode_linear_route)
        rows = x.numel() // x.shape[-1]
        route = decode_linear_route(
            rows, x.shape[-1], torch.int8,
            use_hip(x) and x.dtype == torch.bfloat16,
            torch.is_grad_enabled(), decode_gemm_mode())
        if route != "library":
            # decode path: the weights stay int8 in HBM
            x2 = x.reshape(rows, -1).contiguous()
            scale = self.scale.view(-1)
            if route == "gemv":
                y = get_ext().w8_gemv(self.qweight, scale, x2)
            else:
                y = get_ext().decode_gemm(self.qweight, x2, scale)
            y = y.view(*x.shape[:-1], self.out_features)
        else:
            w = (self.qweight.to(x.dtype) * self.scale.to(x.dtype))
            y = torch.nn.functional.linear(x, w)
        if self.bias:
            y = y + self.bias_buf.to(x.dtype)
        return y

    def extra_repr(self):
        return f"in={self.in_features}, out={self.out_features}, w8"


W4_GROUP = 128   # input features per scale
_W4_ROW_PAD = 64  # output features are padded to whole 4-tile blocks
# nibble position p of a dword holds k offset 2 (p % 4) + p / 4, so byte b
# has k offsets _W4_LO[b] (low nibble) and _W4_HI[b] (high nibble)
_W4_LO, _W4_HI = (0, 4, 1, 5), (2, 6, 3, 7)


def pack_int4(q: torch.Tensor, scales: torch.Tensor):
    """q [out, K] integers in [-7, 7], scales [out, K/128] bf16 ->
    (qweight uint8 [out_pad/16, K/128, 64, 16], scales bf16 [K/128, out_pad])
    in the order decode_gemm_w4.hip streams (out_pad = out rounded up to 64).

    The 16 bytes of tile t, group G, lane 16 g + r hold row 16 t + r at
    k = 128 G + 32 g + 0..31 as four little-endian dwords of 8 k each,
    offset-binary (u = q + 8); within a dword nibble position p holds k
    offset 2 (p % 4) + p / 4, so (dw >> 4 i) & 0x000F000F is the pair
    (2 i, 2 i + 1).  Pad rows have u = 8 and scale 0."""
    out, K = q.shape
    if K % W4_GROUP != 0 or K == 0:
        raise ValueError(f"in_features must be a multiple of {W4_GROUP}, "
                         f"got {K}")
    ng = K // W4_GROUP
    if scales.shape != (out, ng) or scales.dtype != torch.bfloat16:
        raise ValueError(f"scales must be bf16 [{out}, {ng}]")
    out_pad = -(-out // _W4_ROW_PAD) * _W4_ROW_PAD
    u = torch.full((out_pad, K), 8, dtype=torch.uint8, device=q.device)
    u[:out] = (q + 8).to(torch.uint8)
    u = u.view(out_pad // 16, 16, ng, 4, 4, 8)        # t, r, G, g, dword, e
    by = u[..., list(_W4_LO)] | (u[..., list(_W4_HI)] << 4)
    qweight = by.permute(0, 2, 3, 1, 4, 5).reshape(out_pad // 16, ng, 64, 16)
    sc = torch.zeros(ng, out_pad, dtype=torch.bfloat16, device=q.device)
    sc[:, :out] = scales.t()
    return qweight.contiguous(), sc


def unpack_int4(qweight: torch.Tensor, scales: torch.Tensor, out: int,
                dequant: bool = True):
    """Inverse of pack_int4.  -> the dequantised fp32 weight [out, K]
    (q * scale is exact in fp32), or with dequant=False the pair
    (q int8 [out, K], scales bf16 [out, K/128]) that was packed."""
    nt, ng = qweight.shape[:2]
    by = qweight.view(nt, ng, 4, 16, 4, 4)            # t, G, g, r, dword, b
    u = torch.empty(nt, ng, 4, 16, 4, 8, dtype=torch.uint8,
                    device=qweight.device)
    u[..., list(_W4_LO)] = by & 15
    u[..., list(_W4_HI)] = by >> 4
    q = (u.permute(0, 3, 1, 2, 4, 5).reshape(nt * 16, ng * W4_GROUP)[:out]
         .to(torch.int8) - 8)
    sc = scales[:, :out].t().contiguous()
    if not dequant:
        return q, sc
    return (q.float().view(out, ng, W4_GROUP)
            * sc.float()[:, :, None]).view(out, ng * W4_GROUP)


class W4Linear(nn.Module):
    """Symmetric int4 weights with a bf16 scale per (output feature, group of
    128 consecutive input features); bf16 activations.

    scale = amax(group) / 7 (at least 1e-8, rounded to bf16), q = round(w /
    scale) in [-7, 7]; the buffers are in pack_int4's order.  Up to 16 rows
    of bf16 activations on the GPU run decode_gemm_w4 (decode_gemm_w4.hip),
    which streams the 4-bit weights once (FENGSHEN_DECODE_GEMM = auto | 1);
    everything else, and mode 0, dequantises the weight and calls
    F.linear."""

    def __init__(self, weight: torch.Tensor, bias=None, group_size=W4_GROUP):
        super().__init__()
        if group_size != W4_GROUP:
            raise ValueError(f"W4Linear supports group_size={W4_GROUP} only, "
                             f"got {group_size}")
        out, K = weight.shape
        if K % W4_GROUP != 0 or K == 0:
            raise ValueError(f"W4Linear needs in_features % {W4_GROUP} == 0, "
                             f"got {K}")
        w = weight.detach().double().view(out, K // W4_GROUP, W4_GROUP)
        scale = (w.abs().amax(dim=2) / 7.0).clamp(min=1e-8).to(torch.bfloat16)
        q = torch.round(w / scale.double()[:, :, None]).clamp(-7, 7)
        qweight, scales = pack_int4(q.view(out, K).to(torch.int8), scale)
        self.register_buffer("qweight", qweight)
        self.register_buffer("scales", scales)
        self.bias = None
        if bias is not None:
            self.register_buffer("bias_buf", bias.detach().clone())
            self.bias = True
        self.out_features, self.in_features = out, K

    def dequantized(self) -> torch.Tensor:
        return unpack_int4(self.qweight, self.scales, self.out_features)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        from fengshen_amd.ops import use_hip, get_ext
        from fengshen_amd.ops.functional import (
            decode_gemm_mode, decode_linear_route)
        rows = x.numel() // x.shape[-1]
        route = decode_linear_route(
            rows, x.shape[-1], torch.uint8,
            use_hip(x) and x.dtype == torch.bfloat16,
            torch.is_grad_enabled(), decode_gemm_mode())
        if route == "decode_gemm_w4":
            # decode path: the weights stay 4-bit in HBM
            y = get_ext().decode_gemm_w4(
                self.qweight, self.scales, x.reshape(rows, -1).contiguous(),
                self.out_features)
            y = y.view(*x.shape[:-1], self.out_features)
        else:
            y = torch.nn.functional.linear(x, self.dequantized().to(x.dtype))
        if self.bias:
            y = y + self.bias_buf.to(x.dtype)
        return y

    def extra_repr(self):
        return f"in={self.in_features}, out={self.out_features}, w4g128"


_QUANT_TARGETS = ("qkv_proj", "out_proj", "gate_up_proj", "down_proj",
                  "fc_in", "fc_out", "lm_head")


def _quantize_model(model: nn.Module, targets, cls) -> nn.Module:
    from fengshen_amd.parallel.layers import (
        ColumnParallelLinear, RowParallelLinear)

    for name, module in model.named_children():
        if isinstance(module, (nn.Linear, ColumnParallelLinear,
                               RowParallelLinear)) and \
                any(t in name for t in targets):
            setattr(model, name, cls(module.weight,
                                     getattr(module, "bias", None)))
        else:
            _quantize_model(module, targets, cls)
    return model


def quantize_model_int8(model: nn.Module, targets=_QUANT_TARGETS) -> nn.Module:
    """Replace target Linear-like modules with W8Linear (in place)."""
    return _quantize_model(model, targets, W8Linear)


def quantize_model_int4(model: nn.Module, targets=_QUANT_TARGETS) -> nn.Module:
    """Replace target Linear-like modules with W4Linear (in place); their
    in_features must be multiples of 128."""
    return _quantize_model(model, targets, W4Linear)


def quantized_bytes(model: nn.Module) -> int:
    total = 0
    for p in model.parameters():
        total += p.numel() * p.element_size()
    for b in model.buffers():
        total += b.numel() * b.element_size()
    return total
