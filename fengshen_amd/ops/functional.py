"""Fused-op functional API: HIP kernel dispatch + eager oracles.

Each op mirrors a hot-path op the reference fuses (or left unfused):
  scaled_masked_softmax   — ref fused_kernels/scaled_masked_softmax.h (wave64 redesign)
  scaled_causal_softmax   — ref scaled_upper_triang_masked_softmax.h
  layer_norm              — ref layer_norm_cuda.cpp (vestigial apex LN, now real)
  rms_norm                — ref layers/norms.py:35-52 (fp32 variance)
  bias_gelu               — ref layers/activations.py:60-94 (jit fused)
  bias_dropout_add        — ref layers/fused_bias_dropout.py:44-55
  rotary (apply_rotary)   — ref layers/positional_embeddings.py:54-87
  swiglu                  — ref LLaMAParallelMLP silu(w1)*w3 (transformer.py:571-623)
  swiglu_mlp_residual     — the same MLP with its residual add as one node
  fused attention         — ref flash_attention.py (flash_attn v1 import)

The eager implementations double as numerics oracles in tests
(SURVEY.md §4 "fallback-path pattern").
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch

from fengshen_amd.ops import use_hip, get_ext


# ---------------------------------------------------------------------------
# softmax family
# ---------------------------------------------------------------------------
def eager_scaled_masked_softmax(x: torch.Tensor, mask: Optional[torch.Tensor],
                                scale: float) -> torch.Tensor:
    """x [b, np, sq, sk]; mask [b or 1, 1, sq, sk] (True = MASKED, like the
    reference's uint8 pad mask); fp32 accumulation."""
    y = x.float() * scale
    if mask is not None:
        y = y.masked_fill(mask.bool(), -10000.0)
    return torch.softmax(y, dim=-1).to(x.dtype)


def eager_scaled_causal_softmax(x: torch.Tensor, scale: float) -> torch.Tensor:
    """x [attn_batches, sq, sk] with sq == sk; causal mask by index compare."""
    sq, sk = x.shape[-2], x.shape[-1]
    y = x.float() * scale
    causal = torch.ones(sq, sk, dtype=torch.bool, device=x.device).triu(1)
    y = y.masked_fill(causal, -10000.0)
    return torch.softmax(y, dim=-1).to(x.dtype)


class _ScaledMaskedSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, scale):
        if use_hip(x):
            out = get_ext().scaled_masked_softmax_fwd(x.contiguous(), mask,
                                                      scale)
        else:
            out = eager_scaled_masked_softmax(x, mask, scale)
        ctx.save_for_backward(out)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (out,) = ctx.saved_tensors
        if use_hip(out):
            grad_in = get_ext().scaled_softmax_bwd(grad_out.contiguous(), out,
                                                   ctx.scale)
        else:
            g = grad_out.float() * out.float()
            grad_in = ((g - out.float() * g.sum(dim=-1, keepdim=True))
                       * ctx.scale).to(out.dtype)
        return grad_in, None, None


class _ScaledCausalSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, scale):
        if use_hip(x):
            out = get_ext().scaled_causal_softmax_fwd(x.contiguous(), scale)
        else:
            out = eager_scaled_causal_softmax(x, scale)
        ctx.save_for_backward(out)
        ctx.scale = scale
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (out,) = ctx.saved_tensors
        if use_hip(out):
            grad_in = get_ext().scaled_softmax_bwd(grad_out.contiguous(), out,
                                                   ctx.scale)
        else:
            g = grad_out.float() * out.float()
            grad_in = ((g - out.float() * g.sum(dim=-1, keepdim=True))
                       * ctx.scale).to(out.dtype)
        return grad_in, None


def scaled_masked_softmax(x, mask, scale: float = 1.0):
    return _ScaledMaskedSoftmax.apply(x, mask, scale)


def scaled_causal_softmax(x, scale: float = 1.0):
    return _ScaledCausalSoftmax.apply(x, scale)


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------
def eager_rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float):
    """fp32 variance like the reference RMSNorm (norms.py:35-52)."""
    x32 = x.float()
    var = x32.pow(2).mean(-1, keepdim=True)
    y = x32 * torch.rsqrt(var + eps)
    return (weight.float() * y).to(x.dtype)


def fused_norm_enabled() -> bool:
    """FENGSHEN_FUSED_NORM=0 forces the LDS-staged norm kernels and the
    separate residual adds (bias_dropout_add + rms_norm)."""
    return os.environ.get("FENGSHEN_FUSED_NORM", "1") != "0"


def _rms_norm_bwd_eager(g_h, x, weight, invrms):
    x32 = x.float()
    g32 = g_h.float()
    w32 = weight.float()
    xhat = x32 * invrms
    gy_w = g32 * w32
    # d/dx: invrms * (gy_w - xhat * mean(gy_w * xhat))
    mean_term = (gy_w * xhat).mean(-1, keepdim=True)
    gx = (invrms * (gy_w - xhat * mean_term)).to(x.dtype)
    gw = (g32 * xhat).sum(dim=tuple(range(x.dim() - 1))).to(weight.dtype)
    return gx, gw


class _RMSNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        ctx.fused = fused_norm_enabled()
        if use_hip(x):
            x = x.contiguous()  # kernel reads rows as flat vectors
            if ctx.fused:
                _, out, invrms = get_ext().residual_rms_norm_fwd(
                    x, None, weight, eps)
            else:
                out, invrms = get_ext().rms_norm_fwd(x, weight, eps)
        else:
            x32 = x.float()
            var = x32.pow(2).mean(-1, keepdim=True)
            invrms = torch.rsqrt(var + eps)
            out = (x32 * invrms * weight.float()).to(x.dtype)
        ctx.save_for_backward(x, weight, invrms)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, invrms = ctx.saved_tensors
        if use_hip(x):
            if ctx.fused:
                gx, gw = get_ext().residual_rms_norm_bwd(
                    grad_out.contiguous(), None, x, weight, invrms)
            else:
                gx, gw = get_ext().rms_norm_bwd(grad_out.contiguous(), x,
                                                weight, invrms)
            return gx, gw, None
        gx, gw = _rms_norm_bwd_eager(grad_out, x, weight, invrms)
        return gx, gw, None


def rms_norm(x, weight, eps: float = 1e-6):
    return _RMSNorm.apply(x, weight, eps)


class _ResidualRMSNorm(torch.autograd.Function):
    """(res, h) = (x + delta, rms_norm(x + delta)) in one pass; the backward
    folds the gradient arriving at ``res`` into the norm's input gradient.

    ``res`` is rounded to x's dtype before it is normalised, so both outputs
    equal a torch add followed by rms_norm; with delta=None ``res`` is x.
    The backward rounds the norm's input gradient to x's dtype before adding
    g_res, as the separate add did."""

    @staticmethod
    def forward(ctx, x, delta, weight, eps):
        ctx.set_materialize_grads(False)
        ctx.has_delta = delta is not None
        if use_hip(x):
            xc = x.contiguous()  # kernel reads rows as flat vectors
            dc = delta.contiguous() if ctx.has_delta else None
            res, h, invrms = get_ext().residual_rms_norm_fwd(
                xc, dc, weight, eps)
            if not ctx.has_delta:
                res = x
        else:
            res = x + delta if ctx.has_delta else x
            r32 = res.float()
            invrms = torch.rsqrt(r32.pow(2).mean(-1, keepdim=True) + eps)
            h = (r32 * invrms * weight.float()).to(x.dtype)
        ctx.save_for_backward(res, weight, invrms)
        return res, h

    @staticmethod
    def backward(ctx, g_res, g_h):
        res, weight, invrms = ctx.saved_tensors
        if g_h is None:
            g, gw = g_res, None
        elif use_hip(res):
            g, gw = get_ext().residual_rms_norm_bwd(
                g_h.contiguous(), None if g_res is None else g_res.contiguous(),
                res.contiguous(), weight, invrms)
        else:
            g, gw = _rms_norm_bwd_eager(g_h, res, weight, invrms)
            if g_res is not None:
                g = g + g_res
        return g, (g if ctx.has_delta else None), gw, None


def residual_rms_norm(x, delta, weight, eps: float = 1e-6):
    """-> (res, h): res = x + delta (x itself when delta is None) and
    h = rms_norm(res).  FENGSHEN_FUSED_NORM=0 composes the same result from
    bias_dropout_add and rms_norm."""
    if not fused_norm_enabled():
        res = x if delta is None else bias_dropout_add(delta, None, x, 0.0,
                                                       False)
        return res, rms_norm(res, weight, eps)
    return _ResidualRMSNorm.apply(x, delta, weight, eps)


def eager_layer_norm(x, weight, bias, eps):
    return torch.nn.functional.layer_norm(
        x.float(), (x.shape[-1],), weight.float(),
        bias.float() if bias is not None else None, eps).to(x.dtype)


class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        if use_hip(x):
            x = x.contiguous()  # kernel reads rows as flat vectors
            out, mean, invstd = get_ext().layer_norm_fwd(x, weight, bias, eps)
            ctx.save_for_backward(x, weight, mean, invstd)
            ctx.has_bias = bias is not None
            return out
        ctx.eps = eps
        ctx.fallback = True
        x32 = x.float()
        mean = x32.mean(-1, keepdim=True)
        var = x32.var(-1, unbiased=False, keepdim=True)
        invstd = torch.rsqrt(var + eps)
        out = (x32 - mean) * invstd * weight.float()
        if bias is not None:
            out = out + bias.float()
        ctx.save_for_backward(x, weight, mean, invstd)
        ctx.has_bias = bias is not None
        return out.to(x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        x, weight, mean, invstd = ctx.saved_tensors
        if use_hip(x):
            gx, gw, gb = get_ext().layer_norm_bwd(
                grad_out.contiguous(), x, weight, mean, invstd)
            return gx, gw, (gb if ctx.has_bias else None), None
        x32 = x.float()
        g32 = grad_out.float()
        w32 = weight.float()
        xhat = (x32 - mean) * invstd
        gy_w = g32 * w32
        n = x.shape[-1]
        gx = (invstd * (gy_w - gy_w.mean(-1, keepdim=True)
                        - xhat * (gy_w * xhat).mean(-1, keepdim=True))).to(x.dtype)
        dims = tuple(range(x.dim() - 1))
        gw = (g32 * xhat).sum(dims).to(weight.dtype)
        gb = g32.sum(dims).to(weight.dtype) if ctx.has_bias else None
        return gx, gw, gb, None


def layer_norm(x, weight, bias=None, eps: float = 1e-5):
    return _LayerNorm.apply(x, weight, bias, eps)


# ---------------------------------------------------------------------------
# activations
# ---------------------------------------------------------------------------
def eager_gelu(x):
    """tanh-approx GELU (reference bias_gelu, activations.py:60-77)."""
    return x * 0.5 * (1.0 + torch.tanh(0.79788456 * x * (1 + 0.044715 * x * x)))


class _BiasGelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias):
        ctx.save_for_backward(x, bias)
        if use_hip(x):
            return get_ext().bias_gelu_fwd(x, bias)
        y = x.float() + bias.float()
        return eager_gelu(y).to(x.dtype)

    @staticmethod
    def backward(ctx, grad_out):
        x, bias = ctx.saved_tensors
        if use_hip(x):
            gx = get_ext().bias_gelu_bwd(grad_out.contiguous(), x, bias)
        else:
            y = (x.float() + bias.float())
            t = torch.tanh(0.79788456 * y * (1 + 0.044715 * y * y))
            ff = 0.5 * y * ((1 - t * t) * (0.79788456 + 0.1070322243 * y * y)) \
                + 0.5 * (1 + t)
            gx = (ff * grad_out.float()).to(x.dtype)
        gb = gx.sum(dim=tuple(range(gx.dim() - 1))).to(bias.dtype)
        return gx, gb


def bias_gelu(x, bias):
    return _BiasGelu.apply(x, bias)


def eager_swiglu(gate, up):
    return torch.nn.functional.silu(gate.float()).to(gate.dtype) * up


class _SwiGLU(torch.autograd.Function):
    """fused silu(gate) * up over a [..., 2h] packed tensor (gate|up)."""

    @staticmethod
    def forward(ctx, packed):
        ctx.save_for_backward(packed)
        if use_hip(packed):
            return get_ext().swiglu_fwd(packed)
        gate, up = packed.chunk(2, dim=-1)
        return eager_swiglu(gate, up)

    @staticmethod
    def backward(ctx, grad_out):
        (packed,) = ctx.saved_tensors
        if use_hip(packed):
            return get_ext().swiglu_bwd(grad_out.contiguous(), packed)
        gate, up = packed.chunk(2, dim=-1)
        g32, u32, go = gate.float(), up.float(), grad_out.float()
        sig = torch.sigmoid(g32)
        silu = g32 * sig
        dgate = go * u32 * sig * (1 + g32 * (1 - sig))
        dup = go * silu
        return torch.cat([dgate, dup], dim=-1).to(packed.dtype)


def swiglu(packed):
    return _SwiGLU.apply(packed)


class _BiasDropoutAdd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, bias, residual, p, training):
        if not training or p == 0.0:
            ctx.p = 0.0
            ctx.save_for_backward(torch.tensor([]))
            y = x if bias is None else x + bias
            ctx.has_bias = bias is not None
            return y + residual
        keep = 1.0 - p
        mask = (torch.rand_like(x, dtype=torch.float32) < keep)
        y = x if bias is None else x + bias
        out = y * mask.to(x.dtype) / keep + residual
        ctx.p = p
        ctx.has_bias = bias is not None
        ctx.save_for_backward(mask)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.p == 0.0:
            gb = (grad_out.sum(dim=tuple(range(grad_out.dim() - 1)))
                  if ctx.has_bias else None)
            return grad_out, gb, grad_out, None, None
        (mask,) = ctx.saved_tensors
        keep = 1.0 - ctx.p
        gx = grad_out * mask.to(grad_out.dtype) / keep
        gb = gx.sum(dim=tuple(range(gx.dim() - 1))) if ctx.has_bias else None
        return gx, gb, grad_out, None, None


def bias_dropout_add(x, bias, residual, p: float, training: bool):
    return _BiasDropoutAdd.apply(x, bias, residual, p, training)


def fused_mlp_enabled() -> bool:
    """FENGSHEN_FUSED_MLP=0 keeps the SwiGLU MLP and its residual add as
    separate autograd nodes (linear, swiglu, linear, bias_dropout_add)."""
    return os.environ.get("FENGSHEN_FUSED_MLP", "1") != "0"


def _unused_output_like(t: torch.Tensor) -> torch.Tensor:
    """What swiglu_mlp_residual returns under output_unused=True: the right
    shape and dtype, contents unspecified.  Nothing may read it."""
    return torch.empty_like(t)


def _swiglu_bwd_act_eager(d_act, packed):
    """-> (d_packed, act) with the formulas of _SwiGLU's eager path."""
    gate, up = packed.chunk(2, dim=-1)
    g32, u32, go = gate.float(), up.float(), d_act.float()
    sig = torch.sigmoid(g32)
    dgate = go * u32 * sig * (1 + g32 * (1 - sig))
    dup = go * (g32 * sig)
    return (torch.cat([dgate, dup], dim=-1).to(packed.dtype),
            eager_swiglu(gate, up))


class _SwiGLUMLPResidual(torch.autograd.Function):
    """residual + down(swiglu(gate_up(h2))) as one node.

    Saves h2, packed = h2 @ w_gate_up^T and the two weights; act =
    silu(gate) * up is rebuilt in the backward by the kernel that already
    reads packed.  The backward needs none of the forward's outputs, so with
    output_unused=True the forward stops after packed."""

    @staticmethod
    def forward(ctx, h2, residual, w_gate_up, w_down, output_unused):
        packed = torch.nn.functional.linear(h2, w_gate_up)
        ctx.save_for_backward(h2, packed, w_gate_up, w_down)
        if output_unused:
            return _unused_output_like(residual)
        if use_hip(packed):
            act = get_ext().swiglu_fwd(packed)
        else:
            act = eager_swiglu(*packed.chunk(2, dim=-1))
        return torch.nn.functional.linear(act, w_down) + residual

    @staticmethod
    def backward(ctx, g):
        h2, packed, w_gate_up, w_down = ctx.saved_tensors
        g2d = g.reshape(-1, g.shape[-1])
        packed2d = packed.view(-1, packed.shape[-1])
        h2_2d = h2.reshape(-1, h2.shape[-1])
        # the GEMMs F.linear's autograd issues, on the same operands
        d_act = g2d.mm(w_down)
        if use_hip(packed):
            # act overwrites d_act in place
            d_packed, act = get_ext().swiglu_bwd_act(d_act, packed2d, d_act)
        else:
            d_packed, act = _swiglu_bwd_act_eager(d_act, packed2d)
        del d_act
        d_w_down = g2d.t().mm(act) if ctx.needs_input_grad[3] else None
        del act
        d_w_gate_up = d_packed.t().mm(h2_2d) if ctx.needs_input_grad[2] \
            else None
        d_h2 = d_packed.mm(w_gate_up).view(h2.shape) \
            if ctx.needs_input_grad[0] else None
        return d_h2, g, d_w_gate_up, d_w_down, None


def swiglu_mlp_residual(h2, residual, w_gate_up, w_down,
                        output_unused: bool = False):
    """residual + linear(swiglu(linear(h2, w_gate_up)), w_down): the bias-free
    SwiGLU MLP with its residual add (hidden dropout inactive).

    output_unused=True is the caller's promise that nobody reads the result,
    as when an activation-checkpoint recompute re-runs a layer only to
    rebuild what the backward saved.  The down projection and the add are
    then skipped and the returned tensor has residual's shape and dtype but
    unspecified contents; gradients are the same either way."""
    return _SwiGLUMLPResidual.apply(h2, residual, w_gate_up, w_down,
                                    output_unused)


# FENGSHEN_DECODE_GEMM=auto: from this many rows up to 16, a bias-free bf16
# decode linear runs decode_gemm (decode_gemm.hip) instead of hipBLASLt
# (bf16 weights) or w8_gemv (int8 weights); None = never under auto.  Set
# from scripts/decode_gemm_bench.py to the smallest measured row count from
# which decode_gemm wins at all five 13B shapes (docs/KERNELS.md,
# "decode_gemm.hip"), and never below 3: one-row calls and the two-row calls
# of the earlier decode tests keep the kernels they always ran.
# Measured: int8 wins at every shape from 4 rows (2-6x at 8 and 16; at 2 rows
# it loses at 5120 x 5120); bf16 loses to hipBLASLt at 8 and 16 rows at four
# of the five shapes, so auto never routes bf16 weights to it.
_DECODE_GEMM_MIN_ROWS = {torch.bfloat16: None, torch.int8: 4}


def decode_gemm_mode() -> str:
    mode = os.environ.get("FENGSHEN_DECODE_GEMM", "auto")
    if mode not in ("auto", "0", "1"):
        raise ValueError("FENGSHEN_DECODE_GEMM must be auto, 0 or 1, "
                         f"got {mode!r}")
    return mode


def decode_linear_route(rows: int, in_features: int, weight_dtype,
                        on_gpu: bool, grad_enabled: bool, mode: str) -> str:
    """Which kernel a bias-free linear on bf16 activations runs:

    "gemv"         bf16_gemv (bf16 weights, one row) or w8_gemv (int8
                   weights, up to 16 rows): what ran before decode_gemm
    "decode_gemm"  the MFMA weight-streaming kernel, 2..16 rows, K % 64 == 0
    "decode_gemm_w4"  the split-K MFMA kernel for int4 weights (weight_dtype
                   torch.uint8, W4Linear), 1..16 rows, K % 128 == 0
    "library"      F.linear, or the dequantised matmul for int8 and int4
                   weights

    on_gpu means the HIP path is usable for the call (use_hip) and the
    activations are bf16.  mode is FENGSHEN_DECODE_GEMM: "0" never picks
    decode_gemm or decode_gemm_w4, "1" picks them wherever they can run,
    "auto" takes decode_gemm from _DECODE_GEMM_MIN_ROWS[weight_dtype] rows
    and decode_gemm_w4 always (int4 weights have no other kernel).  This is
    the only place that decides."""
    if weight_dtype == torch.uint8:
        if on_gpu and not grad_enabled and 1 <= rows <= 16 and \
                in_features % 128 == 0 and mode != "0":
            return "decode_gemm_w4"
        return "library"
    w8 = weight_dtype == torch.int8
    if not on_gpu or not (w8 or weight_dtype == torch.bfloat16):
        return "library"
    if not w8 and grad_enabled:
        return "library"
    if in_features % 16 != 0:
        return "library"
    if 2 <= rows <= 16 and in_features % 64 == 0 and not grad_enabled:
        min_rows = _DECODE_GEMM_MIN_ROWS[weight_dtype]
        if mode == "1" or (mode == "auto" and min_rows is not None
                           and rows >= min_rows):
            return "decode_gemm"
    if (rows <= 16) if w8 else (rows == 1):
        return "gemv"
    return "library"


def linear(x: torch.Tensor, weight: torch.Tensor,
           bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear with two decode fast paths for bias-free bf16 inference
    calls, chosen by decode_linear_route: one row runs the bf16 GEMV
    kernel, 2..16 rows can run decode_gemm, the MFMA weight-streaming
    kernel (FENGSHEN_DECODE_GEMM = auto | 0 | 1); both stream the weight
    matrix once instead of going through hipBLASLt's skinny-M GEMM tiles.
    F.linear everywhere else (training, CPU, other dtypes, a bias), so
    autograd semantics are unchanged."""
    if bias is None and x.shape[-1] == weight.shape[1]:
        rows = x.numel() // x.shape[-1]
        route = decode_linear_route(
            rows, weight.shape[1], weight.dtype,
            use_hip(x) and x.dtype == torch.bfloat16,
            torch.is_grad_enabled(), decode_gemm_mode())
        if route == "gemv":
            y = get_ext().bf16_gemv(weight.contiguous(), x.contiguous())
            return y.view(*x.shape[:-1], weight.shape[0])
        if route == "decode_gemm":
            y = get_ext().decode_gemm(weight.contiguous(), x.contiguous())
            return y.view(*x.shape[:-1], weight.shape[0])
    return torch.nn.functional.linear(x, weight, bias)


# ---------------------------------------------------------------------------
# rotary embedding
# ---------------------------------------------------------------------------
def build_rope_cache(seq_len: int, dim: int, base: float = 10000.0,
                     device=None, dtype=torch.float32):
    """Host-precomputed cos/sin tables (guide Appendix B: no on-device trig)."""
    inv_freq = 1.0 / (base ** (torch.arange(0, dim, 2, device=device,
                                            dtype=torch.float32) / dim))
    t = torch.arange(seq_len, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _rotate_half(x):
    x1, x2 = x.chunk(2, dim=-1)
    return torch.cat((-x2, x1), dim=-1)


def eager_apply_rotary(q, k, cos, sin, offset: int = 0):
    """q,k [b, np, s, hn]; cos/sin [max_s, hn]."""
    s = q.shape[-2]
    c = cos[offset:offset + s].to(q.dtype)
    si = sin[offset:offset + s].to(q.dtype)
    q_out = q * c + _rotate_half(q) * si
    k_out = k * c + _rotate_half(k) * si
    return q_out, k_out


class _ApplyRotary(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, offset):
        ctx.save_for_backward(cos, sin)
        ctx.offset = offset
        if use_hip(q):
            return tuple(get_ext().rope_fwd(q.contiguous(), k.contiguous(),
                                            cos, sin, offset))
        return eager_apply_rotary(q, k, cos, sin, offset)

    @staticmethod
    def backward(ctx, gq, gk):
        cos, sin = ctx.saved_tensors
        offset = ctx.offset
        # rotation is orthogonal: grad = rotate by -theta
        if use_hip(gq):
            gq_out, gk_out = get_ext().rope_bwd(gq.contiguous(), gk.contiguous(),
                                                cos, sin, offset)
            return gq_out, gk_out, None, None, None
        s = gq.shape[-2]
        c = cos[offset:offset + s].to(gq.dtype)
        si = sin[offset:offset + s].to(gq.dtype)
        gq_out = gq * c - _rotate_half(gq * si)
        gk_out = gk * c - _rotate_half(gk * si)
        return gq_out, gk_out, None, None, None


def apply_rotary(q, k, cos, sin, offset: int = 0):
    return _ApplyRotary.apply(q, k, cos, sin, offset)


# ---------------------------------------------------------------------------
# attention (composite; flash HIP kernel replaces this on GPU)
# ---------------------------------------------------------------------------
def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
              causal: bool = False, mask: Optional[torch.Tensor] = None,
              dropout_p: float = 0.0, training: bool = False,
              scale: Optional[float] = None,
              kstart: Optional[torch.Tensor] = None,
              route=None) -> torch.Tensor:
    """q: [b, np, sq, hn], k,v: [b, nkv, sk, hn] -> context [b, np, sq, hn].

    nkv < np is grouped-query attention (np % nkv == 0, query head j uses
    KV head j // (np / nkv)); where the grouped-query kernels do not cover
    the call, K/V are expanded to np heads and autograd sums the group's
    gradients.

    Which kernels run -- flash, or hipBLASLt bmm + the fused softmax; on the
    CPU the eager oracle -- is decided by ops.flash.route_attention alone
    (table: docs/KERNELS.md, "Attention routing").  ``route`` is for a
    caller that has already asked it for exactly this call: the decision is
    then taken as given and the mask is not looked at again.

    kstart (int32 [b, s], causal self-attention only): row i sees keys
    kstart[i] <= j <= i (ops/flash.py).  Callers that have it pass it
    instead of, or next to, the dense mask it stands for; a causal mask
    given without it is converted when it is of that form.  Shapes the
    kstart kernels do not cover run under the dense mask as before.
    """
    from fengshen_amd.ops.flash import (
        expand_kv, flash_attention, route_attention)
    b, np_, sq, hn = q.shape
    sk = k.shape[-2]
    if scale is None:
        scale = 1.0 / math.sqrt(hn)
    drop = dropout_p if training else 0.0
    if route is None:
        route = route_attention(
            on_gpu=use_hip(q), dtype=q.dtype, heads=np_, kv_heads=k.shape[1],
            sq=sq, sk=sk, head_dim=hn, causal=causal, mask=mask,
            kstart=kstart, dropout_p=drop)
    if route.expand_kv:
        k, v = expand_kv(k, np_), expand_kv(v, np_)
    if route.path == "flash":
        return flash_attention(q, k, v, scale, causal=causal,
                               klens=route.klens, dropout_p=drop,
                               kstart=route.kstart)
    mask = route.mask
    # bmm path: scores in [b*np, sq, sk]
    q2 = q.reshape(b * np_, sq, hn)
    k2 = k.reshape(b * np_, sk, hn)
    scores = torch.bmm(q2, k2.transpose(1, 2)).view(b, np_, sq, sk)
    if causal and sq == sk and mask is None:
        probs = scaled_causal_softmax(scores.view(b * np_, sq, sk), scale)
        probs = probs.view(b, np_, sq, sk)
    else:
        m = mask
        if causal:
            # Rectangular causal for chunked prefill (sq < sk with a KV
            # cache): query i sits at global position (sk - sq + i), so key
            # j is visible iff j <= sk - sq + i.
            cm = torch.ones(sq, sk, dtype=torch.bool,
                            device=q.device).triu(1 + sk - sq)
            m = cm if mask is None else (mask.bool() | cm)
        probs = scaled_masked_softmax(scores, m, scale)
    if dropout_p > 0.0 and training:
        from fengshen_amd.parallel.random import get_rng_tracker
        with get_rng_tracker().fork():
            probs = torch.nn.functional.dropout(probs, p=dropout_p)
    ctx = torch.bmm(probs.view(b * np_, sq, sk), v.reshape(b * np_, sk, hn))
    return ctx.view(b, np_, sq, hn)
