"""Packed-QKV attention path: strided v3 flash kernels, in-place rotary and
the ParallelAttention routing.

The strided entries run the same arithmetic on the same values as the
contiguous entries (only addresses differ), so every comparison here is
bit-exact (torch.equal).  The contiguous entries themselves are checked
against the fp32 oracle in test_ops_gpu.py.  All tests require an MI355X."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda",
                       dtype=torch.float32).to(torch.bfloat16)


def _views(buf, np_):
    """[b, s, >=3*np*d] packed buffer -> q, k, v as [b, np, s, d] views."""
    h = buf.shape[-1] // 3
    return [buf.narrow(2, i * h, h).unflatten(2, (np_, -1)).transpose(1, 2)
            for i in range(3)]


def _bhsd(x, np_):
    """[b, s, np*d] -> [b, np, s, d] view."""
    return x.unflatten(2, (np_, -1)).transpose(1, 2)


def _packed(b, s, np_, d, wide, seed=0):
    """Packed qkv values; with ``wide`` the tensor is a slice of a wider
    allocation (row stride > 3*np*d, base offset 8 elements), so the thirds
    of neighbouring rows are not adjacent in memory."""
    w = 3 * np_ * d
    if not wide:
        return _rand(b, s, w, seed=seed)
    pad = _rand(b, s, w + 24, seed=seed)
    return pad[:, :, 8:8 + w]


def _run_both(b, s, np_, d, causal, klens=None, wide=False):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    scale = 1.0 / math.sqrt(d)
    qkv = _packed(b, s, np_, d, wide)
    q, k, v = _views(qkv, np_)
    do_p = _packed(b, s, np_, d, wide, seed=1)[:, :, :np_ * d]  # strided dO
    do = _bhsd(do_p, np_)

    # contiguous reference entry on copies of the same values
    qc, kc, vc = q.contiguous(), k.contiguous(), v.contiguous()
    o_ref, lse_ref = ext.flash_attn_fwd_v3(qc, kc, vc, scale, causal, klens,
                                           0.0, 0)
    dq_ref, dk_ref, dv_ref = ext.flash_attn_bwd_v3(
        qc, kc, vc, o_ref, do.contiguous(), lse_ref, scale, causal, klens,
        0.0, 0)

    # strided entry: reads the packed buffer, writes O as [b, s, np*d] and
    # dq/dk/dv into the thirds of one packed gradient (NaN-prefilled so an
    # element the kernels skip cannot compare equal)
    o_p = torch.full((b, s, np_ * d), float("nan"), device="cuda",
                     dtype=torch.bfloat16)
    lse = ext.flash_attn_fwd_v3_strided(q, k, v, _bhsd(o_p, np_), scale,
                                        causal, klens)
    if wide:
        g_full = torch.full((b, s, 3 * np_ * d + 24), float("nan"),
                            device="cuda", dtype=torch.bfloat16)
        g_p = g_full[:, :, 8:8 + 3 * np_ * d]
    else:
        g_p = torch.full((b, s, 3 * np_ * d), float("nan"), device="cuda",
                         dtype=torch.bfloat16)
    dq, dk, dv = _views(g_p, np_)
    ext.flash_attn_bwd_v3_strided(q, k, v, _bhsd(o_p, np_), do, lse, dq, dk,
                                  dv, scale, causal, klens)
    torch.cuda.synchronize()

    assert torch.equal(_bhsd(o_p, np_), o_ref), "O differs"
    assert torch.equal(lse, lse_ref), "LSE differs"
    assert torch.equal(dq, dq_ref), "dq differs"
    assert torch.equal(dk, dk_ref), "dk differs"
    assert torch.equal(dv, dv_ref), "dv differs"
    if wide:  # nothing written outside the slice
        assert g_full[:, :, :8].isnan().all()
        assert g_full[:, :, 8 + 3 * np_ * d:].isnan().all()


@pytest.mark.parametrize("s", [64, 320])
def test_strided_matches_contiguous_d128_causal(s):
    # np=3 (odd): a wrong head stride shows.  s=64: one partial 256-row
    # block (clamping); s=320: multiple of 64, not of 256.
    _run_both(2, s, 3, 128, True)


def test_strided_slice_of_wider_allocation():
    _run_both(2, 320, 3, 128, True, wide=True)


def test_strided_d64_noncausal_klens():
    klens = torch.tensor([128, 70], device="cuda", dtype=torch.int32)
    _run_both(2, 128, 3, 64, False, klens=klens)


def test_strided_d96_causal():
    _run_both(2, 128, 3, 96, True)


@pytest.mark.parametrize("wide", [False, True])
def test_rope_inplace_matches_out_of_place(wide):
    from fengshen_amd.ops import get_ext
    from fengshen_amd.ops.functional import build_rope_cache
    ext = get_ext()
    b, np_, hn, s = 2, 3, 128, 64
    cos, sin = build_rope_cache(s, hn, device="cuda")
    for bwd in (False, True):
        qkv = _packed(b, s, np_, hn, wide, seed=3)
        before = qkv.clone()
        q, k, v = _views(qkv, np_)
        fn = ext.rope_bwd if bwd else ext.rope_fwd
        q_ref, k_ref = fn(q.contiguous(), k.contiguous(), cos, sin, 0)
        ext.rope_inplace(q, k, cos, sin, 0, bwd)
        torch.cuda.synchronize()
        assert torch.equal(q, q_ref)
        assert torch.equal(k, k_ref)
        assert torch.equal(v, _views(before, np_)[2]), "v third touched"
        assert not torch.equal(q, _views(before, np_)[0])  # did rotate


def _layer_run(packed, use_ckpt, bias):
    """One ParallelAttention forward+backward from a fixed seed; returns
    (out, dx, dWqkv, dWout)."""
    from fengshen_amd.models.layers import ParallelAttention
    from fengshen_amd.parallel.random import checkpoint
    old = os.environ.get("FENGSHEN_PACKED_ATTN")
    os.environ["FENGSHEN_PACKED_ATTN"] = "1" if packed else "0"
    try:
        torch.manual_seed(7)
        layer = ParallelAttention(384, 3, causal=True, rotary=True,
                                  bias=bias, max_positions=512,
                                  dtype=torch.bfloat16).cuda()
        x = _rand(2, 320, 384, seed=5).requires_grad_(True)
        gy = _rand(2, 320, 384, seed=6)
        out = checkpoint(layer, x) if use_ckpt else layer(x)
        out.backward(gy)
        torch.cuda.synchronize()
        return (out.detach(), x.grad, layer.qkv_proj.weight.grad,
                layer.out_proj.weight.grad)
    finally:
        if old is None:
            os.environ.pop("FENGSHEN_PACKED_ATTN", None)
        else:
            os.environ["FENGSHEN_PACKED_ATTN"] = old


# bias=True makes the projection output a view (addmm + view), the case in
# which autograd restricts in-place updates; bias=False is the LLaMA layout
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("use_ckpt", [False, True])
def test_layer_packed_equals_unpacked(use_ckpt, bias, monkeypatch):
    # prove the switch really routes: count packed-function calls
    from fengshen_amd.ops import flash
    calls = []
    orig = flash.packed_self_attention

    def counted(*a, **kw):
        calls.append(1)
        return orig(*a, **kw)

    monkeypatch.setattr(flash, "packed_self_attention", counted)
    new = _layer_run(True, use_ckpt, bias)
    n_packed = len(calls)
    ref = _layer_run(False, use_ckpt, bias)
    assert n_packed == (2 if use_ckpt else 1)  # recompute runs it again
    assert len(calls) == n_packed, "FENGSHEN_PACKED_ATTN=0 still ran packed"
    for name, a, r in zip(("out", "dx", "dWqkv", "dWout"), new, ref):
        assert a is not None and r is not None, name
        assert torch.equal(a, r), f"{name} differs"


def test_binding_rejects_bad_layout():
    """Host-side checks only: nothing is launched for a rejected call."""
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    b, s, np_, d = 1, 64, 2, 64
    qkv = _rand(b, s, 3 * np_ * d)
    q, k, v = _views(qkv, np_)
    o = torch.empty(b, s, np_ * d, device="cuda", dtype=torch.bfloat16)
    ov = _bhsd(o, np_)
    scale = 0.125
    # non-unit last stride
    wide = _rand(b, np_, s, 2 * d)
    with pytest.raises(RuntimeError, match="unit-stride"):
        ext.flash_attn_fwd_v3_strided(wide[..., ::2], k, v, ov, scale, True,
                                      None)
    # misaligned base offset (4 elements = 8 bytes)
    shifted = _rand(b, s, 3 * np_ * d + 8)[:, :, 4:4 + 3 * np_ * d]
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.flash_attn_fwd_v3_strided(*_views(shifted, np_), ov, scale, True,
                                      None)
    # q and v with different strides
    with pytest.raises(RuntimeError, match="share strides"):
        ext.flash_attn_fwd_v3_strided(q, k, v.contiguous(), ov, scale, True,
                                      None)
    cos = torch.ones(s, d, device="cuda")
    with pytest.raises(RuntimeError, match="unit-stride"):
        ext.rope_inplace(wide[..., ::2], wide[..., ::2], cos, cos, 0, False)
    with pytest.raises(RuntimeError, match="table too short"):
        ext.rope_inplace(q, k, cos, cos, 1, False)
