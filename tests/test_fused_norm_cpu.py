"""residual_rms_norm on CPU fp32 against `x + delta` followed by rms_norm.

The eager branch of the fused op must compute exactly the composition it
replaces, so CPU models are unchanged: outputs bit-equal, gradients to
rtol 1e-6 (the two graphs add the same gradient terms in a different order).
"""
import pytest
import torch

from fengshen_amd.ops import functional as F
from fengshen_amd.parallel.random import checkpoint

EPS = 1e-6
H = 48


def _inputs(with_delta=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(3, 5, H, generator=g).requires_grad_(True)
    d = torch.randn(3, 5, H, generator=g).requires_grad_(True) \
        if with_delta else None
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).requires_grad_(True)
    g_res = torch.randn(3, 5, H, generator=g)
    g_h = torch.randn(3, 5, H, generator=g)
    return x, d, w, g_res, g_h


def _reference(x, d, w):
    res = x if d is None else x + d
    return res, F.rms_norm(res, w, EPS)


def _run(fn, with_delta, use_res, use_h):
    x, d, w, g_res, g_h = _inputs(with_delta)
    res, h = fn(x, d, w)
    loss = 0.0
    if use_res:
        loss = loss + (res * g_res).sum()
    if use_h:
        loss = loss + (h * g_h).sum()
    loss.backward()
    return (res.detach(), h.detach(), x.grad,
            None if d is None else d.grad, w.grad)


def _fused(x, d, w):
    return F.residual_rms_norm(x, d, w, EPS)


def _compare(got, ref):
    assert torch.equal(got[0], ref[0]), "res differs"
    assert torch.equal(got[1], ref[1]), "h differs"
    for name, a, r in zip(("g_x", "g_delta", "g_w"), got[2:], ref[2:]):
        if r is None:
            assert a is None or not a.any(), name
            continue
        assert a is not None, name
        torch.testing.assert_close(a, r, rtol=1e-6, atol=1e-6, msg=name)


@pytest.mark.parametrize("with_delta", [True, False])
@pytest.mark.parametrize("use_res,use_h", [(True, True), (True, False),
                                            (False, True)])
def test_matches_add_then_norm(with_delta, use_res, use_h):
    _compare(_run(_fused, with_delta, use_res, use_h),
             _run(_reference, with_delta, use_res, use_h))


def test_res_aliases_x_without_delta():
    x, _, w, _, _ = _inputs(False)
    res, _h = F.residual_rms_norm(x, None, w, EPS)
    assert res.data_ptr() == x.data_ptr()


@pytest.mark.parametrize("with_delta", [True, False])
def test_inside_checkpoint(with_delta):
    def block(fn):
        def run(x, d, w):
            def body(x_, w_, *rest):
                res, h = fn(x_, rest[0] if rest else None, w_)
                return res + 2.0 * h
            args = (x, w) + ((d,) if d is not None else ())
            out = checkpoint(body, *args)
            return out, out
        return run

    x, d, w, g_res, _ = _inputs(with_delta)
    outs = []
    for fn in (_fused, _reference):
        xs = [t.detach().clone().requires_grad_(True) if t is not None
              else None for t in (x, d, w)]
        out, _ = block(fn)(*xs)
        (out * g_res).sum().backward()
        outs.append((out.detach(),) + tuple(
            None if t is None else t.grad for t in xs))
    assert torch.equal(outs[0][0], outs[1][0])
    for name, a, r in zip(("g_x", "g_delta", "g_w"), outs[0][1:], outs[1][1:]):
        if r is None:
            assert a is None
            continue
        torch.testing.assert_close(a, r, rtol=1e-6, atol=1e-6, msg=name)


def test_env_switch_composes_old_ops(monkeypatch):
    monkeypatch.setenv("FENGSHEN_FUSED_NORM", "0")
    _compare(_run(_fused, True, True, True),
             _run(_reference, True, True, True))
