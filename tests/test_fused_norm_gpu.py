"""Register-resident residual RMSNorm kernels against an fp64 oracle and
against the composition they replace (LDS-staged norm kernels + torch add,
selected with FENGSHEN_FUSED_NORM=0).

Oracle: fp64 torch with the kernels' rounding points modelled — the norm is
taken of the sum already rounded to the tensor dtype, and the backward rounds
the norm's input gradient to the tensor dtype before the residual gradient is
added.  Error measure: max |a - ref| / max(1, max |ref|), as test_ops_gpu's
_close.  All tests require an MI355X."""
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = 1e-6

# (rows, H, dispatch branch).  "reg<V>" = register-resident kernels with V
# vectors per thread, "lds" = LDS-staged fallback.  4099 rows is above both
# grid caps (2048 forward, 1024 backward), so blocks loop over several rows
# and accumulate several rows into one weight-gradient partial.
SHAPES = [
    (1, 8, "lds"),
    (5, 200, "lds"),
    (3, 512, "reg1"),
    (5, 768, "reg1"),
    (7, 1024, "reg1"),
    (3, 2048, "reg1"),
    (3, 4096, "reg2"),
    (33, 5120, "reg3"),
    (3, 8192, "reg4"),
    (4099, 512, "reg1"),
    (4099, 5120, "reg3"),
]
ALL_BRANCHES = {"lds", "reg1", "reg2", "reg3", "reg4"}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


@pytest.fixture(autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"


def _rand(*shape, dtype=torch.bfloat16, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda",
                       dtype=torch.float32).to(dtype)


def _measure(a, ref):
    a = a.double()
    ref = ref.double()
    return ((a - ref).abs().max() / ref.abs().max().clamp(min=1.0)).item()


class _env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("FENGSHEN_FUSED_NORM")
        os.environ["FENGSHEN_FUSED_NORM"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FENGSHEN_FUSED_NORM", None)
        else:
            os.environ["FENGSHEN_FUSED_NORM"] = self.old


def _run(fused, x, d, w, g_res, g_h):
    """-> (res, h, g, gw) through the autograd entry point."""
    from fengshen_amd.ops import functional as F
    with _env("1" if fused else "0"):
        xs = x.detach().clone().requires_grad_(True)
        ds = None if d is None else d.detach().clone().requires_grad_(True)
        ws = w.detach().clone().requires_grad_(True)
        res, h = F.residual_rms_norm(xs, ds, ws, EPS)
        outs, grads = [h], [g_h]
        if g_res is not None:
            outs.append(res)
            grads.append(g_res)
        torch.autograd.backward(outs, grads)
        if ds is not None:
            assert torch.equal(xs.grad, ds.grad)
        return res.detach(), h.detach(), xs.grad, ws.grad


def _oracle(res, w, g_res, g_h):
    """fp64 h, g, gw from the (already rounded) sum."""
    r = res.double()
    w64 = w.double()
    ir = torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + EPS)
    xhat = r * ir
    h = xhat * w64
    gyw = g_h.double() * w64
    inner = ir * (gyw - xhat * (gyw * xhat).mean(-1, keepdim=True))
    g = inner
    if g_res is not None:
        g = inner.to(res.dtype).double() + g_res.double()
    gw = (g_h.double() * xhat).sum(0)
    return h, g, gw


def _ordered_bits(t):
    """16-bit float bit patterns mapped so that adjacent values differ by 1."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _pair_figures(new, old, ref, dtype):
    fig = {"m_new": _measure(new, ref), "m_old": _measure(old, ref),
           "ndiff": (new != old).sum().item(), "numel": new.numel(),
           "max_step": 0}
    if dtype != torch.float32:
        fig["max_step"] = (_ordered_bits(new) - _ordered_bits(old)) \
            .abs().max().item()
    return fig


@functools.lru_cache(maxsize=None)
def _figures(rows, H, dtype):
    """Every figure the tests below assert on, computed once per shape and
    dtype and printed; keys are (with_residual, name)."""
    x = _rand(rows, H, dtype=dtype, seed=1)
    delta = _rand(rows, H, dtype=dtype, seed=2)
    w = (1.0 + 0.1 * _rand(H, dtype=torch.float32, seed=3)).to(dtype)
    g_res_t = _rand(rows, H, dtype=dtype, seed=4)
    g_h = _rand(rows, H, dtype=dtype, seed=5)
    figs = {}
    for with_res in (True, False):
        d = delta if with_res else None
        g_res = g_res_t if with_res else None
        res, h, g, gw = _run(True, x, d, w, g_res, g_h)
        res_o, h_o, g_o, _gw_o = _run(False, x, d, w, g_res, g_h)
        want_sum = x + delta if with_res else x
        figs[with_res, "sum_equal"] = (torch.equal(res, want_sum)
                                       and torch.equal(res, res_o))
        h_ref, g_ref, gw_ref = _oracle(res, w, g_res, g_h)
        figs[with_res, "h"] = _pair_figures(h, h_o, h_ref, dtype)
        figs[with_res, "g"] = _pair_figures(g, g_o, g_ref, dtype)
        figs[with_res, "gw_rel"] = ((gw.double() - gw_ref).abs().max()
                                    / gw_ref.abs().max()).item()
        print(f"[{rows}x{H} {dtype} residual={with_res}] "
              f"gw rel err {figs[with_res, 'gw_rel']:.4g}")
        for name in ("h", "g"):
            f = figs[with_res, name]
            print(f"  {name}: measure fused {f['m_new']:.4g} composed "
                  f"{f['m_old']:.4g} differing {f['ndiff']}/{f['numel']} "
                  f"max step {f['max_step']} ulp")
    return figs


def _pairs(figs):
    for with_res in (True, False):
        for name in ("h", "g"):
            yield f"{name} residual={with_res}", figs[with_res, name]


def test_every_branch_is_covered():
    assert {b for _r, _h, b in SHAPES} == ALL_BRANCHES


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,H,branch", SHAPES)
def test_against_oracle(rows, H, branch, dtype):
    """sum bit-equal to torch's add; h and g within the project's 2e-2 of the
    fp64 oracle (1e-5 for fp32); gw within 2e-2 relative."""
    from fengshen_amd.ops import get_ext
    assert get_ext().fused_norm_branch(H) == branch
    figs = _figures(rows, H, dtype)
    bound = 1e-5 if dtype == torch.float32 else 2e-2
    for with_res in (True, False):
        assert figs[with_res, "sum_equal"], "sum is not torch's x + delta"
        assert figs[with_res, "gw_rel"] < 2e-2
    for what, f in _pairs(figs):
        assert f["m_new"] < bound, what


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,H,branch", SHAPES)
def test_not_worse_than_composition(rows, H, branch, dtype):
    """The oracle measure of h and g is no larger than that of the LDS
    kernels + torch add on the same inputs (equal, since the outputs are
    bit-identical: test_bit_identical_to_composition)."""
    for what, f in _pairs(_figures(rows, H, dtype)):
        assert f["m_new"] <= f["m_old"], \
            f"{what}: {f['m_new']} > composed {f['m_old']}"


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=["bf16", "fp16"])
@pytest.mark.parametrize("rows,H,branch", SHAPES)
def test_rare_single_ulp_differences_from_composition(rows, H, branch, dtype):
    """Against the LDS kernels + torch add at most 1e-4 of the elements of h
    and g differ, each by one unit in the last place.  This is the bound a
    kernel with its own summation order would have to meet; the kernels as
    they stand meet the stricter test below."""
    for what, f in _pairs(_figures(rows, H, dtype)):
        assert f["ndiff"] <= 1e-4 * f["numel"], \
            f"{what}: {f['ndiff']} of {f['numel']} differ"
        assert f["max_step"] <= 1, f"{what}: differs by {f['max_step']} ulp"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,H,branch", SHAPES)
def test_bit_identical_to_composition(rows, H, branch, dtype):
    """h and g equal the LDS kernels + torch add bit for bit, so a model's
    outputs do not move when it switches kernels.  The register kernels take
    the row sums in the order the LDS kernels compile to (ROCm 7.2 hipcc,
    -O3 -ffast-math); if a compiler change reorders either side, this test
    is what reports it, and the two tests above say whether the results are
    still acceptable."""
    for what, f in _pairs(_figures(rows, H, dtype)):
        assert f["ndiff"] == 0, f"{what}: {f['ndiff']} of {f['numel']} differ"


def test_noncontiguous_grad():
    """g_h arriving as a strided view (a slice of a wider buffer): same bits
    as from a contiguous copy, and within bounds of the fp64 oracle."""
    rows, H = 33, 5120
    x = _rand(rows, H, seed=1)
    delta = _rand(rows, H, seed=2)
    w = (1.0 + 0.1 * _rand(H, dtype=torch.float32, seed=3)).bfloat16()
    g_res = _rand(rows, H, seed=4)
    wide = _rand(rows, H + 64, seed=5)
    g_h = wide[:, 8:8 + H]
    assert not g_h.is_contiguous()
    got = _run(True, x, delta, w, g_res, g_h)
    want = _run(True, x, delta, w, g_res, g_h.contiguous())
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    res, h, g, gw = got
    h_ref, g_ref, gw_ref = _oracle(res, w, g_res, g_h)
    assert _measure(h, h_ref) < 2e-2 and _measure(g, g_ref) < 2e-2
    assert ((gw.double() - gw_ref).abs().max() / gw_ref.abs().max()) < 2e-2


def test_weight_grad_is_reproducible():
    rows, H = 4099, 5120
    x = _rand(rows, H, seed=1)
    w = (1.0 + 0.1 * _rand(H, dtype=torch.float32, seed=3)).bfloat16()
    g_h = _rand(rows, H, seed=5)
    a = _run(True, x, None, w, None, g_h)
    b = _run(True, x, None, w, None, g_h)
    assert torch.equal(a[3], b[3]), "gw differs between two calls"
    assert torch.equal(a[2], b[2])


def test_rms_norm_uses_the_same_kernels():
    """F.rms_norm is the no-residual form of the fused op."""
    from fengshen_amd.ops import functional as F
    x = _rand(33, 5120, seed=1).requires_grad_(True)
    w = (1.0 + 0.1 * _rand(5120, dtype=torch.float32, seed=3)).bfloat16() \
        .requires_grad_(True)
    g_h = _rand(33, 5120, seed=5)
    F.rms_norm(x, w, EPS).backward(g_h)
    _res, h, g, gw = _run(True, x, None, w, None, g_h)
    assert torch.equal(x.grad, g) and torch.equal(w.grad, gw)
    assert torch.equal(F.rms_norm(x, w, EPS).detach(), h)


def _layer_run(fused, use_ckpt):
    from fengshen_amd.models.layers import ParallelTransformerLayer
    from fengshen_amd.parallel.random import checkpoint
    with _env("1" if fused else "0"):
        torch.manual_seed(11)
        layer = ParallelTransformerLayer(
            512, 4, causal=True, norm="rmsnorm", norm_eps=EPS,
            mlp_type="swiglu", ffn_hidden_size=1408, rotary=True,
            max_positions=512, bias=False, dtype=torch.bfloat16).cuda()
        with torch.no_grad():  # weights away from 1 so gw paths matter
            layer.input_norm.weight.add_(0.1 * _rand(512, seed=8))
            layer.post_attention_norm.weight.add_(0.1 * _rand(512, seed=9))
        x = _rand(2, 64, 512, seed=5).requires_grad_(True)
        gy = _rand(2, 64, 512, seed=6)
        out = checkpoint(layer, x) if use_ckpt else layer(x)
        out.backward(gy)
        torch.cuda.synchronize()
        grads = {n: p.grad for n, p in layer.named_parameters()}
        return out.detach(), x.grad, grads


@pytest.mark.parametrize("use_ckpt", [False, True], ids=["plain", "ckpt"])
def test_layer_matches_unfused(use_ckpt):
    out, dx, grads = _layer_run(True, use_ckpt)
    out_r, dx_r, grads_r = _layer_run(False, use_ckpt)

    def close(name, a, r):
        assert a is not None and r is not None, name
        m = _measure(a, r)
        print(f"  {name}: {m:.4g}")
        assert m < 2e-2, name

    close("out", out, out_r)
    close("dx", dx, dx_r)
    assert grads.keys() == grads_r.keys() and grads
    for n in grads:
        close(n, grads[n], grads_r[n])
