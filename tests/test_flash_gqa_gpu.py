"""Grouped-query attention on the causal v3 flash kernels: k/v carry h_kv
heads, query head j uses KV head j // (h / h_kv).

Oracle: fp32 eager attention on K/V expanded in that order, autograd giving
dK/dV per KV head; measure: the relative-to-range error of
test_flash_varlen_gpu.py at its 2e-2.  What must not change a bit is compared
with torch.equal: O, LSE and dQ against the plain kernels on expanded K/V
(per query head the arithmetic is the same), dK/dV of one group member
against the plain kernels on that head (the other members add exact zeros),
and a second run.  All tests require an MI355X."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-2
HEADS = [(4, 2), (4, 1), (6, 2)]


@pytest.fixture(autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"


def _close(a, b, tol=TOL):
    """relative-to-range closeness (bf16 outputs vs fp32 oracle)."""
    a = a.float()
    b = b.float()
    scale = b.abs().max().clamp(min=1.0)
    err = (a - b).abs().max() / scale
    assert err.item() < tol, f"rel err {err.item():.4g} (scale {scale.item():.3g})"


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda",
                       dtype=torch.float32).to(torch.bfloat16)


def _views(buf, h, h_kv):
    """[b, s, (h + 2*h_kv)*d] packed buffer -> q [b, h, s, d] and k, v
    [b, h_kv, s, d] views."""
    d = buf.shape[-1] // (h + 2 * h_kv)
    q = buf.narrow(2, 0, h * d).unflatten(2, (h, d)).transpose(1, 2)
    k, v = [buf.narrow(2, (h + i * h_kv) * d, h_kv * d)
            .unflatten(2, (h_kv, d)).transpose(1, 2) for i in range(2)]
    return q, k, v


def _bhsd(x, np_):
    return x.unflatten(2, (np_, -1)).transpose(1, 2)


def _expand(x, h):
    b, h_kv, s, d = x.shape
    return x[:, :, None].expand(b, h_kv, h // h_kv, s, d).reshape(b, h, s, d)


def _from_starts(s, rows):
    """int32 [b, s] from per-batch-row lists of document starts."""
    ks = torch.zeros(len(rows), s, dtype=torch.int32)
    for bi, starts in enumerate(rows):
        for st in sorted(x for x in starts if x < s):
            ks[bi, st:] = st
    return ks.cuda()


def _kstart(pattern, s):
    if pattern == "none":
        return None
    if pattern == "docs":
        # starts inside a 32-row sub-tile, at a tile edge, a one-token
        # document, a start at the second 256-row block, starts off every edge
        return _from_starts(s, [[0, 37, 64, 65, 256], [0, 1, 100, 191, 290]])
    assert pattern == "pad"
    from fengshen_amd.ops.flash import mask_to_kstart
    m = torch.zeros(2, s, dtype=torch.bool, device="cuda")
    m[0, s - 27:] = True       # right padding
    m[1, :37] = True           # left padding
    return mask_to_kstart(m, s)


def _oracle(q, k, v, do, ks, h):
    """fp32 attention on expanded K/V; grads per KV head by autograd."""
    from fengshen_amd.ops.flash import kstart_to_mask
    s, d = q.shape[-2], q.shape[-1]
    q, k, v = [t.float().detach().requires_grad_(True) for t in (q, k, v)]
    sc = torch.matmul(q, _expand(k, h).transpose(-1, -2)) / math.sqrt(d)
    if ks is not None:
        mask = kstart_to_mask(ks)
    else:
        mask = torch.ones(s, s, dtype=torch.bool, device="cuda").triu(1)
    sc = sc.masked_fill(mask, float("-inf"))
    o = torch.matmul(torch.softmax(sc, dim=-1), _expand(v, h))
    o.backward(do.float())
    return o.detach(), q.grad, k.grad, v.grad


@functools.lru_cache(maxsize=None)
def _case(h, h_kv, d, s, pattern):
    """Inputs and the fp32 oracle of one case, computed once and shared by
    the tests that need it (never written to)."""
    b = 2
    qkv = _rand(b, s, (h + 2 * h_kv) * d, seed=h * 7 + h_kv + d + s)
    do = _rand(b, s, h * d, seed=h * 7 + h_kv + d + s + 1)
    ks = _kstart(pattern, s)
    q, k, v = _views(qkv, h, h_kv)
    return qkv, do, ks, _oracle(q, k, v, _bhsd(do, h), ks, h)


GRID = [pytest.param(h, h_kv, d, s, p, id=f"h{h}kv{h_kv}-d{d}-s{s}-{p}")
        for (h, h_kv) in HEADS for d in (64, 96, 128) for s in (64, 128, 320)
        for p in ("none", "docs", "pad")]


@pytest.mark.parametrize("h,h_kv,d,s,pattern", GRID)
def test_contiguous_matches_fp32_oracle(h, h_kv, d, s, pattern):
    from fengshen_amd.ops.flash import flash_attention
    qkv, do, ks, ref = _case(h, h_kv, d, s, pattern)
    q, k, v = [t.contiguous().requires_grad_(True)
               for t in _views(qkv, h, h_kv)]
    o = flash_attention(q, k, v, 1.0 / math.sqrt(d), causal=True, kstart=ks)
    o.backward(_bhsd(do, h))
    torch.cuda.synchronize()
    assert k.grad.shape == k.shape and v.grad.shape == v.shape
    for name, a, r in zip(("O", "dQ", "dK", "dV"),
                          (o, q.grad, k.grad, v.grad), ref):
        assert a.isfinite().all(), name
        _close(a, r)


@pytest.mark.parametrize("h,h_kv,d,s,pattern", GRID)
def test_packed_matches_fp32_oracle(h, h_kv, d, s, pattern):
    from fengshen_amd.ops.flash import packed_self_attention
    qkv, do, ks, ref = _case(h, h_kv, d, s, pattern)
    x = qkv.clone().requires_grad_(True)
    o = packed_self_attention(x, h, None, None, 0, 1.0 / math.sqrt(d),
                              causal=True, kstart=ks, num_kv_heads=h_kv)
    assert o.shape == (2, s, h * d)
    o.backward(do)
    torch.cuda.synchronize()
    assert x.grad.shape == x.shape
    got = (_bhsd(o, h),) + tuple(_views(x.grad, h, h_kv))
    for name, a, r in zip(("O", "dQ", "dK", "dV"), got, ref):
        assert a.isfinite().all(), name
        _close(a, r)


def _ext_run(q, k, v, do, ks, d, o_lse=None):
    """Contiguous extension entries -> (o, lse, dq, dk, dv); with o_lse the
    backward runs on that saved (o, lse) instead of a forward of its own."""
    from fengshen_amd.ops import get_ext
    from fengshen_amd.ops.flash import kstart_qend
    ext = get_ext()
    scale = 1.0 / math.sqrt(d)
    kw_f, kw_b = {}, {}
    if ks is not None:
        kw_f = {"kstart": ks}
        kw_b = {"kstart": ks, "qend": kstart_qend(ks)}
    if o_lse is None:
        o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, True, None, 0.0, 0,
                                       **kw_f)
    else:
        o, lse = o_lse
    dq, dk, dv = ext.flash_attn_bwd_v3(q, k, v, o, do, lse, scale, True, None,
                                       0.0, 0, **kw_b)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def _contig(h, h_kv, d, s, pattern):
    qkv, do, ks, _ = _case(h, h_kv, d, s, pattern)
    q, k, v = [t.contiguous() for t in _views(qkv, h, h_kv)]
    return q, k, v, _bhsd(do, h).contiguous(), ks


@pytest.mark.parametrize("pattern", ["none", "docs"])
@pytest.mark.parametrize("d", [64, 96, 128])
@pytest.mark.parametrize("h,h_kv", HEADS)
def test_bitexact_against_plain_kernels_on_expanded_kv(h, h_kv, d, pattern):
    """Per query head the grouped kernels do the arithmetic of the plain
    ones: O, LSE and dQ are the same bits."""
    s = 320
    q, k, v, do, ks = _contig(h, h_kv, d, s, pattern)
    o, lse, dq, _, _ = _ext_run(q, k, v, do, ks, d)
    ke, ve = _expand(k, h).contiguous(), _expand(v, h).contiguous()
    o2, lse2, dq2, _, _ = _ext_run(q, ke, ve, do, ks, d)
    assert lse.shape == (2, h, s)
    assert torch.equal(o, o2)
    assert torch.equal(lse, lse2)
    assert torch.equal(dq, dq2)


@pytest.mark.parametrize("pattern", ["none", "docs"])
@pytest.mark.parametrize("d", [64, 96, 128])
@pytest.mark.parametrize("h,h_kv", HEADS)
def test_dkv_group_loop_one_member_at_a_time(h, h_kv, d, pattern):
    """With dO zeroed for every member of the group but m, the others add
    exact zeros (dP = 0 and delta = 0 give dS = 0), so dK/dV are the bits
    the plain kernel gives for member m's head alone — on the O and LSE the
    grouped forward saved.  Catches a wrong LSE, delta or dO offset in the
    group loop."""
    s = 320
    g = h // h_kv
    q, k, v, do, ks = _contig(h, h_kv, d, s, pattern)
    o, lse, _, _, _ = _ext_run(q, k, v, do, ks, d)
    for m in range(g):
        heads = [kv * g + m for kv in range(h_kv)]
        do_m = torch.zeros_like(do)
        do_m[:, heads] = do[:, heads]
        _, _, _, dk, dv = _ext_run(q, k, v, do_m, ks, d, o_lse=(o, lse))
        _, _, _, dk1, dv1 = _ext_run(
            q[:, heads].contiguous(), k, v, do[:, heads].contiguous(), ks, d,
            o_lse=(o[:, heads].contiguous(), lse[:, heads].contiguous()))
        assert dk.isfinite().all() and dv.isfinite().all()
        assert torch.equal(dk, dk1), f"dK, member {m}"
        assert torch.equal(dv, dv1), f"dV, member {m}"


@pytest.mark.parametrize("h,h_kv", HEADS)
def test_two_runs_same_bits(h, h_kv):
    q, k, v, do, ks = _contig(h, h_kv, 128, 320, "docs")
    a = _ext_run(q, k, v, do, ks, 128)
    b = _ext_run(q, k, v, do, ks, 128)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


@pytest.mark.parametrize("h,h_kv", HEADS)
def test_packed_rotary_equals_out_of_place(h, h_kv):
    from fengshen_amd.ops import functional as F_ops
    from fengshen_amd.ops.flash import flash_attention, packed_self_attention
    d, s = 64, 128
    qkv, do, _, _ = _case(h, h_kv, d, s, "none")
    cos, sin = F_ops.build_rope_cache(s + 8, d)
    cos, sin = cos.cuda(), sin.cuda()
    scale = 1.0 / math.sqrt(d)

    x = qkv.clone().requires_grad_(True)
    o = packed_self_attention(x * 1, h, cos, sin, 3, scale, causal=True,
                              num_kv_heads=h_kv)
    o.backward(do)

    q, k, v = [t.contiguous() for t in _views(qkv, h, h_kv)]
    qr, kr = F_ops.apply_rotary(q, k, cos, sin, offset=3)
    o2 = flash_attention(qr, kr, v, scale, causal=True)
    torch.cuda.synchronize()
    assert torch.equal(_bhsd(o, h), o2)

    # fp32 oracle of the input gradient: eager rotary + eager attention
    x32 = qkv.float().detach().requires_grad_(True)
    q32, k32, v32 = _views(x32, h, h_kv)
    q32, k32 = F_ops.eager_apply_rotary(q32, k32, cos, sin, offset=3)
    sc = torch.matmul(q32, _expand(k32, h).transpose(-1, -2)) * scale
    sc = sc.masked_fill(
        torch.ones(s, s, dtype=torch.bool, device="cuda").triu(1),
        float("-inf"))
    o32 = torch.matmul(torch.softmax(sc, dim=-1), _expand(v32, h))
    o32.backward(_bhsd(do, h).float())
    assert x.grad.isfinite().all()
    _close(x.grad, x32.grad)


def _count_calls(monkeypatch, name):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    real = getattr(ext, name)
    calls = []

    def wrapper(*a, **kw):
        calls.append((tuple(a[0].shape), tuple(a[1].shape)))
        return real(*a, **kw)
    monkeypatch.setattr(ext, name, wrapper)
    return calls


def _layer_run(layer, x):
    layer.zero_grad(set_to_none=True)
    xi = x.clone().requires_grad_(True)
    out = layer(xi)
    out.float().square().mean().backward()
    torch.cuda.synchronize()
    return [out.detach(), xi.grad] + [p.grad.clone()
                                      for p in layer.parameters()]


def test_layer_takes_packed_gqa_path(monkeypatch):
    from fengshen_amd.models.layers import ParallelAttention
    torch.manual_seed(0)
    layer = ParallelAttention(256, 4, causal=True, rotary=True,
                              num_kv_heads=2, bias=False,
                              max_positions=128).cuda().to(torch.bfloat16)
    x = _rand(2, 128, 256, seed=5)
    fwd = _count_calls(monkeypatch, "flash_attn_fwd_v3_strided")
    bwd = _count_calls(monkeypatch, "flash_attn_bwd_v3_strided")
    native = _layer_run(layer, x)
    # q with 4 heads and k with 2, both views of the packed projection
    assert fwd == [((2, 4, 128, 64), (2, 2, 128, 64))]
    assert bwd == [((2, 4, 128, 64), (2, 2, 128, 64))]

    for var in ("FENGSHEN_GQA_FLASH", "FENGSHEN_PACKED_ATTN"):
        del fwd[:]
        with monkeypatch.context() as mp:
            mp.setenv(var, "0")
            other = _layer_run(layer, x)
        assert fwd == []     # neither takes the packed entry
        for a, r in zip(other, native):
            assert a.isfinite().all()
            _close(a, r)


def test_tiny_llama_right_padded_native_vs_expansion(monkeypatch):
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=64)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda()
    assert model.model.layers[0].attention.num_kv_heads == 2
    ids = torch.randint(3, 512, (2, 64), device="cuda")
    am = torch.ones(2, 64, dtype=torch.long, device="cuda")
    am[1, 40:] = 0
    labels = ids.masked_fill(am == 0, -100)
    fwd = _count_calls(monkeypatch, "flash_attn_fwd_v3_strided")
    native = model(ids, attention_mask=am, labels=labels).loss.item()
    assert len(fwd) == 2 and fwd[0][1][1] == 2
    monkeypatch.setenv("FENGSHEN_GQA_FLASH", "0")
    expanded = model(ids, attention_mask=am, labels=labels).loss.item()
    assert math.isfinite(native) and math.isfinite(expanded)
    assert abs(native - expanded) / abs(expanded) < TOL


def _peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def test_native_allocates_less_than_expansion():
    from fengshen_amd.ops.flash import expand_kv, flash_attention
    b, h, h_kv, s, d = 1, 16, 2, 4096, 128
    q = _rand(b, h, s, d, seed=1).requires_grad_(True)
    k = _rand(b, h_kv, s, d, seed=2).requires_grad_(True)
    v = _rand(b, h_kv, s, d, seed=3).requires_grad_(True)
    do = _rand(b, h, s, d, seed=4)
    scale = 1.0 / math.sqrt(d)

    def native():
        flash_attention(q, k, v, scale, causal=True).backward(do)

    def expanded():
        flash_attention(q, expand_kv(k, h), expand_kv(v, h), scale,
                        causal=True).backward(do)

    peaks = {}
    for name, fn in (("native", native), ("expanded", expanded)):
        fn()                       # warm-up: leaves .grad allocated
        peaks[name] = _peak_of(fn)
    print(f"peak bytes: native {peaks['native']}, "
          f"expanded {peaks['expanded']}")
    assert peaks["native"] < peaks["expanded"]


def test_binding_refusals():
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    b, h, s, d = 2, 4, 64, 64
    q = _rand(b, h, s, d)
    k2, v2 = _rand(b, 2, s, d, seed=1), _rand(b, 2, s, d, seed=2)
    o = torch.empty_like(q)
    with pytest.raises(RuntimeError, match="GQA.*multiple"):
        ext.flash_attn_fwd_v3(q, _rand(b, 3, s, d), _rand(b, 3, s, d), 0.125,
                              True, None, 0.0, 0)
    with pytest.raises(RuntimeError, match="GQA.*causal"):
        ext.flash_attn_fwd_v3(q, k2, v2, 0.125, False, None, 0.0, 0)
    with pytest.raises(RuntimeError, match="GQA.*dropout"):
        ext.flash_attn_fwd_v3(q, k2, v2, 0.125, True, None, 0.1, 7)
    klens = torch.full((b,), s, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="GQA.*klens"):
        ext.flash_attn_fwd_v3_strided(q, k2, v2, o, 0.125, True, klens)
    with pytest.raises(RuntimeError, match="GQA"):
        ext.flash_attn_fwd_v3_strided(q, k2, v2, o, 0.125, False, klens)
    # k and v with different strides
    wide = _rand(b, 2, s, 2 * d, seed=3)
    with pytest.raises(RuntimeError, match="share strides"):
        ext.flash_attn_fwd_v3_strided(q, k2, wide.narrow(3, 0, d), o, 0.125,
                                      True, None)
    # a k/v row stride that is no multiple of 8 elements
    odd_k = _rand(b, 2, s, d + 4, seed=4).narrow(3, 0, d)
    odd_v = _rand(b, 2, s, d + 4, seed=5).narrow(3, 0, d)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.flash_attn_fwd_v3_strided(q, odd_k, odd_v, o, 0.125, True, None)
    # the backward entry refuses the same way
    lse = torch.zeros(b, h, s, device="cuda")
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k2), \
        torch.empty_like(v2)
    with pytest.raises(RuntimeError, match="GQA.*causal"):
        ext.flash_attn_bwd_v3_strided(q, k2, v2, o, q, lse, dq, dk, dv, 0.125,
                                      False, None)
    with pytest.raises(RuntimeError, match="share strides"):
        ext.flash_attn_bwd_v3_strided(q, k2, v2, o, q, lse, dq, dk,
                                      wide.narrow(3, 0, d), 0.125, True, None)
