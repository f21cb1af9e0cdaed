"""Causal flash attention with a per-row key start (kstart): row i sees keys
kstart[i] <= j <= i — padded and packed batches on the v3 kernels.

Oracle: fp32 eager attention under the dense mask expanded from kstart;
measure: the relative-to-range error of test_ops_gpu.py at its 2e-2, on O,
dQ, dK and dV.  What must not change a bit (kstart = 0 against the plain
causal call, a neighbour document's tokens, a second run) is compared with
torch.equal.  All tests require an MI355X."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

TOL = 2e-2


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


def _views(buf, np_):
    """[b, s, 3*np*d] packed buffer -> q, k, v as [b, np, s, d] views."""
    h = buf.shape[-1] // 3
    return [buf.narrow(2, i * h, h).unflatten(2, (np_, -1)).transpose(1, 2)
            for i in range(3)]


def _bhsd(x, np_):
    return x.unflatten(2, (np_, -1)).transpose(1, 2)


def _from_starts(s, rows):
    """int32 [b, s] from per-batch-row lists of document starts."""
    ks = torch.zeros(len(rows), s, dtype=torch.int32)
    for bi, starts in enumerate(rows):
        for st in sorted(x for x in starts if x < s):
            ks[bi, st:] = st
    return ks.cuda()


def _kstart(pattern, s):
    if pattern == "docs":
        # row 0: a start inside a 32-row MFMA sub-tile (37), at a tile edge
        # (64), a one-token document (64..64) and a start at 256 (block 1
        # skips four tiles, its later waves all but one);
        # row 1: a one-token first document and starts off every edge (100:
        # rows 100.. meet tile 0 fully masked, because rows 96..99 of their
        # wave still see it)
        return _from_starts(s, [[0, 37, 64, 65, 256], [0, 1, 100, 191, 290]])
    assert pattern == "pad"
    from fengshen_amd.ops.flash import mask_to_kstart
    m = torch.zeros(2, s, dtype=torch.bool, device="cuda")
    m[0, s - 27:] = True       # right padding
    m[1, :37] = True           # left padding
    return mask_to_kstart(m, s)


@functools.lru_cache(maxsize=None)
def _case(d, s, pattern):
    """Inputs and the fp32 oracle of one case, computed once and shared by
    the contiguous and the strided test (never written to)."""
    from fengshen_amd.ops.flash import kstart_to_mask
    b, h = 2, 2
    qkv = _rand(b, s, 3 * h * d, seed=d + s)
    do = _rand(b, s, h * d, seed=d + s + 1)
    ks = _kstart(pattern, s)
    q, k, v = [t.float().detach().requires_grad_(True)
               for t in _views(qkv, h)]
    sc = torch.matmul(q, k.transpose(-1, -2)) / math.sqrt(d)
    sc = sc.masked_fill(kstart_to_mask(ks), float("-inf"))
    o = torch.matmul(torch.softmax(sc, dim=-1), v)
    o.backward(_bhsd(do, h).float())
    return qkv, do, ks, (o.detach(), q.grad, k.grad, v.grad)


@pytest.mark.parametrize("pattern", ["docs", "pad"])
@pytest.mark.parametrize("s", [64, 128, 320])
@pytest.mark.parametrize("d", [64, 96, 128])
def test_contiguous_matches_fp32_oracle(d, s, pattern):
    from fengshen_amd.ops.flash import flash_attention
    qkv, do, ks, ref = _case(d, s, pattern)
    q, k, v = [t.contiguous().requires_grad_(True) for t in _views(qkv, 2)]
    o = flash_attention(q, k, v, 1.0 / math.sqrt(d), causal=True, kstart=ks)
    o.backward(_bhsd(do, 2))
    torch.cuda.synchronize()
    for name, a, r in zip(("O", "dQ", "dK", "dV"),
                          (o, q.grad, k.grad, v.grad), ref):
        assert a.isfinite().all(), name
        _close(a, r)


@pytest.mark.parametrize("pattern", ["docs", "pad"])
@pytest.mark.parametrize("s", [64, 128, 320])
@pytest.mark.parametrize("d", [64, 96, 128])
def test_strided_matches_fp32_oracle(d, s, pattern):
    from fengshen_amd.ops.flash import packed_self_attention
    qkv, do, ks, ref = _case(d, s, pattern)
    x = qkv.clone().requires_grad_(True)
    o = packed_self_attention(x, 2, None, None, 0, 1.0 / math.sqrt(d),
                              causal=True, kstart=ks)
    o.backward(do)
    torch.cuda.synchronize()
    got = (_bhsd(o, 2),) + tuple(_views(x.grad, 2))
    for name, a, r in zip(("O", "dQ", "dK", "dV"), got, ref):
        assert a.isfinite().all(), name
        _close(a, r)


def _ext_run(q, k, v, do, ks, d, qend=None, check_values=False):
    """Contiguous extension entries -> (o, lse, dq, dk, dv)."""
    from fengshen_amd.ops import get_ext
    from fengshen_amd.ops.flash import kstart_qend
    ext = get_ext()
    scale = 1.0 / math.sqrt(d)
    if ks is None:
        o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, True, None, 0.0, 0)
        grads = ext.flash_attn_bwd_v3(q, k, v, o, do, lse, scale, True, None,
                                      0.0, 0)
    else:
        if qend is None:
            qend = kstart_qend(ks)
        o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, True, None, 0.0, 0,
                                       kstart=ks, check_values=check_values)
        grads = ext.flash_attn_bwd_v3(q, k, v, o, do, lse, scale, True, None,
                                      0.0, 0, kstart=ks, qend=qend,
                                      check_values=check_values)
    torch.cuda.synchronize()
    return (o, lse) + tuple(grads)


def _qkvdo(d, s, seed=0, b=2, h=2):
    return [_rand(b, h, s, d, seed=seed + i) for i in range(4)]


NAMES = ("O", "LSE", "dQ", "dK", "dV")


@pytest.mark.parametrize("d", [64, 96, 128])
def test_kstart_zeros_is_bit_identical_to_plain_causal(d):
    s = 320
    q, k, v, do = _qkvdo(d, s)
    zeros = torch.zeros(2, s, dtype=torch.int32, device="cuda")
    plain = _ext_run(q, k, v, do, None, d)
    got = _ext_run(q, k, v, do, zeros, d, check_values=True)
    for name, a, r in zip(NAMES, got, plain):
        assert torch.equal(a, r), f"{name} differs"


def test_kstart_zeros_is_bit_identical_strided():
    from fengshen_amd.ops import get_ext
    from fengshen_amd.ops.flash import kstart_qend
    ext = get_ext()
    b, s, h, d = 2, 320, 3, 128
    scale = 1.0 / math.sqrt(d)
    qkv = _rand(b, s, 3 * h * d)
    do = _bhsd(_rand(b, s, h * d, seed=1), h)
    q, k, v = _views(qkv, h)
    zeros = torch.zeros(b, s, dtype=torch.int32, device="cuda")
    res = []
    for kw_f, kw_b in (({}, {}), ({"kstart": zeros},
                                  {"kstart": zeros,
                                   "qend": kstart_qend(zeros)})):
        o = torch.full((b, s, h * d), float("nan"), device="cuda",
                       dtype=torch.bfloat16)
        g = torch.full((b, s, 3 * h * d), float("nan"), device="cuda",
                       dtype=torch.bfloat16)
        lse = ext.flash_attn_fwd_v3_strided(q, k, v, _bhsd(o, h), scale, True,
                                            None, **kw_f)
        ext.flash_attn_bwd_v3_strided(q, k, v, _bhsd(o, h), do, lse,
                                      *_views(g, h), scale, True, None,
                                      **kw_b)
        torch.cuda.synchronize()
        res.append((o, lse, g))
    for name, a, r in zip(("O", "LSE", "dQKV"), res[1], res[0]):
        assert torch.equal(a, r), f"{name} differs"


@pytest.mark.parametrize("d", [64, 128])
def test_documents_are_isolated_bitwise(d):
    """Other tokens in document 1 leave document 2's O, dQ, dK, dV as they
    are, bit for bit (start 100: inside a tile and a sub-tile)."""
    s, st = 320, 100
    ks = _from_starts(s, [[0, st], [0, st]])
    q, k, v, do = _qkvdo(d, s)
    a = _ext_run(q, k, v, do, ks, d)
    q2, k2, v2 = [t.clone() for t in (q, k, v)]
    for t, seed in ((q2, 11), (k2, 12), (v2, 13)):
        t[:, :, :st] = _rand(2, 2, st, d, seed=seed)
    b_ = _ext_run(q2, k2, v2, do, ks, d)
    for name, x, y in zip(NAMES, a, b_):
        assert torch.equal(x[:, :, st:], y[:, :, st:]), f"{name} of doc 2"
        assert not torch.equal(x[:, :, :st], y[:, :, :st]), name


@pytest.mark.parametrize("d", [64, 96, 128])
def test_document_in_pack_agrees_with_document_alone(d):
    s, st = 320, 128
    ks = _from_starts(s, [[0, st], [0, 37, st]])
    q, k, v, do = _qkvdo(d, s)
    packed = _ext_run(q, k, v, do, ks, d)
    alone = _ext_run(*[t[:, :, st:].contiguous() for t in (q, k, v, do)],
                     None, d)
    for name, x, y in zip(NAMES, packed, alone):
        if name != "LSE":
            _close(x[:, :, st:], y)


def test_two_runs_are_bit_identical():
    d, s = 128, 320
    ks = _kstart("docs", s)
    q, k, v, do = _qkvdo(d, s)
    a = _ext_run(q, k, v, do, ks, d)
    b_ = _ext_run(q, k, v, do, ks, d)
    for name, x, y in zip(NAMES, a, b_):
        assert torch.equal(x, y), f"{name} differs between runs"


def test_out_of_range_values_only_change_visibility():
    """kstart past its row acts as kstart = row, a negative one as 0, and a
    qend past the end as the end: values are clamped where they are read."""
    d, s = 64, 128
    q, k, v, do = _qkvdo(d, s)
    ar = torch.arange(s, dtype=torch.int32, device="cuda")
    good = torch.stack([ar, torch.zeros_like(ar)])
    bad = torch.stack([ar + (1 << 30), torch.zeros_like(ar) - 7])
    from fengshen_amd.ops.flash import kstart_qend
    a = _ext_run(q, k, v, do, good, d)
    b_ = _ext_run(q, k, v, do, bad, d,
                  qend=kstart_qend(good) + (1 << 30))
    for name, x, y in zip(NAMES, a, b_):
        assert torch.equal(x, y), name
    # a row that sees only itself returns its own v
    assert torch.equal(a[0][0], v[0])
    from fengshen_amd.ops import get_ext
    with pytest.raises(RuntimeError, match="outside"):
        get_ext().flash_attn_fwd_v3(q, k, v, 0.125, True, None, 0.0, 0,
                                    kstart=bad, check_values=True)


def test_bindings_raise_before_launch():
    from fengshen_amd.ops import get_ext
    from fengshen_amd.ops.flash import kstart_qend
    ext = get_ext()
    b, s, h, d = 2, 128, 2, 64
    q, k, v, do = _qkvdo(d, s)
    ks = torch.zeros(b, s, dtype=torch.int32, device="cuda")
    qe = kstart_qend(ks)
    klens = torch.full((b,), s, dtype=torch.int32, device="cuda")
    o = torch.full((b, h, s, d), float("nan"), device="cuda",
                   dtype=torch.bfloat16)
    lse = torch.zeros(b, h, s, device="cuda")
    g = [torch.full_like(o, float("nan")) for _ in range(3)]

    def fwd_c(kstart=ks, causal=True, klens=None, drop=0.0):
        ext.flash_attn_fwd_v3(q, k, v, 0.125, causal, klens, drop, 0,
                              kstart=kstart)

    def fwd_s(kstart=ks, causal=True, klens=None):
        ext.flash_attn_fwd_v3_strided(q, k, v, o, 0.125, causal, klens,
                                      kstart=kstart)

    def bwd_c(kstart=ks, causal=True, klens=None, drop=0.0, qend=qe):
        ext.flash_attn_bwd_v3(q, k, v, q, do, lse, 0.125, causal, klens,
                              drop, 0, kstart=kstart, qend=qend)

    def bwd_s(kstart=ks, causal=True, klens=None, qend=qe):
        ext.flash_attn_bwd_v3_strided(q, k, v, q, do, lse, *g, 0.125, causal,
                                      klens, kstart=kstart, qend=qend)

    bad = [
        ("int32", dict(kstart=ks.long())),
        (r"must be \[2, 128\]", dict(kstart=ks[:, :64].contiguous())),
        (r"must be \[2, 128\]", dict(kstart=ks[0])),
        ("contiguous", dict(kstart=torch.zeros(
            b, 2 * s, dtype=torch.int32, device="cuda")[:, ::2])),
        ("device", dict(kstart=ks.cpu())),
        ("causal", dict(causal=False)),
        ("klens", dict(klens=klens)),
    ]
    for fn in (fwd_c, fwd_s, bwd_c, bwd_s):
        for match, kw in bad:
            with pytest.raises(RuntimeError, match=match):
                fn(**kw)
    for fn in (fwd_c, bwd_c):
        with pytest.raises(RuntimeError, match="dropout"):
            fn(drop=0.1)
    for fn in (bwd_c, bwd_s):
        with pytest.raises(RuntimeError, match="needs qend"):
            fn(qend=None)
        with pytest.raises(RuntimeError, match="qend must be int32"):
            fn(qend=qe.long())
        with pytest.raises(RuntimeError, match=r"qend must be \[2, 2\]"):
            fn(qend=qe[:, :1].contiguous())
        with pytest.raises(RuntimeError, match="device"):
            fn(qend=qe.cpu())
    with pytest.raises(RuntimeError, match="expected"):
        ext.flash_attn_bwd_v3(q, k, v, q, do, lse, 0.125, True, None, 0.0, 0,
                              kstart=ks, qend=qe - 1, check_values=True)
    torch.cuda.synchronize()
    # nothing ran: the outputs of the strided entries are still untouched
    assert o.isnan().all() and all(t.isnan().all() for t in g)


# ---- routing -------------------------------------------------------------
def _tiny_llama():
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=256, hidden_size=128, num_hidden_layers=2,
                      num_attention_heads=2, intermediate_size=256,
                      max_position_embeddings=256)
    torch.manual_seed(0)
    return LlamaForCausalLM(cfg).to(torch.bfloat16).cuda()


def _spy(monkeypatch, name):
    """Count calls of an extension entry that carry a kstart."""
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    orig = getattr(ext, name)
    calls = []

    def spy(*a, **kw):
        if kw.get("kstart") is not None:
            calls.append(kw["kstart"])
        return orig(*a, **kw)

    monkeypatch.setattr(ext, name, spy)
    return calls


def _train_step(model, ids, am, monkeypatch, varlen):
    monkeypatch.setenv("FENGSHEN_VARLEN_FLASH", "1" if varlen else "0")
    model.zero_grad()
    out = model(ids, attention_mask=am,
                labels=ids.masked_fill(am == 0, -100))
    out.loss.backward()
    torch.cuda.synchronize()
    return (out.logits.detach(), out.loss.detach(),
            [p.grad.clone() for p in model.parameters()])


@pytest.mark.parametrize("ckpt", [False, True])
def test_llama_padded_batch_runs_the_kernels(ckpt, monkeypatch):
    model = _tiny_llama()
    if ckpt:
        model.gradient_checkpointing_enable()
    model.train()
    s = 128
    ids = torch.randint(3, 256, (2, s), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(1))
    am = torch.ones(2, s, dtype=torch.long, device="cuda")
    am[0, 90:] = 0
    am[1, 37:] = 0
    fwd = _spy(monkeypatch, "flash_attn_fwd_v3_strided")
    bwd = _spy(monkeypatch, "flash_attn_bwd_v3_strided")
    new = _train_step(model, ids, am, monkeypatch, True)
    n_layers = 2
    assert len(fwd) == n_layers * (2 if ckpt else 1)
    assert len(bwd) == n_layers
    want = torch.where(am.bool(), 0, torch.arange(s, device="cuda")).int()
    assert all(torch.equal(ks, want) for ks in fwd)
    n_f, n_b = len(fwd), len(bwd)
    old = _train_step(model, ids, am, monkeypatch, False)
    assert (len(fwd), len(bwd)) == (n_f, n_b), \
        "FENGSHEN_VARLEN_FLASH=0 still ran the kstart kernels"
    real = am.bool()
    _close(new[0][real], old[0][real])
    _close(new[1], old[1])
    for g_new, g_old in zip(new[2], old[2]):
        assert g_new.isfinite().all()
        _close(g_new, g_old)


def test_llama_left_padded_prefill_with_cache_runs_the_kernels(monkeypatch):
    from transformers.cache_utils import DynamicCache
    model = _tiny_llama().eval()
    s = 128
    ids = torch.randint(3, 256, (2, s), device="cuda",
                        generator=torch.Generator("cuda").manual_seed(2))
    am = torch.ones(2, s, dtype=torch.long, device="cuda")
    am[0, :37] = 0
    am[1, :100] = 0
    fwd = _spy(monkeypatch, "flash_attn_fwd_v3")
    res = []
    for varlen in (True, False):
        monkeypatch.setenv("FENGSHEN_VARLEN_FLASH", "1" if varlen else "0")
        cache = DynamicCache()
        with torch.no_grad():
            out = model(ids, attention_mask=am, past_key_values=cache,
                        use_cache=True)
        torch.cuda.synchronize()
        assert cache.get_seq_length() == s
        res.append(out.logits)
        assert len(fwd) == 2, "one kstart call per layer, none with =0"
    real = am.bool()
    _close(res[0][real], res[1][real])


def test_padded_attention_needs_no_score_tensor():
    """b1 h8 s4096 d128 under a padded mask: forward + backward allocate
    less than one [h, s, s] bf16 score tensor (the bmm path holds several)."""
    from fengshen_amd.ops import functional as F
    h, s, d = 8, 4096, 128
    q, k, v, do = [t.requires_grad_(True)
                   for t in _qkvdo(d, s, b=1, h=h)]
    mask = torch.zeros(1, 1, 1, s, dtype=torch.bool, device="cuda")
    mask[..., 3000:] = True
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    o = F.attention(q, k, v, causal=True, mask=mask)
    o.backward(do.detach())
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print(f"peak {peak / 2**20:.1f} MiB, one score tensor "
          f"{h * s * s * 2 / 2**20:.1f} MiB")
    assert peak < h * s * s * 2
    assert q.grad.isfinite().all() and o.isfinite().all()
