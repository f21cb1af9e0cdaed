"""Block-sparse flash kernels (csrc/sparse_flash.hip) against fp32 dense
attention under the expanded layout.  All tests require an MI355X.

Tolerances are the project's flash tolerances (tests/test_ops_gpu.py):
relative-to-range 2e-2 for O and 3e-2 for each gradient."""
import math

import pytest
import torch

from tests.test_sparse_flash_cpu import make_config

pytestmark = pytest.mark.gpu

FWD_TOL = 2e-2
BWD_TOL = 3e-2


def _hip_ready():
    if not torch.cuda.is_available():
        return False
    from fengshen_amd.ops import has_ext
    return has_ext()


@pytest.fixture(autouse=True)
def _require_ext(monkeypatch):
    assert _hip_ready(), "HIP extension missing on GPU box"
    monkeypatch.delenv("FENGSHEN_SPARSE_FLASH", raising=False)


def _rand(*shape, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(*shape, generator=g, device="cuda",
                       dtype=torch.float32).to(torch.bfloat16)


def _close(a, b, tol=FWD_TOL, what=""):
    """relative-to-range closeness (bf16 outputs vs fp32 oracle)."""
    a = a.float()
    b = b.float()
    scale = b.abs().max().clamp(min=1.0)
    err = (a - b).abs().max() / scale
    print(f"{what} rel err {err.item():.4g} (scale {scale.item():.3g})")
    assert err.item() < tol, \
        f"{what} rel err {err.item():.4g} (scale {scale.item():.3g})"


def _visibility(cfg, s, key_keep=None, b=1):
    """[b, h, s, s] bool on the GPU: layout, causal triangle in
    unidirectional mode (as the eager path applies it), key mask."""
    B = cfg.block
    lay = cfg.make_layout(s)
    vis = lay.repeat_interleave(B, 1).repeat_interleave(B, 2).cuda()
    if cfg.attention == "unidirectional":
        vis = vis & torch.tril(torch.ones(s, s, dtype=torch.bool,
                                          device="cuda"))
    vis = vis[None].expand(b, -1, -1, -1)
    if key_keep is not None:
        vis = vis & (key_keep.cuda() != 0)[:, None, None, :]
    return vis


def _oracle(q, k, v, do, vis, scale):
    """fp32 dense attention with -inf masks.  Rows with no visible key are
    excluded: they return 0 and carry no gradient (their scores are left
    unmasked so the softmax stays finite, then the row is zeroed)."""
    qf, kf, vf = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    row_ok = vis.any(dim=-1, keepdim=True)
    scores = (qf @ kf.transpose(-1, -2)) * scale
    scores = scores.masked_fill(~(vis | ~row_ok), float("-inf"))
    o = torch.softmax(scores, dim=-1) @ vf
    o = o * row_ok
    o.backward(do.float())
    return o.detach(), qf.grad, kf.grad, vf.grad, row_ok[..., 0]


def _run(attn, q, k, v, do, key_keep=None):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    assert attn.uses_kernel(q)
    o = attn(q, k, v, attention_mask=key_keep)
    o.backward(do)
    return o.detach(), q.grad, k.grad, v.grad


def _check_all(cfg, b, h, s, d, seed=0):
    from fengshen_amd.ops.sparse_attention import SparseSelfAttention
    attn = SparseSelfAttention(cfg)
    q, k, v, do = (_rand(b, h, s, d, seed=seed + i) for i in range(4))
    scale = 1.0 / math.sqrt(d)
    got = _run(attn, q, k, v, do)
    vis = _visibility(cfg, s, b=b)
    assert vis.any(dim=-1).all()
    want = _oracle(q, k, v, do, vis, scale)
    for g in got:
        assert torch.isfinite(g.float()).all()
    _close(got[0], want[0], FWD_TOL, "O")
    _close(got[1], want[1], BWD_TOL, "dQ")
    _close(got[2], want[2], BWD_TOL, "dK")
    _close(got[3], want[3], BWD_TOL, "dV")


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fixed", "variable", "local", "bigbird",
                                  "bslongformer"])
def test_five_layouts_fwd_bwd(name):
    # s = 192: partial last query tile (64 of 128 rows), three key tiles
    _check_all(make_config(name, 16, "unidirectional"), 2, 2, 192, 64)


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,block,d", [
    ("local", 32, 128), ("bigbird", 32, 128),
    ("local", 64, 128), ("bigbird", 64, 128),
    ("local", 128, 128), ("bigbird", 128, 128),
    ("fixed", 32, 96), ("bigbird", 16, 96),
])
def test_block_sizes_and_head_dims(name, block, d):
    s = 384 if block > 16 else 192
    _check_all(make_config(name, block, "unidirectional"), 2, 2, s, d,
               seed=10)


# 3 ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["local", "bslongformer"])
def test_bidirectional(name):
    _check_all(make_config(name, 16, "bidirectional"), 2, 2, 192, 64, seed=20)


# 4 ---------------------------------------------------------------------------
def test_key_mask():
    from fengshen_amd.ops.sparse_attention import (
        LocalSlidingWindowSparsityConfig, SparseSelfAttention)
    b, h, s, d = 2, 2, 192, 64
    cfg = LocalSlidingWindowSparsityConfig(h, block=16,
                                           num_sliding_window_blocks=2)
    keep = torch.ones(b, s, dtype=torch.uint8)
    keep[0, 40:71] = 0
    keep[1, 150:] = 0
    keep = keep.cuda()
    attn = SparseSelfAttention(cfg)
    q, k, v, do = (_rand(b, h, s, d, seed=30 + i) for i in range(4))
    o, dq, dk, dv = _run(attn, q, k, v, do, key_keep=keep)
    vis = _visibility(cfg, s, key_keep=keep, b=b)
    wo, wdq, wdk, wdv, row_ok = _oracle(q, k, v, do, vis, 1 / math.sqrt(d))

    # the excluded rows are exactly those without a visible key under the
    # oracle's own mask: 7 (batch 0) + 16 (batch 1) of 384 per head
    assert torch.equal(row_ok, vis.any(dim=-1))
    dead = ~row_ok
    assert dead[:, 0].sum().item() == 7 + 16
    share = dead.float().mean().item()
    assert 0 < share <= 0.10, share

    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()
    assert (o[dead] == 0).all()
    assert (dq[dead] == 0).all()
    _close(o, wo, FWD_TOL, "O")
    _close(dq, wdq, BWD_TOL, "dQ")
    _close(dk, wdk, BWD_TOL, "dK")
    _close(dv, wdv, BWD_TOL, "dV")
    off = (keep == 0)[:, None, :].expand(b, h, s)
    assert (dk[off] == 0).all() and (dv[off] == 0).all()


# 5 ---------------------------------------------------------------------------
def test_fully_masked_batch_element():
    from fengshen_amd.ops.sparse_attention import SparseSelfAttention
    b, h, s, d = 2, 2, 192, 64
    cfg = make_config("bigbird", 16, "unidirectional")
    keep = torch.ones(b, s, dtype=torch.uint8)
    keep[1] = 0
    keep = keep.cuda()
    attn = SparseSelfAttention(cfg)
    q, k, v, do = (_rand(b, h, s, d, seed=40 + i) for i in range(4))
    got = _run(attn, q, k, v, do, key_keep=keep)
    vis = _visibility(cfg, s, key_keep=keep, b=b)
    want = _oracle(q, k, v, do, vis, 1 / math.sqrt(d))
    for g, w, tol, nm in zip(got, want, (FWD_TOL,) + (BWD_TOL,) * 3,
                             ("O", "dQ", "dK", "dV")):
        assert torch.isfinite(g.float()).all()
        assert (g[1] == 0).all(), nm
        _close(g[0], w[0], tol, nm)


# 6 ---------------------------------------------------------------------------
def test_determinism():
    from fengshen_amd.ops.sparse_attention import SparseSelfAttention
    cfg = make_config("bigbird", 16, "unidirectional")
    attn = SparseSelfAttention(cfg)
    q, k, v, do = (_rand(2, 2, 192, 64, seed=i) for i in range(4))
    a = _run(attn, q, k, v, do)
    b = _run(attn, q, k, v, do)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# 7 ---------------------------------------------------------------------------
def test_long_context_memory_and_tail():
    from fengshen_amd.ops.sparse_attention import SparseSelfAttention
    b, h, s, d = 1, 2, 8192, 64
    cfg = make_config("bigbird", 16, "unidirectional")
    attn = SparseSelfAttention(cfg)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    q, k, v, do = (_rand(b, h, s, d, seed=50 + i) for i in range(4))
    o, dq, dk, dv = _run(attn, q, k, v, do)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"peak memory rise {rise / 2**20:.1f} MiB")
    # q, k, v, their clones, O, dO, three gradients (bf16, 2 MiB each) +
    # LSE and delta: ~ 25 MiB; one fp32 [h, s, s] would be 512 MiB
    assert rise < 64 * 2**20, rise
    for t in (o, dq, dk, dv):
        assert torch.isfinite(t.float()).all()

    tail = 256
    lay = cfg.make_layout(s)[:, -(tail // 16):, :]
    vis = lay.repeat_interleave(16, 1).repeat_interleave(16, 2).cuda()
    rows = torch.arange(s - tail, s, device="cuda")[:, None]
    vis = vis & (torch.arange(s, device="cuda")[None, :] <= rows)
    scores = (q[0, :, -tail:].float() @ k[0].float().transpose(-1, -2)) \
        / math.sqrt(d)                                    # [2, 256, 8192]
    scores = scores.masked_fill(~vis, float("-inf"))
    want = torch.softmax(scores, dim=-1) @ v[0].float()
    _close(o[0, :, -tail:], want, FWD_TOL, "O tail")


# 8 ---------------------------------------------------------------------------
def test_routing_and_binding_checks(monkeypatch):
    import fengshen_amd.ops.sparse_flash as sf
    from fengshen_amd.ops import get_ext
    from fengshen_amd.ops.sparse_attention import SparseSelfAttention
    cfg = make_config("bigbird", 16, "unidirectional")
    attn = SparseSelfAttention(cfg)
    q, k, v = (_rand(2, 2, 192, 64, seed=i) for i in range(3))

    calls = []
    real = sf.block_sparse_attention

    def spy(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(sf, "block_sparse_attention", spy)
    kern = attn(q, k, v)
    assert calls == [1]
    monkeypatch.setenv("FENGSHEN_SPARSE_FLASH", "0")
    assert not attn.uses_kernel(q)
    eager = attn(q, k, v)
    assert calls == [1], "FENGSHEN_SPARSE_FLASH=0 must take the eager path"
    # and that is the blockwise result the fp32 GPU path gives
    eager32 = attn(q.float(), k.float(), v.float())
    assert calls == [1]
    _close(eager, eager32, FWD_TOL, "eager bf16 vs fp32")
    _close(kern, eager, FWD_TOL, "kernel vs eager")
    monkeypatch.delenv("FENGSHEN_SPARSE_FLASH")

    ext = get_ext()
    ls = attn.tile_lists(192, q.device)
    scale = 0.125
    args = (ls.row_ptr, ls.row_idx, ls.row_mask, None, scale, True, True)
    ext.sparse_flash_fwd(q, k, v, *args)               # valid lists pass
    bad = ls.row_idx.clone()
    bad[0] = 3                                         # only key tiles 0..2
    with pytest.raises(RuntimeError, match="out of range"):
        ext.sparse_flash_fwd(q, k, v, ls.row_ptr, bad, ls.row_mask, None,
                             scale, True, True)
    with pytest.raises(RuntimeError, match="bf16"):
        ext.sparse_flash_fwd(q.half(), k.half(), v.half(), *args)
    with pytest.raises(RuntimeError, match="device"):
        ext.sparse_flash_fwd(q, k, v, ls.row_ptr.cpu(), ls.row_idx.cpu(),
                             ls.row_mask.cpu(), None, scale, True, True)
    with pytest.raises(RuntimeError, match="expected"):
        ext.sparse_flash_fwd(q, k, v, ls.row_ptr[:-1].contiguous(),
                             ls.row_idx, ls.row_mask, None, scale, True, True)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.sparse_flash_fwd(q.transpose(1, 2), k.transpose(1, 2),
                             v.transpose(1, 2), *args)
    torch.cuda.synchronize()


# 9 ---------------------------------------------------------------------------
def test_tiny_llama_matches_eager_path(monkeypatch):
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, intermediate_size=512,
                      max_position_embeddings=128,
                      attention_config=[[["bigbird"], 2]],
                      sparsity_config={"block": 16})
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda()
    assert all(layer.attention.attention_type == "bigbird"
               for layer in model.model.layers)
    ids = torch.randint(3, 512, (2, 128), device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        out = model(ids, labels=ids)
        out.loss.backward()
        return out.loss.detach().float(), \
            {n: p.grad.detach().clone() for n, p in model.named_parameters()}

    import fengshen_amd.ops.sparse_flash as sf
    calls = []
    real = sf.block_sparse_attention
    monkeypatch.setattr(
        sf, "block_sparse_attention",
        lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    loss_k, grads_k = step()
    assert len(calls) == 2, "both layers must run the kernel path"
    monkeypatch.setenv("FENGSHEN_SPARSE_FLASH", "0")
    loss_e, grads_e = step()
    assert len(calls) == 2
    assert loss_k.isfinite() and loss_e.isfinite()
    _close(loss_k, loss_e, FWD_TOL, "loss")
    assert grads_k.keys() == grads_e.keys()
    for n in grads_k:
        a, b = grads_k[n].float(), grads_e[n].float()
        rng = b.abs().max().clamp(min=1e-6)
        err = ((a - b).abs().max() / rng).item()
        assert err < BWD_TOL, f"{n}: grad rel-to-range err {err:.4g}"
