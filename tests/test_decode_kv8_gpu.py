"""decode_attn_split_q8 (split-KV decode over an int8 KV cache with one fp32
scale per row), kv_quantize_int8 and GraphedDecoder(kv_cache="int8") against
fp64.  Shapes, input scale and the 0.03 context bound are those of
tests/test_decode_split_gpu.py.  The context reference reads the cache back
after the call, so P's bf16 rounding is the only error it leaves to the
kernel; a quantised element may be off by half a step (0.501 * scale).
Requires an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 2, 256


def _rot(x):
    x1, x2 = x.chunk(2, -1)
    return torch.cat((-x2, x1), -1)


def _quant(x):
    """The cache format in torch ops: int8 rows, fp32 scale per row."""
    x = x.float()
    amax = x.abs().amax(-1, keepdim=True)
    inv = torch.where(amax > 0, 127 / amax, torch.zeros_like(amax))
    q = (x * inv).round().clamp(-127, 127).to(torch.int8)
    return q, (amax / 127).squeeze(-1)


def _inputs(h, h_kv, d, seed):
    from fengshen_amd.ops import functional as F_ops
    torch.manual_seed(seed)
    qkv = (torch.randn(B, (h + 2 * h_kv) * d, device="cuda") * 0.5).bfloat16()
    kq, ks = _quant((torch.randn(B, h_kv, L, d, device="cuda") * 0.5).bfloat16())
    vq, vs = _quant((torch.randn(B, h_kv, L, d, device="cuda") * 0.5).bfloat16())
    cos, sin = F_ops.build_rope_cache(L, d)
    return qkv, [kq, ks, vq, vs], cos.cuda(), sin.cuda()


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _check(ctx, new, old, qkv, cos, sin, pos, h, h_kv, d):
    """new / old: [kq, k_scale, vq, v_scale] after / before the call."""
    g = h // h_kv
    q, k, v = qkv.double().split([h * d, h_kv * d, h_kv * d], dim=1)
    q, k, v = q.view(B, h, d), k.view(B, h_kv, d), v.view(B, h_kv, d)
    p = torch.tensor(pos, device="cuda")
    c, s = cos[p].double()[:, None], sin[p].double()[:, None]
    q, k = q * c + _rot(q) * s, k * c + _rot(k) * s
    kd = new[0].double() * new[1].double()[..., None]
    vd = new[2].double() * new[3].double()[..., None]
    want = [t.clone() for t in old]
    assert ctx.shape == (B, h * d) and ctx.isfinite().all()
    for i, pi in enumerate(pos):
        kr = kd[i, :, :pi + 1].repeat_interleave(g, 0)
        vr = vd[i, :, :pi + 1].repeat_interleave(g, 0)
        att = torch.einsum("hd,hld->hl", q[i], kr) / math.sqrt(d)
        ref = torch.einsum("hl,hld->hd", att.softmax(-1), vr)
        err = (ctx[i].view(h, d).double() - ref).abs().max()
        print(f"ctx err {float(err):.5f}")
        assert err < 0.03, float(err)
        for row, deq, sc in ((k[i], kd[i, :, pi], new[1][i, :, pi].double()),
                             (v[i], vd[i, :, pi], new[3][i, :, pi].double())):
            amax = row.abs().amax(-1)
            assert ((sc - amax / 127).abs() <= 1e-5 * amax / 127).all()
            assert ((deq - row).abs() <= 0.501 * sc[:, None]).all()
        for w, n in zip(want, new):
            w[i, :, pi] = n[i, :, pi]
    # every other byte keeps its bits (NaN scales included)
    for w, n in zip(want, new):
        assert torch.equal(_bits(w), _bits(n))


_HK = [(4, 4), (8, 2), (20, 1)]
_D = [64, 128]
_POS = [[0, 63], [64, 200], [255, 129]]
_NS = [1, 3, 4]
# a third of the product: every value of every axis, plus the pairs
# (pos [0, 63], nsplit 4) and (G = 20, nsplit 3) for both head dims
_CASES = [(hk, d, p, n)
          for i, hk in enumerate(_HK) for j, d in enumerate(_D)
          for k, p in enumerate(_POS) for m, n in enumerate(_NS)
          if (i + j + k + m) % 3 == 0 or (k == 0 and m == 2 and i == j)
          or (i == 2 and m == 1 and k == j)]


@pytest.mark.parametrize("hk,d,pos,nsplit", _CASES)
def test_q8_matches_fp64(hk, d, pos, nsplit):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv = hk
    qkv, old, cos, sin = _inputs(h, h_kv, d, h * 100 + d + pos[0] + nsplit)
    for i, pi in enumerate(pos):  # rows the kernel must not let through
        old[0][i, :, pi:], old[2][i, :, pi:] = 127, 127
        old[1][i, :, pi:], old[3][i, :, pi:] = float("nan"), float("nan")
    post = torch.tensor(pos, device="cuda")
    scale = 1 / math.sqrt(d)
    new = [t.clone() for t in old]
    ctx = ext.decode_attn_split_q8(qkv, *new, cos, sin, post, scale, True,
                                   nsplit)
    _check(ctx, new, old, qkv, cos, sin, pos, h, h_kv, d)
    again = [t.clone() for t in old]
    ctx2 = ext.decode_attn_split_q8(qkv, *again, cos, sin, post, scale, True,
                                    nsplit)
    assert torch.equal(ctx2, ctx)
    for a, n in zip(again, new):
        assert torch.equal(_bits(a), _bits(n))


def test_q8_graph_replay():
    """The grid and the chunking do not depend on the captured pos."""
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d = 8, 2, 128
    qkv, cache, cos, sin = _inputs(h, h_kv, d, 7)
    pos = torch.tensor([10, 100], device="cuda")
    scale = 1 / math.sqrt(d)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ext.decode_attn_split_q8(qkv, *cache, cos, sin, pos, scale, True, 3)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx = ext.decode_attn_split_q8(qkv, *cache, cos, sin, pos, scale,
                                       True, 3)
    for new_pos in ([200, 31], [255, 0]):
        pos.copy_(torch.tensor(new_pos, device="cuda"))
        qkv.copy_((torch.randn_like(qkv, dtype=torch.float) * 0.5).bfloat16())
        old = [t.clone() for t in cache]
        graph.replay()
        torch.cuda.synchronize()
        _check(ctx, cache, old, qkv, cos, sin, new_pos, h, h_kv, d)


@pytest.mark.parametrize("d", [64, 128])
def test_kv_quantize_int8(d):
    from fengshen_amd.ops import get_ext
    torch.manual_seed(d)
    x = (torch.randn(3, 111, d, device="cuda") * 0.5).bfloat16()
    x[1, 5] = 0
    q, sc = get_ext().kv_quantize_int8(x)
    q_ref, sc_ref = _quant(x)
    assert q.dtype == torch.int8 and q.shape == x.shape
    assert sc.dtype == torch.float32 and sc.shape == x.shape[:-1]
    # ties under -ffast-math may fall either way
    assert (q.int() - q_ref.int()).abs().max() <= 1
    assert ((q.double() * sc.double()[..., None] - x.double()).abs()
            <= 0.501 * sc.double()[..., None]).all()
    assert ((sc - sc_ref).abs() <= 1e-6 * sc_ref).all()
    assert sc[1, 5] == 0 and (q[1, 5] == 0).all()


@pytest.mark.parametrize("case", ["d96", "bf16_cache", "scale_short",
                                  "pos_dtype", "nsplit65", "clamp"])
def test_q8_binding_rejects(case):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    d = 96 if case == "d96" else 64
    qkv, cache, cos, sin = _inputs(4, 2, d, 3)
    pos = torch.tensor([5, 9], device="cuda")
    nsplit = 65 if case == "nsplit65" else 2
    if case == "bf16_cache":
        cache[0], cache[2] = cache[0].bfloat16(), cache[2].bfloat16()
    elif case == "scale_short":
        cache[1] = cache[1][:, :, :L - 1].contiguous()
    elif case == "pos_dtype":
        pos = pos.int()
    elif case == "clamp":  # out-of-range positions are clamped, not trusted
        pos = torch.tensor([L + 7, -3], device="cuda")
        ctx = ext.decode_attn_split_q8(qkv, *cache, cos, sin, pos, 0.125,
                                       True, nsplit)
        assert ctx.isfinite().all()
        return
    with pytest.raises(RuntimeError, match="decode_attn_split_q8"):
        ext.decode_attn_split_q8(qkv, *cache, cos, sin, pos, 0.125, True,
                                 nsplit)


def test_graphed_decode_int8_cache(monkeypatch):
    """Layer 0's K cache depends on the tokens only: every row below a
    sequence's final position, dequantised, is rope(W_k norm(embed(token)))
    of the emitted sequence within 0.02 (the project's bound for a written
    bf16 row) + 0.501 * scale.  That pins prefill quantisation, the per-step
    append and the per-sequence positions together."""
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    torch.manual_seed(321)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().eval()
    ids = torch.randint(3, 512, (2, 16)).cuda()
    ids[1, 9:] = 0
    lens, n, hd, nkv = [16, 9], 8, 64, 2
    dec = GraphedDecoder(model, batch=2, max_len=64, max_new_tokens=n,
                         kv_cache="int8")
    out = dec.generate(ids, prompt_lens=torch.tensor(lens))
    for c, s in zip(dec.k_cache + dec.v_cache, dec.k_scale + dec.v_scale):
        assert c.dtype == torch.int8 and c.shape == (2, nkv, 64, hd)
        assert s.dtype == torch.float32 and s.shape == (2, nkv, 64)
    kd = dec.k_cache[0].double() * dec.k_scale[0].double()[..., None]
    layer = model.model.layers[0]
    wk = layer.attention.qkv_proj.weight.double()[4 * hd:(4 + nkv) * hd]
    for i, ln in enumerate(lens):
        rows = ln + n - 1  # the last token emitted was not fed back
        x = model.model.embed_tokens.weight.double()[out[i][:rows]]
        x = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True)
                            + layer.input_norm.eps)
        k = (x * layer.input_norm.weight.double()) @ wk.T
        k = k.view(rows, nkv, hd).transpose(0, 1)
        k = k * dec.cos[:rows].double() + _rot(k) * dec.sin[:rows].double()
        bound = 0.02 + 0.501 * dec.k_scale[0][i, :, :rows, None].double()
        assert ((kd[i, :, :rows] - k).abs() <= bound).all()
    again = dec.generate(ids, prompt_lens=torch.tensor(lens))
    assert all(torch.equal(a, o) for a, o in zip(again, out))

    monkeypatch.setenv("FENGSHEN_DECODE_SPLIT", "0")
    with pytest.raises(ValueError, match="int8"):
        GraphedDecoder(model, batch=2, max_len=64, kv_cache="int8")
    monkeypatch.delenv("FENGSHEN_DECODE_SPLIT")
    cfg96 = LlamaConfig(vocab_size=512, hidden_size=384, num_hidden_layers=1,
                        num_attention_heads=4, intermediate_size=512,
                        max_position_embeddings=128)
    m96 = LlamaForCausalLM(cfg96).to(torch.bfloat16).cuda()
    with pytest.raises(ValueError, match="int8"):
        GraphedDecoder(m96, batch=1, max_len=64, kv_cache="int8")
