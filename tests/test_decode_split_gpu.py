"""decode_attn_split (split-KV grouped decode with per-sequence positions)
against fp64 eager attention, and the ragged-prompt path of GraphedDecoder.
Inputs and tolerances are those of tests/test_decode_gqa_gpu.py: 0.02 on the
written cache rows, 0.03 on the context.  Requires an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 2, 256


def _rot(x):
    x1, x2 = x.chunk(2, -1)
    return torch.cat((-x2, x1), -1)


def _inputs(h, h_kv, d, seed):
    from fengshen_amd.ops import functional as F_ops
    torch.manual_seed(seed)
    qkv = (torch.randn(B, (h + 2 * h_kv) * d, device="cuda") * 0.5).bfloat16()
    kc = (torch.randn(B, h_kv, L, d, device="cuda") * 0.5).bfloat16()
    vc = (torch.randn(B, h_kv, L, d, device="cuda") * 0.5).bfloat16()
    cos, sin = F_ops.build_rope_cache(L, d)
    return qkv, kc, vc, cos.cuda(), sin.cuda()


def _reference(qkv, kc, vc, cos, sin, pos, h, h_kv, d):
    """fp64 attention over keys 0..pos_b of caches expanded to h heads, row
    pos_b replaced by the roped k / the v of qkv.  Returns ctx [B, h, d] and
    the new rows [B, h_kv, d]."""
    g = h // h_kv
    q, k, v = qkv.double().split([h * d, h_kv * d, h_kv * d], dim=1)
    q, k, v = q.view(B, h, d), k.view(B, h_kv, d), v.view(B, h_kv, d)
    p = torch.tensor(pos, device="cuda")
    c, s = cos[p].double()[:, None], sin[p].double()[:, None]
    q, k = q * c + _rot(q) * s, k * c + _rot(k) * s
    ctx = torch.empty(B, h, d, dtype=torch.float64, device="cuda")
    for i, pi in enumerate(pos):
        kr = torch.cat([kc[i, :, :pi].double(), k[i, :, None]], 1)
        vr = torch.cat([vc[i, :, :pi].double(), v[i, :, None]], 1)
        kr, vr = kr.repeat_interleave(g, 0), vr.repeat_interleave(g, 0)
        att = torch.einsum("hd,hld->hl", q[i], kr) / math.sqrt(d)
        ctx[i] = torch.einsum("hl,hld->hd", att.softmax(-1), vr)
    return ctx, k, v


def _check(ctx, kc2, vc2, qkv, kc, vc, cos, sin, pos, h, h_kv, d):
    ref, k, v = _reference(qkv, kc, vc, cos, sin, pos, h, h_kv, d)
    assert ctx.shape == (B, h * d) and ctx.isfinite().all()
    err = (ctx.view(B, h, d).double() - ref).abs().max()
    assert err < 0.03, float(err)
    want_k, want_v = kc.clone(), vc.clone()
    for i, pi in enumerate(pos):
        assert (kc2[i, :, pi].double() - k[i]).abs().max() < 0.02
        assert (vc2[i, :, pi].double() - v[i]).abs().max() < 0.02
        want_k[i, :, pi], want_v[i, :, pi] = kc2[i, :, pi], vc2[i, :, pi]
    # every other element keeps its bits (NaN rows included)
    assert torch.equal(kc2.view(torch.int16), want_k.view(torch.int16))
    assert torch.equal(vc2.view(torch.int16), want_v.view(torch.int16))


_HK = [(4, 4), (8, 2), (16, 1), (20, 1)]
_D = [64, 96, 128]
_POS = [[0, 63], [64, 200], [255, 129]]
_NS = [1, 3, 4]
# a third of the product: every value of every axis, plus the pairs
# (pos [0, 63], nsplit 4) and (G = 20, nsplit 3) for every head dim
_CASES = [(hk, d, p, n)
          for i, hk in enumerate(_HK) for j, d in enumerate(_D)
          for k, p in enumerate(_POS) for m, n in enumerate(_NS)
          if (i + j + k + m) % 3 == 0 or (k == 0 and m == 2 and i % 3 == j)
          or (i == 3 and m == 1 and k == j)]


@pytest.mark.parametrize("hk,d,pos,nsplit", _CASES)
def test_split_matches_fp64(hk, d, pos, nsplit):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv = hk
    qkv, kc, vc, cos, sin = _inputs(h, h_kv, d, h * 100 + d + pos[0] + nsplit)
    for i, pi in enumerate(pos):  # rows the kernel must not let through
        kc[i, :, pi:], vc[i, :, pi:] = float("nan"), float("nan")
    post = torch.tensor(pos, device="cuda")
    scale = 1 / math.sqrt(d)
    kc2, vc2 = kc.clone(), vc.clone()
    ctx = ext.decode_attn_split(qkv, kc2, vc2, cos, sin, post, scale, True,
                                nsplit)
    _check(ctx, kc2, vc2, qkv, kc, vc, cos, sin, pos, h, h_kv, d)
    kc3, vc3 = kc.clone(), vc.clone()
    ctx3 = ext.decode_attn_split(qkv, kc3, vc3, cos, sin, post, scale, True,
                                 nsplit)
    assert torch.equal(ctx3, ctx)
    assert torch.equal(kc3.view(torch.int16), kc2.view(torch.int16))
    assert torch.equal(vc3.view(torch.int16), vc2.view(torch.int16))


def test_split_graph_replay():
    """The grid and the chunking do not depend on the captured pos."""
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d = 8, 2, 128
    qkv, kc, vc, cos, sin = _inputs(h, h_kv, d, 7)
    pos = torch.tensor([10, 100], device="cuda")
    scale = 1 / math.sqrt(d)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, scale, True, 3)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx = ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, scale, True, 3)
    for new_pos in ([200, 31], [255, 0]):
        pos.copy_(torch.tensor(new_pos, device="cuda"))
        qkv.copy_((torch.randn_like(qkv, dtype=torch.float) * 0.5).bfloat16())
        kc0, vc0 = kc.clone(), vc.clone()
        graph.replay()
        torch.cuda.synchronize()
        _check(ctx, kc, vc, qkv, kc0, vc0, cos, sin, new_pos, h, h_kv, d)


@pytest.mark.parametrize("case", ["pos_dtype", "pos_numel", "d80", "h_mod",
                                  "nsplit65", "cos_short", "clamp"])
def test_split_binding_rejects(case):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d = (6, 4, 64) if case == "h_mod" else (4, 2, 64)
    d = 80 if case == "d80" else d
    qkv, kc, vc, cos, sin = _inputs(h, h_kv, d, 3)
    pos = torch.tensor([5, 9], device="cuda")
    nsplit = 65 if case == "nsplit65" else 2
    if case == "pos_dtype":
        pos = pos.int()
    elif case == "pos_numel":
        pos = torch.tensor([5, 9, 3], device="cuda")
    elif case == "cos_short":
        cos, sin = cos[:L - 1].contiguous(), sin[:L - 1].contiguous()
    elif case == "clamp":  # out-of-range positions are clamped, not trusted
        pos = torch.tensor([L + 7, -3], device="cuda")
        ctx = ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, 0.125, True,
                                    nsplit)
        assert ctx.isfinite().all()
        return
    with pytest.raises(RuntimeError, match="decode_attn_split"):
        ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, 0.125, True, nsplit)


def test_graphed_decode_ragged_matches_single():
    """Two right-padded prompts of lengths 16 and 9 in one graphed batch give
    the greedy tokens of generate() on each prompt alone.  As in
    test_graphed_decode_gqa_matches_eager_generate the seed is one whose fp32
    greedy path keeps a top-2 logit gap above 0.05 over the 8 compared steps
    of both prompts and emits no EOS; asserted before the comparison."""
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    torch.manual_seed(321)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ids = torch.randint(3, 512, (2, 16)).cuda()
    m32 = LlamaForCausalLM(cfg).float()
    m32.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    model, m32 = model.cuda().eval(), m32.cuda().eval()
    lens = [16, 9]
    prompts = [ids[i:i + 1, :n] for i, n in enumerate(lens)]
    want = []
    with torch.no_grad():
        for seq in prompts:
            for _ in range(8):
                top = m32(seq).logits[:, -1].topk(2, dim=-1)
                assert (top.values[:, 0] - top.values[:, 1]).min() > 0.05
                assert (top.indices[:, 0] != cfg.eos_token_id).all()
                seq = torch.cat([seq, top.indices[:, :1]], dim=1)
            want.append(seq[0])

    padded = ids.clone()
    padded[1, 9:] = 0
    dec = GraphedDecoder(model, batch=2, max_len=64, max_new_tokens=12)
    assert dec._fused_attn
    out = dec.generate(padded, max_new_tokens=12,
                       prompt_lens=torch.tensor(lens))
    for i, n in enumerate(lens):
        ref = model.generate(prompts[i], max_new_tokens=8, do_sample=False)
        assert out[i].shape == (n + 12,)
        assert torch.equal(out[i][:n + 8], ref[0]), (out[i], ref[0])
        assert torch.equal(ref[0], want[i])

    cfg96 = LlamaConfig(vocab_size=512, hidden_size=384, num_hidden_layers=1,
                        num_attention_heads=4, intermediate_size=512,
                        max_position_embeddings=128)
    m96 = LlamaForCausalLM(cfg96).to(torch.bfloat16).cuda()
    assert GraphedDecoder(m96, batch=1, max_len=64,
                          max_new_tokens=4)._fused_attn
