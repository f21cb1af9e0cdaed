"""decode_attn_split(..., tokens=T): the multi-token split-KV decode kernel
(decode_attn_mt.hip) against fp64 per-token attention, and greedy lookahead
decoding in GraphedDecoder.  Tolerances are those of
tests/test_decode_split_gpu.py: 0.03 on the context, 0.02 on the written K
rows; V rows are copies.  Requires an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

B, L = 2, 256


def _rot(x):
    x1, x2 = x.chunk(2, -1)
    return torch.cat((-x2, x1), -1)


def _inputs(h, h_kv, d, T, seed):
    """As _inputs of tests/test_decode_split_gpu.py, with T rows of qkv."""
    from fengshen_amd.ops import functional as F_ops
    torch.manual_seed(seed)
    qkv = (torch.randn(B, T, (h + 2 * h_kv) * d, device="cuda")
           * 0.5).bfloat16()
    kc = (torch.randn(B, h_kv, L, d, device="cuda") * 0.5).bfloat16()
    vc = (torch.randn(B, h_kv, L, d, device="cuda") * 0.5).bfloat16()
    cos, sin = F_ops.build_rope_cache(L, d)
    return qkv, kc, vc, cos.cuda(), sin.cuda()


def _check(ctx, kc2, vc2, qkv, kc, vc, cos, sin, pos, h, h_kv, d, T):
    """ctx against fp64 attention of token t over keys 0..pos_b+t, rows pos_b..
    taken from the roped k / the v of qkv; the T written rows; every other
    cache element keeps its bits (NaN rows included)."""
    g = h // h_kv
    q, k, v = qkv.double().split([h * d, h_kv * d, h_kv * d], dim=2)
    q, k = q.view(B, T, h, d), k.view(B, T, h_kv, d)
    at = torch.tensor(pos, device="cuda")[:, None] + torch.arange(
        T, device="cuda")
    c, s = cos[at].double()[:, :, None], sin[at].double()[:, :, None]
    q, k = q * c + _rot(q) * s, k * c + _rot(k) * s
    assert ctx.shape == (B, T, h * d) and ctx.isfinite().all()
    want_k, want_v = kc.clone(), vc.clone()
    for i, pi in enumerate(pos):
        kr = torch.cat([kc[i, :, :pi].double(), k[i].transpose(0, 1)], 1)
        vr = torch.cat([vc[i, :, :pi].double(),
                        v[i].view(T, h_kv, d).transpose(0, 1)], 1)
        kr, vr = kr.repeat_interleave(g, 0), vr.repeat_interleave(g, 0)
        for t in range(T):
            att = torch.einsum("hd,hld->hl", q[i, t], kr[:, :pi + t + 1])
            ref = torch.einsum("hl,hld->hd", (att / math.sqrt(d)).softmax(-1),
                               vr[:, :pi + t + 1])
            err = (ctx[i, t].view(h, d).double() - ref).abs().max()
            assert err < 0.03, (i, t, float(err))
        rows = slice(pi, pi + T)
        kerr = (kc2[i, :, rows].double() - k[i].transpose(0, 1)).abs().max()
        assert kerr < 0.02, float(kerr)
        vnew = qkv[i, :, (h + h_kv) * d:].view(T, h_kv, d).transpose(0, 1)
        assert torch.equal(vc2[i, :, rows], vnew)
        want_k[i, :, rows], want_v[i, :, rows] = kc2[i, :, rows], vnew
    assert torch.equal(kc2.view(torch.int16), want_k.view(torch.int16))
    assert torch.equal(vc2.view(torch.int16), want_v.view(torch.int16))


_HK = [(4, 4), (8, 2), (20, 1)]
_D = [64, 96, 128]
_T = [2, 4, 5, 16]
_NS = [1, 3]
# "end" is L - T.  [62, 126] with T = 5: the new rows straddle a tile (62..66)
# and, with nsplit 3, the chunks [0,64) [64,128) [128,131) of sequence 1
_POS = [[0, "end"], [62, 126], [201, 60]]
# an eighth of the product with every value of every axis, plus T*G = 16
# exactly ((8,2), T 4), ragged last column groups ((8,2) with T 5 on the tile
# and split boundaries, (20,1) with T 2) for several head dims, and MHA at
# pos 0 / L - T
_CASES = [(hk, d, T, n, p)
          for i, hk in enumerate(_HK) for j, d in enumerate(_D)
          for k, T in enumerate(_T) for m, n in enumerate(_NS)
          for q, p in enumerate(_POS)
          if (i + j + k + m + q) % 8 == 0
          or (i == 1 and k in (1, 2) and q == 1 and j % 2 == m)
          or (i == 2 and k == 0 and m == 1 and j == q)
          or (i == 0 and q == 0 and j == k % 3 and m == k % 2)]


@pytest.mark.parametrize("hk,d,T,nsplit,pos", _CASES)
def test_multitok_matches_fp64(hk, d, T, nsplit, pos):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv = hk
    pos = [L - T if p == "end" else p for p in pos]
    qkv, kc, vc, cos, sin = _inputs(h, h_kv, d, T, h * 100 + d + T + nsplit)
    for i, pi in enumerate(pos):  # rows the kernel must not let through
        kc[i, :, pi:], vc[i, :, pi:] = float("nan"), float("nan")
    post = torch.tensor(pos, device="cuda")
    scale = 1 / math.sqrt(d)
    kc2, vc2 = kc.clone(), vc.clone()
    ctx = ext.decode_attn_split(qkv, kc2, vc2, cos, sin, post, scale, True,
                                nsplit, tokens=T)
    _check(ctx, kc2, vc2, qkv, kc, vc, cos, sin, pos, h, h_kv, d, T)
    kc3, vc3 = kc.clone(), vc.clone()
    ctx3 = ext.decode_attn_split(qkv, kc3, vc3, cos, sin, post, scale, True,
                                 nsplit, tokens=T)
    assert torch.equal(ctx3, ctx)
    assert torch.equal(kc3.view(torch.int16), kc2.view(torch.int16))
    assert torch.equal(vc3.view(torch.int16), vc2.view(torch.int16))


def test_tokens_1_is_the_single_token_call():
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    qkv, kc, vc, cos, sin = _inputs(8, 2, 128, 1, 5)
    qkv = qkv.view(B, -1)
    pos = torch.tensor([77, 130], device="cuda")
    kc2, vc2 = kc.clone(), vc.clone()
    ctx = ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, 0.125, True, 3)
    ctx2 = ext.decode_attn_split(qkv, kc2, vc2, cos, sin, pos, 0.125, True, 3,
                                 tokens=1)
    assert torch.equal(ctx, ctx2)
    assert torch.equal(kc, kc2) and torch.equal(vc, vc2)


def test_multitok_graph_replay():
    """The grid and the chunking do not depend on the captured pos."""
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d, T = 8, 2, 128, 5
    qkv, kc, vc, cos, sin = _inputs(h, h_kv, d, T, 7)
    pos = torch.tensor([10, 100], device="cuda")
    scale = 1 / math.sqrt(d)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, scale, True, 3,
                              tokens=T)
    torch.cuda.current_stream().wait_stream(st)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ctx = ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, scale, True,
                                    3, tokens=T)
    for new_pos in ([200, 62], [L - T, 0]):
        pos.copy_(torch.tensor(new_pos, device="cuda"))
        qkv.copy_((torch.randn_like(qkv, dtype=torch.float) * 0.5).bfloat16())
        kc0, vc0 = kc.clone(), vc.clone()
        graph.replay()
        torch.cuda.synchronize()
        _check(ctx, kc, vc, qkv, kc0, vc0, cos, sin, new_pos, h, h_kv, d, T)


@pytest.mark.parametrize("case", ["tokens0", "tokens17", "qkv2d", "short_L",
                                  "clamp"])
def test_multitok_binding_rejects(case):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d = 4, 2, 64
    T = {"tokens0": 0, "tokens17": 17, "clamp": 4}.get(case, 2)
    qkv, kc, vc, cos, sin = _inputs(h, h_kv, d, max(T, 1), 3)
    pos = torch.tensor([5, 9], device="cuda")
    if case == "qkv2d":
        qkv = qkv.view(B, -1)
    elif case == "short_L":
        kc, vc = kc[:, :, :1].contiguous(), vc[:, :, :1].contiguous()
    elif case == "clamp":  # out-of-range positions are clamped, not trusted
        pos = torch.tensor([L + 7, -3], device="cuda")
        kc2, vc2 = kc.clone(), vc.clone()
        ctx = ext.decode_attn_split(qkv, kc2, vc2, cos, sin, pos, 0.125, True,
                                    2, tokens=T)
        assert ctx.isfinite().all()
        for new, old in ((kc2, kc), (vc2, vc)):  # rows [L-T, L) and [0, T)
            assert torch.equal(new[0, :, :L - T], old[0, :, :L - T])
            assert torch.equal(new[1, :, T:], old[1, :, T:])
        return
    with pytest.raises(RuntimeError, match="decode_attn_split:"):
        ext.decode_attn_split(qkv, kc, vc, cos, sin, pos, 0.125, True, 2,
                              tokens=T)


def test_graphed_decode_lookahead_matches_greedy():
    """Model and pattern of test_graphed_decode_ragged_matches_single: two
    right-padded prompts of lengths 16 and 9.  lookahead=4 gives the greedy
    tokens of the fp32 path with and without a hint, and with the true
    continuation as the hint it needs fewer replays than tokens.  The seed is
    one whose fp32 greedy path keeps a top-2 logit gap above 0.05 over the 10
    steps of both prompts and emits no EOS; asserted before the comparison."""
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    torch.manual_seed(1323)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ids = torch.randint(3, 512, (2, 16)).cuda()
    m32 = LlamaForCausalLM(cfg).float()
    m32.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    model, m32 = model.cuda().eval(), m32.cuda().eval()
    lens, n = [16, 9], 10
    want = []
    with torch.no_grad():
        for i, ln in enumerate(lens):
            seq = ids[i:i + 1, :ln]
            for _ in range(n):
                top = m32(seq).logits[:, -1].topk(2, dim=-1)
                assert (top.values[:, 0] - top.values[:, 1]).min() > 0.05
                assert (top.indices[:, 0] != cfg.eos_token_id).all()
                seq = torch.cat([seq, top.indices[:, :1]], dim=1)
            want.append(seq[0])

    padded = ids.clone()
    padded[1, 9:] = 0
    dec = GraphedDecoder(model, batch=2, max_len=64, max_new_tokens=n,
                         lookahead=4)
    hint = torch.stack([w[ln:] for w, ln in zip(want, lens)])
    for hint_ids in (None, hint):
        out = dec.generate(padded, prompt_lens=torch.tensor(lens),
                           hint_ids=hint_ids)
        for i in range(2):
            assert torch.equal(out[i], want[i]), (out[i], want[i])
        assert 1 <= dec.last_replays <= n - 1
    assert dec.last_replays < n - 1  # the hinted call

    for bad in (dict(kv_cache="int8"), dict(do_sample=True)):
        with pytest.raises(ValueError, match="lookahead"):
            GraphedDecoder(model, batch=2, max_len=64, max_new_tokens=n,
                           lookahead=4, **bad)
