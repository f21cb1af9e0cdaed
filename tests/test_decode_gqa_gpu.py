"""Grouped-query decode: decode_attn on [b, h_kv, L, d] caches and the graphed
decoder on a 2-KV-head LLaMA.  Tolerances are those of
test_decode_attn_matches_eager (0.02 cache row, 0.03 context) against an
fp32 eager reference on expanded caches.  Requires an MI355X."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _rot(x):
    x1, x2 = x.chunk(2, -1)
    return torch.cat((-x2, x1), -1)


@pytest.mark.parametrize("pos_i", [0, 127, 128, 200])
@pytest.mark.parametrize("d", [64, 128])
@pytest.mark.parametrize("h,h_kv", [(4, 2), (4, 1)])
def test_decode_attn_gqa_matches_eager(h, h_kv, d, pos_i):
    from fengshen_amd.ops import functional as F_ops
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    assert ext is not None
    torch.manual_seed(h * 100 + h_kv * 10 + d + pos_i)
    b, L, g = 2, 256, h // h_kv
    qkv = (torch.randn(b, (h + 2 * h_kv) * d, device="cuda") * 0.5).bfloat16()
    kc = (torch.randn(b, h_kv, L, d, device="cuda") * 0.5).bfloat16()
    vc = (torch.randn(b, h_kv, L, d, device="cuda") * 0.5).bfloat16()
    cos, sin = F_ops.build_rope_cache(L, d)
    cos, sin = cos.cuda(), sin.cuda()
    pos = torch.tensor([pos_i], device="cuda")
    scale = 1 / math.sqrt(d)

    kc2, vc2 = kc.clone(), vc.clone()
    ctx = ext.decode_attn(qkv, kc2, vc2, cos, sin, pos, scale, True)
    torch.cuda.synchronize()
    assert ctx.shape == (b, h * d)

    q, k, v = qkv.float().split([h * d, h_kv * d, h_kv * d], dim=1)
    q, k, v = q.view(b, h, d), k.view(b, h_kv, d), v.view(b, h_kv, d)
    c, s = cos[pos_i], sin[pos_i]
    q = q * c + _rot(q) * s
    k = k * c + _rot(k) * s
    assert (kc2[:, :, pos_i].float() - k).abs().max() < 0.02
    assert (vc2[:, :, pos_i].float() - v).abs().max() < 0.02
    # every other cache row is untouched
    keep = torch.ones(L, dtype=torch.bool, device="cuda")
    keep[pos_i] = False
    assert torch.equal(kc2[:, :, keep], kc[:, :, keep])
    assert torch.equal(vc2[:, :, keep], vc[:, :, keep])

    # fp32 reference on caches expanded to h heads (head j <- KV head j // g)
    kr, vr = kc.float(), vc.float()
    kr[:, :, pos_i], vr[:, :, pos_i] = k, v
    kr = kr[:, :, :pos_i + 1].repeat_interleave(g, dim=1)
    vr = vr[:, :, :pos_i + 1].repeat_interleave(g, dim=1)
    att = torch.einsum("bhd,bhld->bhl", q, kr) * scale
    ref = torch.einsum("bhl,bhld->bhd", att.softmax(-1), vr)
    err = (ctx.view(b, h, d).float() - ref).abs().max()
    assert err < 0.03, float(err)

    # a second call on fresh clones gives the same bits
    kc3, vc3 = kc.clone(), vc.clone()
    ctx3 = ext.decode_attn(qkv, kc3, vc3, cos, sin, pos, scale, True)
    torch.cuda.synchronize()
    assert torch.equal(ctx3, ctx)
    assert torch.equal(kc3, kc2) and torch.equal(vc3, vc2)


def test_graphed_decode_gqa_matches_eager_generate():
    """hipGraph-captured decode on 2-KV-head caches gives the greedy tokens
    of generate() on the eager path.

    Greedy tokens of two bf16 paths can only be compared where the argmax
    is not a near-tie: a randomly initialised model of this size has top-2
    logit gaps below bf16 noise (a few 1e-3 at logits of order 1) at about
    every third step.  The seed is therefore one whose fp32 greedy path
    keeps a top-2 gap of 0.05 (over 10 bf16 ulps) through the 8 compared
    steps and emits no EOS; that is a property of the inputs, computed from
    an fp32 copy of the model, and is asserted here before the comparison."""
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    torch.manual_seed(182)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ids = torch.randint(3, 512, (2, 16)).cuda()
    m32 = LlamaForCausalLM(cfg).float()
    m32.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    model, m32 = model.cuda().eval(), m32.cuda().eval()
    seq = ids
    with torch.no_grad():
        for _ in range(8):
            top = m32(seq).logits[:, -1].topk(2, dim=-1)
            assert (top.values[:, 0] - top.values[:, 1]).min() > 0.05
            assert (top.indices[:, 0] != cfg.eos_token_id).all()
            seq = torch.cat([seq, top.indices[:, :1]], dim=1)

    ref = model.generate(ids, max_new_tokens=12, do_sample=False)
    dec = GraphedDecoder(model, batch=2, max_len=64, max_new_tokens=12)
    assert dec._fused_attn           # head dim 64: the fused kernel
    assert dec.k_cache[0].shape[1] == 2
    out = dec.generate(ids, max_new_tokens=12)
    # as test_graphed_decode_matches_eager_generate: the first 8 of 12
    # greedy tokens are identical
    assert torch.equal(out[:, 16:24], ref[:, 16:24]), (
        out[:, 16:].tolist(), ref[:, 16:].tolist())
    assert torch.equal(ref[:, 16:24], seq[:, 16:])
