"""Grouped-query attention on the CPU: layer construction, the K/V expansion
of F_ops.attention, HF LLaMA parity (weights, logits, greedy generation with
a 2-KV-head cache) and the head-count checks."""
import pytest
import torch

from fengshen_amd.models.layers import ParallelAttention, check_kv_heads
from fengshen_amd.ops import functional as F_ops


def test_layer_constructs_and_runs():
    torch.manual_seed(0)
    attn = ParallelAttention(64, 4, causal=True, num_kv_heads=2)
    assert attn.qkv_proj.weight.shape == ((4 + 2 * 2) * 16, 64)
    x = torch.randn(2, 8, 64, requires_grad=True)
    out = attn(x)
    assert out.shape == (2, 8, 64)
    out.sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert torch.isfinite(attn.qkv_proj.weight.grad).all()


@pytest.mark.parametrize("h,h_kv", [(4, 2), (4, 1), (6, 2)])
def test_attention_equals_expanded(h, h_kv):
    torch.manual_seed(1)
    b, s, d, g = 2, 12, 16, h // h_kv
    q = torch.randn(b, h, s, d, requires_grad=True)
    k = torch.randn(b, h_kv, s, d, requires_grad=True)
    v = torch.randn(b, h_kv, s, d, requires_grad=True)
    do = torch.randn(b, h, s, d)
    out = F_ops.attention(q, k, v, causal=True)
    gq, gk, gv = torch.autograd.grad(out, (q, k, v), do)

    ke = k.detach().repeat_interleave(g, dim=1).requires_grad_()
    ve = v.detach().repeat_interleave(g, dim=1).requires_grad_()
    qe = q.detach().clone().requires_grad_()
    ref = F_ops.attention(qe, ke, ve, causal=True)
    rq, rk, rv = torch.autograd.grad(ref, (qe, ke, ve), do)
    assert torch.allclose(out, ref)
    assert torch.allclose(gq, rq)
    assert torch.allclose(gk, rk.view(b, h_kv, g, s, d).sum(2))
    assert torch.allclose(gv, rv.view(b, h_kv, g, s, d).sum(2))


@pytest.fixture(scope="module")
def hf_pair():
    transformers = pytest.importorskip("transformers")
    from fengshen_amd.models.llama.configuration_llama import llama_tiny_config
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.utils.llama_convert import hf_to_fs_llama

    torch.manual_seed(0)
    hf_cfg = transformers.LlamaConfig(
        vocab_size=256, hidden_size=64, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=2, intermediate_size=128,
        rms_norm_eps=1e-6, max_position_embeddings=128,
        tie_word_embeddings=False, pad_token_id=0, bos_token_id=1,
        eos_token_id=2)
    hf = transformers.LlamaForCausalLM(hf_cfg).float().eval()
    fs_sd = hf_to_fs_llama(hf.state_dict(), 2)
    ours = LlamaForCausalLM(llama_tiny_config(num_key_value_heads=2,
                                              torch_dtype="float32")).float()
    missing, unexpected = ours.load_state_dict(fs_sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return hf, ours.eval(), fs_sd


def test_hf_logits_parity(hf_pair):
    hf, ours, _ = hf_pair
    torch.manual_seed(2)
    ids = torch.randint(3, 256, (2, 32))
    with torch.no_grad():
        ref = hf(ids).logits
        out = ours(ids).logits
    err = (out - ref).abs().max().item()
    print(f"max |logits - HF| = {err:.3e}, range {ref.abs().max().item():.3f}")
    assert err < 1e-5


def test_fs_to_hf_roundtrip_kv_rows(hf_pair):
    from fengshen_amd.utils.llama_convert import fs_to_hf_llama

    hf, _, fs_sd = hf_pair
    back = fs_to_hf_llama(fs_sd, 2)
    hf_sd = hf.state_dict()
    for i in range(2):
        for name in ("q_proj", "k_proj", "v_proj"):
            key = f"model.layers.{i}.self_attn.{name}.weight"
            assert torch.equal(back[key], hf_sd[key]), key
        assert back[f"model.layers.{i}.self_attn.k_proj.weight"].shape \
            == (32, 64)
        assert back[f"model.layers.{i}.self_attn.v_proj.weight"].shape \
            == (32, 64)


def test_generate_matches_hf_with_two_kv_heads(hf_pair):
    from transformers import DynamicCache

    hf, ours, _ = hf_pair
    torch.manual_seed(3)
    ids = torch.randint(3, 256, (1, 8))
    with torch.no_grad():
        ref = hf.generate(ids, max_new_tokens=8, do_sample=False,
                          use_cache=True)
        gen = ours.generate(ids, max_new_tokens=8, do_sample=False,
                            use_cache=True)
        # the same greedy decode by hand, to look into the cache
        cache = DynamicCache()
        seq = ids
        out = ours(seq, past_key_values=cache, use_cache=True)
        for _ in range(8):
            nxt = out.logits[:, -1].argmax(-1, keepdim=True)
            seq = torch.cat([seq, nxt], dim=1)
            out = ours(nxt, past_key_values=cache, use_cache=True)
    assert ref.shape[1] == 16
    assert torch.equal(gen, ref)
    assert torch.equal(seq, ref)
    layer0 = cache.layers[0].keys if hasattr(cache, "layers") \
        else cache.key_cache[0]
    assert layer0.shape[1] == 2


def test_bad_head_counts_raise():
    with pytest.raises(ValueError):
        ParallelAttention(64, 4, causal=True, num_kv_heads=3)
    # one KV head cannot be split over a tensor-parallel group of 2
    with pytest.raises(ValueError):
        check_kv_heads(4, 1, 2)
    check_kv_heads(4, 2, 2)
