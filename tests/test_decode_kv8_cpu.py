"""GraphedDecoder's kv_cache option without a GPU: the int8 cache needs the
fused HIP path and never falls back to a bf16 cache."""
import pytest
import torch


def test_kv_cache_option_on_cpu():
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    cfg = LlamaConfig(vocab_size=64, hidden_size=128, num_hidden_layers=1,
                      num_attention_heads=2, intermediate_size=128,
                      max_position_embeddings=32)
    model = LlamaForCausalLM(cfg)
    with pytest.raises(ValueError, match="int8"):
        GraphedDecoder(model, max_len=32, max_new_tokens=4, kv_cache="int8")
    with pytest.raises(ValueError, match="fp8"):
        GraphedDecoder(model, max_len=32, max_new_tokens=4, kv_cache="fp8")
    dec = GraphedDecoder(model, max_len=32, max_new_tokens=4)
    assert dec.kv_cache == "bf16" and dec.k_cache[0].dtype == torch.float32
