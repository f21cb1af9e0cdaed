"""decode_gemm_w4 (split-K MFMA GEMM for int4 weights, 1..16 rows) against an
fp64 matmul on the dequantised weight, its binding's checks, and its routes
through W4Linear and GraphedDecoder.  Requires an MI355X."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (K, out, rows).  K 128 is one group and one step, 256 the smallest chunk
# that splits, 640 five groups (uneven over 2 and 3 splits), 3456 twenty-seven
# (four LDS passes at ksplit 1, and every wave turns its register ring); out 8
# is less than one tile, 72 a partial second 64-row block (and, for tw = 2, a
# wave whose second tile does not exist), 200 takes the vector store.
SHAPES = [(128, 8, 1), (128, 72, 16), (256, 200, 7), (256, 8, 16),
          (640, 72, 7), (640, 200, 16), (3456, 72, 1), (3456, 200, 16),
          (3456, 8, 7)]
CASES = [(K, out, rows, ks) for K, out, rows in SHAPES for ks in (0, 1, 2, 3)
         if ks <= K // 128]


def _ext():
    from fengshen_amd.ops import get_ext
    return get_ext()


@functools.lru_cache(maxsize=None)
def _inputs(K, out):
    """-> (W4Linear on the GPU, x [16, K] bf16, fp64 dequantised weight).
    Neighbouring 128-k groups differ in magnitude, so a scale applied to the
    wrong group shows."""
    from fengshen_amd.utils.quantize import W4Linear
    torch.manual_seed(K + out)
    factor = torch.tensor([1.0, 4.0, 0.5, 2.0]).repeat(K // 128 // 4 + 1)
    w = torch.randn(out, K) * 0.05 * factor[:K // 128].repeat_interleave(128)
    lin = W4Linear(w).cuda()
    x = torch.randn(16, K, device="cuda").bfloat16()
    return lin, x, lin.dequantized().double()


@pytest.mark.parametrize("tw", [1, 2])
@pytest.mark.parametrize("K,out,rows,ksplit", CASES)
def test_matches_fp64(K, out, rows, ksplit, tw):
    """The bound of test_decode_gemm_gpu.py on the dequantised weight:
    |y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |W_d|^T)."""
    lin, x, wd = _inputs(K, out)
    x = x[:rows]
    y = _ext().decode_gemm_w4(lin.qweight, lin.scales, x, out, ksplit, tw)
    assert y.shape == (rows, out) and y.dtype == torch.bfloat16
    assert torch.isfinite(y).all()
    ref = x.double() @ wd.T
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x.double().abs()
                                                     @ wd.abs().T)
    err = (y.double() - ref).abs()
    print(f"K={K} out={out} rows={rows} ksplit={ksplit} tw={tw}: "
          f"max(err - bound)={(err - bound).max().item()} "
          f"max(err / bound)={(err / bound).max().item()}")
    assert (err <= bound).all()


@pytest.mark.parametrize("ksplit", [0, 1, 3])
@pytest.mark.parametrize("K,out", [(640, 72), (3456, 200)])
def test_row_independent_and_deterministic(K, out, ksplit):
    lin, x, _ = _inputs(K, out)

    def f(xx):
        return _ext().decode_gemm_w4(lin.qweight, lin.scales, xx, out, ksplit)
    y16, y7 = f(x), f(x[:7])
    assert torch.equal(y16, f(x))
    for i in (0, 6, 7, 15):
        one = f(x[i:i + 1])[0]
        assert torch.equal(y16[i], one)
        assert i >= 7 or torch.equal(y7[i], one)


def _t(shape, dtype=torch.bfloat16, device="cuda"):
    return torch.ones(shape, device=device, dtype=dtype)


def _good():
    return dict(qweight=_t((4, 2, 64, 16), torch.uint8), scales=_t((2, 64)),
                x=_t((4, 256)), out=40, ksplit=0)


REJECTS = {
    "int8 qweight": dict(qweight=lambda: _t((4, 2, 64, 16), torch.int8)),
    "qweight lanes": dict(qweight=lambda: _t((4, 2, 32, 16), torch.uint8)),
    "out_pad % 64": dict(qweight=lambda: _t((3, 2, 64, 16), torch.uint8),
                         scales=lambda: _t((2, 48))),
    "scales shape": dict(scales=lambda: _t((2, 40))),
    "fp32 scales": dict(scales=lambda: _t((2, 64), torch.float32)),
    "out=0": dict(out=lambda: 0),
    "out>out_pad": dict(out=lambda: 65),
    "fp16 x": dict(x=lambda: _t((4, 256), torch.float16)),
    "x of another K": dict(x=lambda: _t((4, 128))),
    "x not contiguous": dict(x=lambda: _t((4, 512))[:, ::2]),
    "rows=17": dict(x=lambda: _t((17, 256))),
    "scales on the CPU": dict(scales=lambda: _t((2, 64), device="cpu")),
    "x misaligned": dict(x=lambda: _t(4 * 256 + 4)[4:].view(4, 256)),
    "ksplit=3": dict(ksplit=lambda: 3),
    "ksplit=-1": dict(ksplit=lambda: -1),
}


@pytest.mark.parametrize("case", list(REJECTS))
def test_binding_rejects(case):
    args = _good()
    args.update({k: v() for k, v in REJECTS[case].items()})
    with pytest.raises(RuntimeError, match="decode_gemm_w4: "):
        _ext().decode_gemm_w4(**args)


def test_w4linear_routes(monkeypatch):
    lin, x, wd = _inputs(640, 72)
    x3 = x[:4].view(4, 1, 640)
    with torch.no_grad():
        monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "auto")
        direct = _ext().decode_gemm_w4(lin.qweight, lin.scales, x[:4], 72)
        assert torch.equal(lin(x3), direct.view(4, 1, 72))
        monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "0")
        assert torch.equal(lin(x3), torch.nn.functional.linear(
            x3, wd.to(torch.bfloat16)))


def test_graph_replay_and_decoder(monkeypatch):
    """Prompts as in test_decode_gemm_gpu.py: rows whose greedy path under
    the fp32 model with the dequantised int4 weights keeps a top-2 logit gap
    above 0.05 over the 8 compared steps and emits no EOS (found on the CPU;
    asserted)."""
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    from fengshen_amd.utils.quantize import W4Linear, quantize_model_int4
    ext = _ext()
    lin, x, _ = _inputs(640, 72)
    xs = x[:8].clone()

    def f(xx):
        return ext.decode_gemm_w4(lin.qweight, lin.scales, xx, 72, 2)
    f(xs)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = f(xs)
    for shift in (1, 2, 3):
        xs.copy_(x[:8].roll(shift, 0) * shift)
        graph.replay()
        assert torch.equal(y, f(xs.clone()))

    monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "auto")
    torch.manual_seed(11)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ids = torch.randint(3, 512, (256, 16))[[63, 80, 97, 233]].cuda()
    m32 = LlamaForCausalLM(cfg).float()
    m32.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
    model = quantize_model_int4(model)
    nq = 0
    for name, mod in model.named_modules():
        if isinstance(mod, W4Linear):
            m32.get_submodule(name).weight.data.copy_(mod.dequantized())
            nq += 1
    assert nq == 2 * 4 + 1  # four projections per layer and the LM head
    model, m32 = model.cuda().eval(), m32.cuda().eval()
    want = ids
    with torch.no_grad():
        for _ in range(8):
            top = m32(want).logits[:, -1].topk(2, dim=-1)
            assert (top.values[:, 0] - top.values[:, 1]).min() > 0.05
            assert (top.indices[:, 0] != cfg.eos_token_id).all()
            want = torch.cat([want, top.indices[:, :1]], dim=1)
    dec = GraphedDecoder(model, batch=4, max_len=64, max_new_tokens=8)
    assert dec._fused_attn
    out = dec.generate(ids, max_new_tokens=8)
    ref = model.generate(ids, max_new_tokens=8, do_sample=False)
    assert torch.equal(out, ref), (out, ref)
    assert torch.equal(ref, want)

