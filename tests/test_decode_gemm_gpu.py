"""decode_gemm (MFMA weight-streaming GEMM for 1..16 rows, bf16 and int8
weights) against an fp64 matmul, its binding's checks, and its routes through
F_ops.linear, W8Linear and GraphedDecoder.  Requires an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (K, out, rows): K 64 is less than one k-step, 192 a tail after one bf16
# step, 1088 several steps per wave plus a tail; out 8 is less than a tile,
# 40 a partial last tile, 272 many blocks plus a tail.  Beyond the sizes of
# the issue: K 3392 is the smallest at which every wave of both dtypes turns
# the prefetch ring at least once (26.5 bf16 steps, 13.25 int8 steps), and
# out 30 takes the element-wise store (out % 4 != 0).
SHAPES = [(64, 8, 1), (192, 16, 2), (320, 40, 7), (1088, 272, 8),
          (64, 272, 9), (1088, 40, 16), (192, 8, 16), (320, 16, 9),
          (3392, 40, 7), (3392, 272, 16), (192, 30, 8)]


def _ext():
    from fengshen_amd.ops import get_ext
    return get_ext()


def _inputs(K, out, rows, w8):
    """-> (w, scale or None, x, fp64 weight the kernel should be using)"""
    torch.manual_seed(K + out + rows)
    x = torch.randn(rows, K, device="cuda").bfloat16()
    w = (torch.randn(out, K, device="cuda") * 0.05).bfloat16()
    if not w8:
        return w, None, x, w.double()
    from fengshen_amd.utils.quantize import W8Linear
    q = W8Linear(w)
    scale = q.scale.view(-1)
    return q.qweight, scale, x, q.qweight.double() * scale.double()[:, None]


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "int8"])
@pytest.mark.parametrize("K,out,rows", SHAPES)
def test_matches_fp64(K, out, rows, w8):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 (|x| @ |W|^T): bf16 rounding of the
    output (half an ulp is 2^-9, doubled) plus the worst case of a length-K
    fp32 sum in any order, doubled for the rounding inside the MFMA."""
    w, scale, x, wd = _inputs(K, out, rows, w8)
    y = _ext().decode_gemm(w, x, scale)
    assert y.shape == (rows, out) and y.dtype == torch.bfloat16
    assert torch.isfinite(y).all()
    ref = x.double() @ wd.T
    bound = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * (x.double().abs()
                                                     @ wd.abs().T)
    excess = ((y.double() - ref).abs() - bound).max().item()
    print(f"K={K} out={out} rows={rows} int8={w8}: max(err - bound)={excess}")
    assert excess <= 0


@pytest.mark.parametrize("w8", [False, True], ids=["bf16", "int8"])
@pytest.mark.parametrize("K,out", [(192, 8), (1088, 40), (3392, 272)])
def test_row_independent_and_deterministic(K, out, w8):
    w, scale, x, _ = _inputs(K, out, 16, w8)
    f = _ext().decode_gemm
    y16, y7 = f(w, x, scale), f(w, x[:7], scale)
    assert torch.equal(y16, f(w, x, scale))
    for i in (0, 6, 7, 15):
        one = f(w, x[i:i + 1], scale)[0]
        assert torch.equal(y16[i], one)
        assert i >= 7 or torch.equal(y7[i], one)


def _t(shape, dtype=torch.bfloat16):
    return torch.ones(shape, device="cuda", dtype=dtype)


REJECTS = {
    "rows=17": lambda: (_t((32, 128)), _t((17, 128)), None),
    "K=96": lambda: (_t((32, 96)), _t((4, 96)), None),
    "x not contiguous": lambda: (_t((32, 128)), _t((4, 256))[:, ::2], None),
    "fp16 x": lambda: (_t((32, 128)), _t((4, 128), torch.float16), None),
    "int8 without scale": lambda: (_t((32, 128), torch.int8), _t((4, 128)),
                                   None),
    "bf16 with scale": lambda: (_t((32, 128)), _t((4, 128)),
                                _t(32, torch.float32)),
    "scale of wrong length": lambda: (_t((32, 128), torch.int8),
                                      _t((4, 128)), _t(31, torch.float32)),
}


@pytest.mark.parametrize("case", list(REJECTS))
def test_binding_rejects(case):
    w, x, scale = REJECTS[case]()
    with pytest.raises(RuntimeError, match="decode_gemm: "):
        _ext().decode_gemm(w, x, scale)


def test_linear_and_w8linear_route(monkeypatch):
    from fengshen_amd.ops import functional as F_ops
    from fengshen_amd.utils.quantize import W8Linear
    ext, K, out = _ext(), 320, 40
    w, _, x, _ = _inputs(K, out, 4, False)
    x3 = x.view(4, 1, K)
    q = W8Linear(w).cuda()
    qs = q.scale.view(-1)
    with torch.no_grad():
        monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "1")
        assert torch.equal(F_ops.linear(x3, w),
                           ext.decode_gemm(w, x).view(4, 1, out))
        assert torch.equal(q(x3),
                           ext.decode_gemm(q.qweight, x, qs).view(4, 1, out))
        monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "0")
        assert torch.equal(F_ops.linear(x3, w),
                           torch.nn.functional.linear(x3, w))
        assert torch.equal(q(x3),
                           ext.w8_gemv(q.qweight, qs, x).view(4, 1, out))
    monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "1")
    wg = w.clone().requires_grad_()
    F_ops.linear(x3, wg).float().sum().backward()
    assert torch.allclose(wg.grad.float(),
                          x.float().sum(0).expand(out, K), rtol=2e-2)


def test_graph_replay_and_decoder(monkeypatch):
    """As in test_graphed_decode_ragged_matches_single, the prompts are ones
    whose fp32 greedy path keeps a top-2 logit gap above 0.05 over the 8
    compared steps and emits no EOS (rows found on the CPU; asserted)."""
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    ext = _ext()
    w, scale, x, _ = _inputs(320, 40, 8, True)
    xs = x.clone()
    ext.decode_gemm(w, xs, scale)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ext.decode_gemm(w, xs, scale)
    for shift in (1, 2, 3):
        xs.copy_(x.roll(shift, 0) * shift)
        graph.replay()
        assert torch.equal(y, ext.decode_gemm(w, xs.clone(), scale))

    monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "1")
    torch.manual_seed(11)
    cfg = LlamaConfig(vocab_size=512, hidden_size=256, num_hidden_layers=2,
                      num_attention_heads=4, num_key_value_heads=2,
                      intermediate_size=512, max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16)
    ids = torch.randint(3, 512, (256, 16))[[80, 89, 97, 126]].cuda()
    m32 = LlamaForCausalLM(cfg).float()
    m32.load_state_dict({k: v.float() for k, v in model.state_dict().items()})
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
