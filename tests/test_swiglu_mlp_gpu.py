"""swiglu_bwd_act against the two kernels it combines, bit for bit, and the
fused MLP tail of a checkpointed LLaMA against FENGSHEN_FUSED_MLP=0.

All comparisons are on integer views of the raw bits, so NaN positions and
signed zeros count.  All tests require an MI355X."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

# rows x h.  The grid is capped at 2048 blocks of 256 threads x 8 elements =
# 4194304 elements per pass of the grid-stride loop; 1025 x 4104 = 4206600
# leaves a short second pass.
SHAPES = [(1, 8), (3, 1408), (5, 13824), (1025, 4104)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
_INT_VIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16,
             torch.float32: torch.int32}
# __expf overflow / underflow edges of the sigmoid
EDGE_GATES = [100.0, -100.0, float("inf"), float("-inf"), 0.0, -0.0, 88.0,
              -88.0, 89.0, -89.0, 104.0, -104.0]


@pytest.fixture(autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"


def _bits(t):
    return t.contiguous().view(_INT_VIEW[t.dtype])


def _inputs(rows, h, dtype):
    g = torch.Generator(device="cuda").manual_seed(rows * 100003 + h)
    packed = (3.0 * torch.randn(rows, 2 * h, generator=g, device="cuda",
                                dtype=torch.float32))
    # edge gate values spread over the gate half, first and last row
    edges = torch.tensor(EDGE_GATES, device="cuda")
    n = min(h, edges.numel())
    packed[0, :n] = edges[:n]
    packed[-1, h - n:h] = edges[:n]
    gy = torch.randn(rows, h, generator=g, device="cuda", dtype=torch.float32)
    return gy.to(dtype), packed.to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
@pytest.mark.parametrize("rows,h", SHAPES)
def test_bwd_act_bit_equal(rows, h, dtype):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    gy, packed = _inputs(rows, h, dtype)
    gpacked_r = ext.swiglu_bwd(gy, packed)
    act_r = ext.swiglu_fwd(packed)
    gpacked, act = ext.swiglu_bwd_act(gy, packed)
    assert gpacked.shape == packed.shape and act.shape == gy.shape
    assert gpacked.dtype == dtype and act.dtype == dtype
    assert torch.equal(_bits(gpacked), _bits(gpacked_r))
    assert torch.equal(_bits(act), _bits(act_r))


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp16", "fp32"])
def test_bwd_act_aliased_onto_gy(dtype):
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    rows, h = SHAPES[-1]
    gy, packed = _inputs(rows, h, dtype)
    gpacked_r = ext.swiglu_bwd(gy, packed)
    act_r = ext.swiglu_fwd(packed)
    buf = gy.clone()
    gpacked, act = ext.swiglu_bwd_act(buf, packed, buf)
    assert act.data_ptr() == buf.data_ptr()
    assert torch.equal(_bits(gpacked), _bits(gpacked_r))
    assert torch.equal(_bits(buf), _bits(act_r))


def test_bwd_act_given_output_buffer():
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    gy, packed = _inputs(3, 1408, torch.bfloat16)
    out = torch.empty_like(gy)
    _gp, act = ext.swiglu_bwd_act(gy, packed, out)
    assert act.data_ptr() == out.data_ptr()
    assert torch.equal(_bits(out), _bits(ext.swiglu_fwd(packed)))


def test_binding_rejects_bad_arguments():
    """Host-side checks: nothing is launched."""
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    gy, packed = _inputs(4, 32, torch.bfloat16)
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.swiglu_bwd_act(gy, packed.t().contiguous().t())
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.swiglu_bwd_act(gy.t().contiguous().t(), packed)
    with pytest.raises(RuntimeError, match="dtype"):
        ext.swiglu_bwd_act(gy.float(), packed)
    with pytest.raises(RuntimeError, match="shape"):
        ext.swiglu_bwd_act(gy[:, :16].contiguous(), packed)
    with pytest.raises(RuntimeError, match="shape"):
        ext.swiglu_bwd_act(gy[:3].contiguous(), packed)
    with pytest.raises(RuntimeError, match="divisible by 16"):
        ext.swiglu_bwd_act(gy[:, :12].contiguous(),
                           packed[:, :24].contiguous())
    with pytest.raises(RuntimeError, match="shape"):
        ext.swiglu_bwd_act(gy, packed, torch.empty_like(packed))
    with pytest.raises(RuntimeError, match="dtype"):
        ext.swiglu_bwd_act(gy, packed, torch.empty_like(gy).float())


class _env:
    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("FENGSHEN_FUSED_MLP")
        os.environ["FENGSHEN_FUSED_MLP"] = self.value

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop("FENGSHEN_FUSED_MLP", None)
        else:
            os.environ["FENGSHEN_FUSED_MLP"] = self.old


def _model_run(fused, skip_interval):
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    with _env("1" if fused else "0"):
        torch.manual_seed(3)
        cfg = LlamaConfig(vocab_size=128, hidden_size=64,
                          num_hidden_layers=2, num_attention_heads=4,
                          intermediate_size=176, max_position_embeddings=64)
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().train()
        model.gradient_checkpointing_enable(skip_interval=skip_interval)
        ids = torch.randint(3, 128, (2, 16),
                            generator=torch.Generator().manual_seed(5)).cuda()
        loss = model(ids, labels=ids).loss
        loss.backward()
        torch.cuda.synchronize()
        return loss.detach(), {n: p.grad for n, p in model.named_parameters()}


@pytest.mark.parametrize("skip_interval", [0, 2])
def test_llama_checkpointed_equals_unfused(skip_interval):
    loss, grads = _model_run(True, skip_interval)
    loss_r, grads_r = _model_run(False, skip_interval)
    assert torch.equal(loss, loss_r)
    assert grads.keys() == grads_r.keys() and grads
    for n in grads:
        assert grads[n] is not None and grads_r[n] is not None, n
        assert torch.equal(_bits(grads[n]), _bits(grads_r[n])), n
