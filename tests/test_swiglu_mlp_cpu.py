"""F_ops.swiglu_mlp_residual (the SwiGLU MLP and its residual add as one
autograd node) against the composition it replaces, and the recompute flag
that lets a checkpointed LLaMA layer skip the down projection.

On the CPU both sides run the same eager ops in the same order, so every
comparison is torch.equal."""
import os

import pytest
import torch

from fengshen_amd.ops import functional as F_ops

SHAPES = [((2, 3, 16), 24), ((1, 5, 32), 40)]
DTYPES = [torch.float32, torch.bfloat16]


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


def _inputs(shape, ffn, dtype):
    g = torch.Generator().manual_seed(7)
    hid = shape[-1]

    def r(*s):
        return torch.randn(*s, generator=g).to(dtype)
    return (r(*shape), r(*shape), 0.3 * r(2 * ffn, hid), 0.3 * r(hid, ffn),
            r(*shape))


def _run(fn, shape, ffn, dtype):
    h2, res, wgu, wd, gy = _inputs(shape, ffn, dtype)
    leaves = [t.requires_grad_(True) for t in (h2, res, wgu, wd)]
    out = fn(*leaves)
    out.backward(gy)
    return out.detach(), [t.grad for t in leaves]


def _composition(h2, res, wgu, wd):
    packed = torch.nn.functional.linear(h2, wgu)
    act = F_ops.swiglu(packed)
    out = torch.nn.functional.linear(act, wd)
    return F_ops.bias_dropout_add(out, None, res, 0.0, True)


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,ffn", SHAPES)
def test_node_equals_composition(shape, ffn, dtype):
    out_r, grads_r = _run(_composition, shape, ffn, dtype)
    out, grads = _run(F_ops.swiglu_mlp_residual, shape, ffn, dtype)
    assert torch.equal(out, out_r)
    for name, a, r in zip(("h2", "residual", "w_gate_up", "w_down"),
                          grads, grads_r):
        assert a.shape == r.shape and a.dtype == r.dtype, name
        assert torch.equal(a, r), name


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
@pytest.mark.parametrize("shape,ffn", SHAPES)
def test_output_unused_keeps_gradients(shape, ffn, dtype):
    _out_r, grads_r = _run(_composition, shape, ffn, dtype)
    out, grads = _run(
        lambda *a: F_ops.swiglu_mlp_residual(*a, output_unused=True),
        shape, ffn, dtype)
    assert out.shape == torch.Size(shape) and out.dtype == dtype
    for name, a, r in zip(("h2", "residual", "w_gate_up", "w_down"),
                          grads, grads_r):
        assert torch.equal(a, r), name


def _tiny_llama():
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    torch.manual_seed(3)
    cfg = LlamaConfig(vocab_size=128, hidden_size=64, num_hidden_layers=2,
                      num_attention_heads=4, intermediate_size=176,
                      max_position_embeddings=64)
    return LlamaForCausalLM(cfg)


def _model_run(fused, skip_interval):
    with _env("1" if fused else "0"):
        model = _tiny_llama().train()
        model.gradient_checkpointing_enable(skip_interval=skip_interval)
        ids = torch.randint(3, 128, (2, 16),
                            generator=torch.Generator().manual_seed(5))
        loss = model(ids, labels=ids).loss
        loss.backward()
        return loss.detach(), {n: p.grad for n, p in model.named_parameters()}


@pytest.fixture(scope="module")
def unfused_model_runs():
    return {skip: _model_run(False, skip) for skip in (0, 2)}


def _assert_same_run(run, ref):
    loss, grads = run
    loss_r, grads_r = ref
    assert torch.equal(loss, loss_r)
    assert grads.keys() == grads_r.keys() and grads
    for n in grads:
        assert grads[n] is not None and grads_r[n] is not None, n
        assert torch.equal(grads[n], grads_r[n]), n


@pytest.mark.parametrize("skip_interval", [0, 2])
def test_llama_checkpointed_equals_unfused(skip_interval, unfused_model_runs):
    _assert_same_run(_model_run(True, skip_interval),
                     unfused_model_runs[skip_interval])


@pytest.mark.parametrize("skip_interval", [0, 2])
def test_llama_never_reads_unused_output(skip_interval, unfused_model_runs,
                                         monkeypatch):
    calls = []

    def nan_like(t):
        calls.append(1)
        return torch.full_like(t, float("nan"))
    monkeypatch.setattr(F_ops, "_unused_output_like", nan_like)
    _assert_same_run(_model_run(True, skip_interval),
                     unfused_model_runs[skip_interval])
    # skip 0 recomputes both layers, skip 2 stores the second one
    assert len(calls) == (2 if skip_interval == 0 else 1)


def test_in_recompute_flag():
    from fengshen_amd.parallel.random import checkpoint, in_recompute
    seen = []

    def fn(x):
        seen.append(in_recompute())
        return x * 2

    assert not in_recompute()
    x = torch.ones(3, requires_grad=True)
    y = checkpoint(fn, x)
    assert seen == [False] and not in_recompute()
    y.sum().backward()
    assert seen == [False, True] and not in_recompute()

    def boom(x):
        if in_recompute():
            raise RuntimeError("boom")
        return x * 2

    y = checkpoint(boom, torch.ones(3, requires_grad=True))
    with pytest.raises(RuntimeError, match="boom"):
        y.sum().backward()
    assert not in_recompute()


def test_nested_checkpoint_forward_is_not_a_recompute():
    """A checkpoint whose forward runs inside another one's recompute
    produces an output that IS used."""
    from fengshen_amd.parallel.random import checkpoint, in_recompute
    seen = []

    def inner(x):
        seen.append(in_recompute())
        return x * 3

    def outer(x):
        return checkpoint(inner, x) + 1

    x = torch.ones(3, requires_grad=True)
    checkpoint(outer, x).sum().backward()
    # outer forward, inner forward inside outer's recompute, inner recompute
    assert seen == [False, False, True]
    assert torch.equal(x.grad, torch.full((3,), 3.0))


def test_eval_layer_forward_unchanged():
    from fengshen_amd.models.layers import ParallelTransformerLayer
    torch.manual_seed(2)
    layer = ParallelTransformerLayer(
        64, 4, causal=True, norm="rmsnorm", norm_eps=1e-6, mlp_type="swiglu",
        ffn_hidden_size=176, rotary=True, max_positions=64, bias=False).eval()
    x = torch.randn(2, 16, 64, generator=torch.Generator().manual_seed(4))
    with torch.no_grad():
        with _env("1"):
            out = layer(x)
        with _env("0"):
            out_r = layer(x)
    assert torch.equal(out, out_r)
