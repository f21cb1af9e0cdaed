"""decode_linear_route: which kernel a decode-shaped linear runs, per
FENGSHEN_DECODE_GEMM mode, row count and weight dtype.  No GPU needed."""
import pytest
import torch

from fengshen_amd.ops import functional as F_ops

BF16, INT8 = torch.bfloat16, torch.int8


def _old(rows, dtype):
    """what ran before decode_gemm existed"""
    if dtype == INT8:
        return "gemv" if rows <= 16 else "library"
    return "gemv" if rows == 1 else "library"


@pytest.mark.parametrize("dtype", [BF16, INT8], ids=["bf16", "int8"])
@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_route_by_rows(mode, dtype):
    lo = F_ops._DECODE_GEMM_MIN_ROWS[dtype]
    assert lo is None or 3 <= lo <= 16
    for rows in {1, 2, (lo or 3) - 1, lo or 3, 16, 17}:
        new = 2 <= rows <= 16 and (
            mode == "1" or (mode == "auto" and lo is not None and rows >= lo))
        want = "decode_gemm" if new else _old(rows, dtype)
        assert F_ops.decode_linear_route(rows, 5120, dtype, True, False,
                                         mode) == want, rows


@pytest.mark.parametrize("dtype", [BF16, INT8], ids=["bf16", "int8"])
@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_route_untouched_calls(mode, dtype):
    route = F_ops.decode_linear_route
    # K = 96 is fine for the GEMVs (K % 16) but not for decode_gemm (K % 64)
    assert route(8, 96, dtype, True, False, mode) == _old(8, dtype)
    assert route(8, 5120, dtype, False, False, mode) == "library"  # CPU
    assert route(8, 5120, torch.float16, True, False, mode) == "library"
    # grad enabled: F.linear for bf16 weights, w8_gemv as before for int8
    assert route(8, 5120, dtype, True, True, mode) == (
        "gemv" if dtype == INT8 else "library")
    assert route(1, 5120, BF16, True, True, mode) == "library"


def test_linear_on_cpu_is_f_linear(monkeypatch):
    torch.manual_seed(0)
    x, w, b = torch.randn(4, 1, 128), torch.randn(24, 128), torch.randn(24)
    for mode in ("0", "1", "auto"):
        monkeypatch.setenv("FENGSHEN_DECODE_GEMM", mode)
        for xx, ww in ((x, w), (x.bfloat16(), w.bfloat16())):
            with torch.no_grad():
                assert torch.equal(F_ops.linear(xx, ww),
                                   torch.nn.functional.linear(xx, ww))
        assert torch.equal(F_ops.linear(x, w, b),
                           torch.nn.functional.linear(x, w, b))
    monkeypatch.setenv("FENGSHEN_DECODE_GEMM", "2")
    with pytest.raises(ValueError, match="FENGSHEN_DECODE_GEMM"):
        F_ops.linear(x, w)
