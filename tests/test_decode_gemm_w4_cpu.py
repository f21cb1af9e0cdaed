"""int4 weight format (pack_int4 / unpack_int4 / W4Linear) and the int4 case
of decode_linear_route.  No GPU needed."""
import pytest
import torch

from fengshen_amd.ops import functional as F_ops
from fengshen_amd.utils.quantize import W4Linear, pack_int4, unpack_int4


@pytest.mark.parametrize("out,K", [(8, 128), (72, 256), (200, 640)])
def test_pack_roundtrip_and_layout(out, K):
    torch.manual_seed(out + K)
    q = torch.randint(-7, 8, (out, K), dtype=torch.int8)
    sc = (torch.rand(out, K // 128) + 0.01).bfloat16()
    qw, sp = pack_int4(q, sc)
    out_pad = -(-out // 64) * 64
    assert qw.shape == (out_pad // 16, K // 128, 64, 16)
    assert qw.dtype == torch.uint8 and sp.shape == (K // 128, out_pad)
    q2, sc2 = unpack_int4(qw, sp, out, dequant=False)
    assert torch.equal(q2, q) and torch.equal(sc2, sc)
    assert torch.equal(unpack_int4(qw, sp, out),
                       q.float() * sc.float().repeat_interleave(128, 1))
    # pad rows: u = 8 in both nibbles, scale 0
    assert (qw.view(out_pad // 16, -1, 4, 16, 16)
            .permute(0, 3, 1, 2, 4).reshape(out_pad, -1)[out:] == 0x88).all()
    assert (sp[:, out:] == 0).all()
    # the documented nibble order, read the way the kernel does
    row, k = out - 1, K - 128 + 32 * 2 + 8 * 3  # group K/128-1, g 2, dword 3
    b = qw[row // 16, K // 128 - 1, 16 * 2 + row % 16, 12:16].tolist()
    dw = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24
    for i in range(4):
        pair = (dw >> 4 * i) & 0x000F000F
        assert pair & 0xFFFF == q[row, k + 2 * i] + 8
        assert pair >> 16 == q[row, k + 2 * i + 1] + 8


def test_quantisation_error_and_cpu_forward():
    torch.manual_seed(0)
    w = torch.randn(72, 256) * torch.tensor([0.05, 2.0]).repeat_interleave(128)
    b = torch.randn(72)
    lin = W4Linear(w, b)
    q, sc = unpack_int4(lin.qweight, lin.scales, 72, dequant=False)
    assert q.abs().max() == 7
    assert torch.equal(
        sc, (w.double().view(72, 2, 128).abs().amax(2) / 7).bfloat16())
    wd = lin.dequantized()
    half = sc.double().repeat_interleave(128, 1) / 2
    assert ((w.double() - wd.double()).abs() <= half).all()
    x = torch.randn(3, 2, 256)
    for xx in (x, x.bfloat16()):
        want = torch.nn.functional.linear(xx, wd.to(xx.dtype)) + b.to(xx.dtype)
        assert torch.equal(lin(xx), want)


def test_constructor_rejects():
    with pytest.raises(ValueError, match="128"):
        W4Linear(torch.randn(16, 192))
    with pytest.raises(ValueError, match="group_size"):
        W4Linear(torch.randn(16, 128), group_size=64)


@pytest.mark.parametrize("mode", ["0", "1", "auto"])
def test_route_int4(mode):
    route = F_ops.decode_linear_route
    for rows in (1, 16, 17):
        for K in (128, 192):
            for grad in (False, True):
                new = rows <= 16 and K == 128 and not grad and mode != "0"
                assert route(rows, K, torch.uint8, True, grad, mode) == (
                    "decode_gemm_w4" if new else "library"), (rows, K, grad)
                assert route(rows, K, torch.uint8, False, grad,
                             mode) == "library"
