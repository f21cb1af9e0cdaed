"""XCD-aware block map of the flash v3 kernels (csrc/flash_blockmap.h).

The kernels no longer take (x, head, batch) from blockIdx but from a map of
the hardware's linear block id, so that the blocks which share an XCD run
whole (batch, head) columns.  The first half checks the map itself through
flash_v3_block_map, which fills its table with the function the kernels
call: a bijection for every grid, balanced over the 8 labels, whole columns
at the flagship grid.  The second half runs the kernels at grids whose block
count is no multiple of 8 (or below it) and checks that every output element
is written, that the results match fp32 autograd, and that a head computes
bit for bit what it computes when it is launched alone: the arithmetic of a
block does not depend on where the block ran, so any difference there is a
mis-mapped pointer.  All tests require an MI355X."""
import functools
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
SCALE = 1.0 / math.sqrt(D)


@pytest.fixture(autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"


def _ext():
    from fengshen_amd.ops import get_ext
    return get_ext()


# ---- the map ---------------------------------------------------------------

GRIDS = [(1, 1, 1), (1, 3, 2), (2, 3, 2), (3, 5, 1), (5, 7, 3), (8, 1, 1),
         (8, 3, 1), (16, 2, 1), (8, 40, 2)]
ENDS = [True, False]


def _weight(x, nx, heavy_last):
    return x + 1 if heavy_last else nx - x


@pytest.mark.parametrize("heavy_last", ENDS, ids=["heavy_last", "heavy_first"])
@pytest.mark.parametrize("grid", GRIDS, ids=["x".join(map(str, g))
                                             for g in GRIDS])
def test_map_is_a_bijection(grid, heavy_last):
    nx, ny, nz = grid
    m = _ext().flash_v3_block_map(nx, ny, nz, heavy_last)
    assert m.dtype == torch.int32 and tuple(m.shape) == (nx * ny * nz, 3)
    got = sorted(map(tuple, m.tolist()))
    want = sorted((x, y, z) for x in range(nx) for y in range(ny)
                  for z in range(nz))
    assert got == want


@pytest.mark.parametrize("heavy_last", ENDS, ids=["heavy_last", "heavy_first"])
@pytest.mark.parametrize("grid", GRIDS, ids=["x".join(map(str, g))
                                             for g in GRIDS])
def test_labels_carry_equal_work_up_to_one_column(grid, heavy_last):
    nx, ny, nz = grid
    m = _ext().flash_v3_block_map(nx, ny, nz, heavy_last).tolist()
    work = [0] * 8
    for L, (x, _, _) in enumerate(m):
        work[L % 8] += _weight(x, nx, heavy_last)
    assert max(work) - min(work) <= nx * (nx + 1) // 2, work


@pytest.mark.parametrize("heavy_last", ENDS, ids=["heavy_last", "heavy_first"])
def test_flagship_grid_gives_each_label_ten_whole_columns(heavy_last):
    nx, ny, nz = 8, 40, 2
    m = _ext().flash_v3_block_map(nx, ny, nz, heavy_last).tolist()
    xs = list(range(nx - 1, -1, -1)) if heavy_last else list(range(nx))
    for label in range(8):
        mine = [tuple(m[L]) for L in range(label, nx * ny * nz, 8)]
        want = []
        for col in range(10 * label, 10 * label + 10):   # col = z * ny + y
            want += [(x, col % ny, col // ny) for x in xs]
        assert mine == want, f"label {label}"


# ---- the kernels at grids that are no multiple of 8 ------------------------
# name: (b, h, h_kv, s, packed documents)
CASES = {
    "b1_h5_s768": (1, 5, 5, 768, False),        # T = 15
    "b1_h3_s2048": (1, 3, 3, 2048, False),      # T = 24, nx = 8
    "b3_h1_s320": (3, 1, 1, 320, False),        # T = 6, last block part empty
    "gqa_b1_h4_kv2_s768": (1, 4, 2, 768, False),    # T = 12, dkv T = 6
    "packed_b2_h3_s768": (2, 3, 3, 768, True),      # T = 18
}
# first rows of the documents of each batch row of the packed case
_DOCS = [[0, 200, 300, 700], [0, 513]]


def _kstart(b, s):
    ks = torch.zeros(b, s, dtype=torch.int32)
    for bi in range(b):
        for st in _DOCS[bi]:
            ks[bi, st:] = st
    return ks.cuda()


def _launch(q, k, v, do, kstart):
    """Forward and backward through the strided entry points, every output
    pre-filled with NaN."""
    from fengshen_amd.ops.flash import kstart_qend
    ext = _ext()
    nan = float("nan")
    o = torch.full_like(q, nan)
    lse = ext.flash_attn_fwd_v3_strided(q, k, v, o, SCALE, True, None,
                                        kstart=kstart)
    dq, dk, dv = (torch.full_like(t, nan) for t in (q, k, v))
    qend = kstart_qend(kstart) if kstart is not None else None
    ext.flash_attn_bwd_v3_strided(q, k, v, o, do, lse, dq, dk, dv, SCALE,
                                  True, None, kstart=kstart, qend=qend)
    torch.cuda.synchronize()
    return {"o": o, "lse": lse, "dq": dq, "dk": dk, "dv": dv}


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs (CPU generator, fixed seed) and the kernels' results, computed
    once and shared by the tests of the case."""
    b, h, h_kv, s, packed = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(1234)

    def rnd(heads):
        return torch.randn(b, heads, s, D, generator=g).to(torch.bfloat16) \
            .cuda()
    q, do = rnd(h), rnd(h)
    k, v = rnd(h_kv), rnd(h_kv)
    kstart = _kstart(b, s) if packed else None
    return (q, k, v, do, kstart), _launch(q, k, v, do, kstart)


@pytest.mark.parametrize("name", list(CASES))
def test_every_output_element_is_written(name):
    _, res = _case(name)
    for n, t in res.items():
        assert not torch.isnan(t).any().item(), f"{n}: NaN left"
        assert torch.isfinite(t.float()).all().item(), f"{n}: not finite"


@pytest.mark.parametrize("name", list(CASES))
def test_matches_fp32_autograd(name):
    """3e-2 of the reference's range, the bound of
    test_d128_causal_s512_grads_match_fp32_oracle."""
    from fengshen_amd.ops.flash import kstart_to_mask
    (q, k, v, do, kstart), res = _case(name)
    b, h, h_kv, s, _ = CASES[name]
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ke = kf.repeat_interleave(h // h_kv, dim=1)
    ve = vf.repeat_interleave(h // h_kv, dim=1)
    scores = qf @ ke.transpose(-1, -2) * SCALE
    if kstart is not None:
        mask = kstart_to_mask(kstart)
    else:
        mask = torch.ones(s, s, device="cuda", dtype=torch.bool).triu(1)
    ref = torch.softmax(scores.masked_fill(mask, float("-inf")), -1) @ ve
    ref.backward(do.float())
    for n, r in (("o", ref.detach()), ("dq", qf.grad), ("dk", kf.grad),
                 ("dv", vf.grad)):
        err = (res[n].float() - r).abs().max() / r.abs().max().clamp(min=1.0)
        print(f"{name} {n}: rel err {err.item():.4g}")
        assert err.item() < 3e-2, f"{n}: rel err {err.item():.4g}"


@pytest.mark.parametrize("name", list(CASES))
def test_head_equals_the_same_head_launched_alone(name):
    """Bit for bit, O, LSE, dQ, dK and dV.  A grouped-query KV head is
    launched alone with the query heads of its group, which is what its
    dK / dV sum over."""
    (q, k, v, do, kstart), res = _case(name)
    b, h, h_kv, s, _ = CASES[name]
    G = h // h_kv
    for bi in range(b):
        ks1 = kstart[bi:bi + 1].contiguous() if kstart is not None else None
        for j in range(h_kv):
            qs_, kv_ = slice(G * j, G * j + G), slice(j, j + 1)
            alone = _launch(q[bi:bi + 1, qs_].contiguous(),
                            k[bi:bi + 1, kv_].contiguous(),
                            v[bi:bi + 1, kv_].contiguous(),
                            do[bi:bi + 1, qs_].contiguous(), ks1)
            for n, t in alone.items():
                sl = kv_ if n in ("dk", "dv") else qs_
                assert torch.equal(res[n][bi:bi + 1, sl], t), \
                    f"{n} of batch {bi}, kv head {j} depends on the grid"
