"""Flash v3 kernels compute bit for bit what the recorded build computed.

tests/golden/flash_v3_parent.json holds SHA-256 digests of O, LSE, dQ, dK
and dV, written by scripts/gen_flash_v3_golden.py on an MI355X with the
build before the kernels moved to one LDS image per tile and transposed LDS
reads.  Inputs come from a CPU generator with a fixed seed.  A change to the
kernels that only moves operands (layouts, staging, tile skipping) must
leave every digest alone; one that reorders a sum will not.  The fp32-oracle
test at the end keeps a wrong golden file from passing unnoticed.  All tests
require an MI355X."""
import importlib.util
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")


def _load_gen():
    spec = importlib.util.spec_from_file_location(
        "gen_flash_v3_golden",
        os.path.join(_ROOT, "scripts", "gen_flash_v3_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


gen = _load_gen()

with open(os.path.join(_ROOT, "tests", "golden", "flash_v3_parent.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(autouse=True)
def _require_ext():
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"


def test_golden_covers_every_case():
    assert sorted(GOLDEN) == sorted(gen.key(n, s) for n, s in gen.variants())


@pytest.mark.parametrize("name,strided", list(gen.variants()),
                         ids=[gen.key(n, s) for n, s in gen.variants()])
def test_bit_identical_to_recorded_build(name, strided):
    from fengshen_amd.ops import get_ext
    res = gen.run_case(get_ext(), name, strided)
    want = GOLDEN[gen.key(name, strided)]
    bad = [n for n in gen.NAMES if gen.digest(res[n]) != want[n]]
    assert not bad, f"{gen.key(name, strided)}: {bad} differ from the record"


def test_d128_causal_s512_grads_match_fp32_oracle():
    """Same inputs as the golden case, against fp32 autograd (tolerance of
    test_flash_bwd_v3_matches_oracle: 3e-2 of the reference's range)."""
    from fengshen_amd.ops import get_ext
    name = "d128_causal_s512"
    res = gen.run_case(get_ext(), name, False)
    q, k, v, do = [t.cuda().float() for t in gen.make_inputs(name)]
    q.requires_grad_(True), k.requires_grad_(True), v.requires_grad_(True)
    s, d = q.shape[-2], q.shape[-1]
    scores = q @ k.transpose(-1, -2) * (1.0 / math.sqrt(d))
    cm = torch.ones(s, s, device="cuda", dtype=torch.bool).triu(1)
    ref = torch.softmax(scores.masked_fill(cm, float("-inf")), -1) @ v
    ref.backward(do)
    for n, r in (("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        err = (res[n].float() - r).abs().max() / r.abs().max().clamp(min=1.0)
        assert err.item() < 3e-2, f"{n}: rel err {err.item():.4g}"
