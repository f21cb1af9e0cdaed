"""Replay of tests/golden/attn_routes_parent.json on the GPU: every
F_ops.attention and ParallelAttention case of scripts/
gen_attn_route_golden.py must still reach the extension entry it reached
when the table was recorded, with the same klens / kstart presence, the same
K head count (grouped K/V expanded or not) and the same exception type, and
must not convert a mask more often (each conversion is a device-to-host
sync).  Requires an MI355X."""
import importlib.util
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ("entry", "klens", "kstart", "k_heads", "raises")
AT_MOST = ("mask_to_kstart", "mask_to_klens")


def load_gen():
    spec = importlib.util.spec_from_file_location(
        "gen_attn_route_golden",
        os.path.join(_ROOT, "scripts", "gen_attn_route_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_golden():
    with open(os.path.join(_ROOT, "tests", "golden",
                           "attn_routes_parent.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("kind", ["fn", "layer"])
def test_every_recorded_route_is_kept(kind):
    assert torch.cuda.is_available()
    from fengshen_amd.ops import has_ext
    assert has_ext(), "HIP extension missing on GPU box"
    gen, golden = load_gen(), load_golden()
    cases = {gen.case_id(c): c
             for c in (gen.fn_cases() if kind == "fn" else gen.layer_cases())}
    assert set(cases) == {i for i in golden if i.startswith(kind + "/")}
    bad = []
    for cid, c in cases.items():
        got, want = gen.run_case(c), golden[cid]
        if any(got[f] != want[f] for f in EXACT) \
                or any(got[f] > want[f] for f in AT_MOST):
            bad.append((cid, got, want))
    assert not bad, f"{len(bad)} of {len(cases)} routes changed: {bad[:5]}"
