"""ops.flash.route_attention against the route table recorded on the GPU
(tests/golden/attn_routes_parent.json, scripts/gen_attn_route_golden.py):
the routing is host logic over shapes, dtypes, switches and a mask, so the
F_ops.attention cases of the table are checked here with CPU tensors."""
import pytest
import torch

from test_attn_route_gpu import load_gen, load_golden

GEN, GOLDEN = load_gen(), load_golden()
FN_CASES = {GEN.case_id(c): c for c in GEN.fn_cases()}
PATH = {"flash_attn_fwd": "flash", "flash_attn_fwd_v3": "flash", "bmm": "bmm"}


def _route(c, on_gpu, monkeypatch):
    """What F_ops.attention does with the case up to the kernel call: ask
    for the route, expand K/V if it says so.  Returns (route, conversion
    counts)."""
    from fengshen_amd.ops import flash
    for name in GEN.SWITCHES:
        monkeypatch.delenv(name, raising=False)
    for name, value in c["env"].items():
        monkeypatch.setenv(name, value)
    counts = {"mask_to_kstart": 0, "mask_to_klens": 0}
    for name in counts:
        def counted(*a, _name=name, _orig=getattr(flash, name)):
            counts[_name] += 1
            return _orig(*a)
        monkeypatch.setattr(flash, name, counted)
    mask = GEN.make_mask(c["mask"], c["b"], c["sq"], c["sk"], "cpu")
    ks = None if c["kstart"] == "none" else \
        GEN.make_kstart(c["b"], c["sq"], "cpu")
    route = flash.route_attention(
        on_gpu=on_gpu, dtype=GEN.DTYPES[c["dtype"]], heads=c["h"],
        kv_heads=c["h_kv"], sq=c["sq"], sk=c["sk"], head_dim=c["d"],
        causal=c["causal"], mask=mask, kstart=ks,
        dropout_p=c["drop"] if c["training"] else 0.0)
    if route.expand_kv:
        flash.expand_kv(torch.empty(1, c["h_kv"], 1, 1), c["h"])
    return route, counts


def test_golden_lists_exactly_the_scripts_cases():
    assert set(FN_CASES) == {i for i in GOLDEN if i.startswith("fn/")}


@pytest.mark.parametrize("cid", sorted(FN_CASES))
def test_route_matches_recorded(cid, monkeypatch):
    c, want = FN_CASES[cid], GOLDEN[cid]
    if want["raises"] in ("ValueError",):
        with pytest.raises(ValueError):
            _route(c, True, monkeypatch)
        return
    route, counts = _route(c, True, monkeypatch)
    if want["raises"] is not None:
        # refused by the softmax binding or by broadcasting, inside the bmm
        # body: no flash entry had run
        assert want["raises"] == "RuntimeError" and want["entry"] is None
        assert route.path == "bmm"
    else:
        assert route.path == PATH[want["entry"]]
    assert (route.klens is not None) == want["klens"]
    assert (route.kstart is not None) == want["kstart"]
    grouped = c["h_kv"] != c["h"]
    if route.path == "flash":
        assert route.expand_kv == (grouped and want["k_heads"] == c["h"])
        assert route.mask is None
    else:  # the bmm body has no grouped form
        assert route.expand_kv == grouped
        assert (route.mask is None) == (c["mask"] == "none"
                                        and c["kstart"] == "none")
    for name, n in counts.items():
        assert n <= want[name], name


@pytest.mark.parametrize("cid", sorted(FN_CASES))
def test_without_the_gpu_everything_is_bmm(cid, monkeypatch):
    c, want = FN_CASES[cid], GOLDEN[cid]
    if want["raises"] == "ValueError":
        with pytest.raises(ValueError):
            _route(c, False, monkeypatch)
        return
    route, counts = _route(c, False, monkeypatch)
    assert route.path == "bmm" and route.klens is None \
        and route.kstart is None
    assert counts == {"mask_to_kstart": 0, "mask_to_klens": 0}


def test_given_kstart_is_handed_on_and_dense_only_on_bmm():
    from fengshen_amd.ops import flash
    ks = GEN.make_kstart(2, 64, "cpu")
    kw = dict(on_gpu=True, dtype=torch.bfloat16, heads=2, kv_heads=2, sq=64,
              sk=64, causal=True, kstart=ks)
    assert flash.route_attention(head_dim=64, **kw).kstart is ks
    r = flash.route_attention(head_dim=80, **kw)
    assert r.path == "bmm" and torch.equal(r.mask, flash.kstart_to_mask(ks))
    # next to a mask, the bmm path keeps the caller's mask
    m = GEN.make_mask("lpad", 2, 64, 64, "cpu")
    assert flash.route_attention(head_dim=80, mask=m, **kw).mask is m


@pytest.mark.parametrize("packed_ok", [True, False])
def test_packed_needs_the_buffer_and_the_switch(packed_ok, monkeypatch):
    from fengshen_amd.ops import flash
    monkeypatch.delenv("FENGSHEN_PACKED_ATTN", raising=False)
    kw = dict(on_gpu=True, dtype=torch.bfloat16, heads=2, kv_heads=1, sq=64,
              sk=64, head_dim=64, causal=True, packed_ok=packed_ok)
    r = flash.route_attention(**kw)
    assert r.path == ("packed" if packed_ok else "flash") and not r.expand_kv
    monkeypatch.setenv("FENGSHEN_PACKED_ATTN", "0")
    assert flash.route_attention(**kw).path == "flash"
    monkeypatch.delenv("FENGSHEN_PACKED_ATTN")
    # grouped-query layouts are causal only; dropout is not packed
    assert flash.route_attention(**{**kw, "causal": False}).path == "flash"
    assert flash.route_attention(dropout_p=0.1, **kw).path == "flash"
