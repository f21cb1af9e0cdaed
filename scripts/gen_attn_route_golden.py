"""Record which attention kernel every call shape is routed to.

    python scripts/gen_attn_route_golden.py [out.json]

Run once on an MI355X with the build whose routing is to be frozen; the
table goes to tests/golden/attn_routes_parent.json.  tests/
test_attn_route_gpu.py replays it through F_ops.attention and a tiny
ParallelAttention with the spies below, and tests/test_attn_route_cpu.py
checks ops.flash.route_attention against its F_ops.attention entries
without a GPU.  `fn_cases`, `layer_cases`, `make_mask`, `make_kstart` and
`run_case` are shared with the tests.

Per case the record holds: the extension entry that ran (or "bmm"), whether
it got klens / kstart, the K head count it saw (grouped K/V expanded or
not), how often mask_to_kstart / mask_to_klens ran (each is a device-to-host
sync) and the type of a Python-side exception.  No case reaches a kernel
with arguments it does not cover: every refusal is a host-side check.
"""
import contextlib
import json
import os
import sys

import torch

H = 2
ENTRIES = ("flash_attn_fwd", "flash_attn_fwd_v3", "flash_attn_fwd_v3_strided")
MASKS = ("none", "rpad4", "rpad2", "lpad", "hole", "docs", "dense")
SWITCHES = ("FENGSHEN_PACKED_ATTN", "FENGSHEN_VARLEN_FLASH",
            "FENGSHEN_GQA_FLASH", "FENGSHEN_FLASH_V3_DROP")
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _case(kind, **kw):
    c = dict(kind=kind, b=2, h=H, h_kv=H, d=64, sq=64, sk=64, dtype="bf16",
             causal=True, mask="none", kstart="none", drop=0.0,
             training=False, env={})
    if kind == "layer":
        # cache: "none", "empty" or "past" (64 tokens already in it)
        c.update(cache="none")
        del c["sk"], c["dtype"]
    c.update(kw)
    return c


def case_id(c):
    parts = [c["kind"], "c" if c["causal"] else "f",
             f"h{c['h']}kv{c['h_kv']}", f"d{c['d']}", f"b{c['b']}",
             f"s{c['sq']}" + (f"x{c['sk']}" if "sk" in c else ""),
             c.get("dtype", c.get("cache")), f"m-{c['mask']}",
             f"ks-{c['kstart']}",
             f"p{c['drop']}{'t' if c['training'] else 'e'}"]
    parts += [f"{k[9:]}={v}" for k, v in sorted(c["env"].items())]
    return "/".join(parts)


def fn_cases():
    """The F_ops.attention cases."""
    out = []

    def add(**kw):
        out.append(_case("fn", **kw))

    varlen0, gqa0 = {"FENGSHEN_VARLEN_FLASH": "0"}, {"FENGSHEN_GQA_FLASH": "0"}
    v3drop = {"FENGSHEN_FLASH_V3_DROP": "1"}
    for causal in (True, False):
        for h_kv in (2, 1):
            # every mask form at a v3 and at a general-kernel head dim
            for d in (64, 80):
                for mask in MASKS:
                    add(causal=causal, h_kv=h_kv, d=d, mask=mask)
            for d in (128, 48):
                for mask in ("none", "rpad4", "dense"):
                    add(causal=causal, h_kv=h_kv, d=d, mask=mask)
            # shapes: tile multiples, below a tile, cross and chunked
            for sq, sk in ((128, 128), (48, 48), (16, 16), (16, 77),
                           (32, 128), (1, 65)):
                for mask in ("none", "rpad4"):
                    add(causal=causal, h_kv=h_kv, sq=sq, sk=sk, mask=mask)
            add(causal=causal, h_kv=h_kv, b=1, sq=128, sk=128, mask="docs")
            for mask in ("none", "rpad4"):
                add(causal=causal, h_kv=h_kv, dtype="fp16", mask=mask)
                # dropout: active, and switched off by eval
                for d in (64, 128):
                    for training in (True, False):
                        add(causal=causal, h_kv=h_kv, d=d, mask=mask,
                            drop=0.1, training=training)
                    add(causal=causal, h_kv=h_kv, d=d, mask=mask, drop=0.1,
                        training=True, env=v3drop)
                add(causal=causal, h_kv=h_kv, d=80, mask=mask, drop=0.1,
                    training=True)
    # one KV head shared by both query heads' halves: h_kv = h/2 with h = 4
    for mask in ("none", "lpad", "dense"):
        add(h=4, h_kv=2, mask=mask)
        add(h=4, h_kv=2, mask=mask, causal=False)
    # a caller's kstart: alone, or next to the mask it stands for, or next
    # to one it does not stand for (the mask is not inspected)
    for h_kv in (2, 1):
        for ks, mask in (("alone", "none"), ("with", "lpad"),
                         ("with", "dense")):
            for d in (64, 128, 80):
                add(h_kv=h_kv, d=d, kstart=ks, mask=mask)
            add(h_kv=h_kv, sq=128, sk=128, kstart=ks, mask=mask)
            add(h_kv=h_kv, sq=48, sk=48, kstart=ks, mask=mask)
            add(h_kv=h_kv, dtype="fp16", kstart=ks, mask=mask)
            add(h_kv=h_kv, kstart=ks, mask=mask, drop=0.1, training=True)
            add(h_kv=h_kv, kstart=ks, mask=mask, drop=0.1, training=False)
            add(h_kv=h_kv, kstart=ks, mask=mask, env=varlen0)
            add(h_kv=h_kv, kstart=ks, mask=mask, env=gqa0)
        # refused: kstart describes causal self-attention
        add(h_kv=h_kv, kstart="alone", causal=False)
        add(h_kv=h_kv, kstart="alone", sq=32, sk=128)
        add(h_kv=h_kv, kstart="with", mask="rpad4", causal=False)
    # the switches, on every kind of case each can affect
    for h_kv in (2, 1):
        for mask in ("rpad4", "rpad2", "lpad", "hole", "docs", "dense"):
            add(h_kv=h_kv, mask=mask, env=varlen0)
        add(h_kv=h_kv, mask="rpad4", causal=False, env=varlen0)
    for mask in MASKS:
        add(h_kv=1, mask=mask, env=gqa0)
    add(h_kv=1, causal=False, env=gqa0)
    add(h_kv=1, d=80, env=gqa0)
    add(h_kv=1, drop=0.1, training=True, env=gqa0)
    add(h=4, h_kv=2, env=gqa0)
    add(h_kv=1, mask="lpad", env={**gqa0, **varlen0})
    for causal in (True, False):
        add(d=96, causal=causal, drop=0.1, training=True, env=v3drop)
    add(drop=0.1, training=False, env=v3drop)
    # query heads that are no multiple of the KV heads
    add(h=3, h_kv=2)
    add(h=3, h_kv=2, causal=False)
    add(h=3, h_kv=2, kstart="alone", causal=False)
    return out


def layer_cases():
    """The ParallelAttention cases (hidden size h*d, bf16, rotary)."""
    out = []

    def add(**kw):
        out.append(_case("layer", **kw))

    packed0 = {"FENGSHEN_PACKED_ATTN": "0"}
    varlen0, gqa0 = {"FENGSHEN_VARLEN_FLASH": "0"}, {"FENGSHEN_GQA_FLASH": "0"}
    for causal in (True, False):
        for h_kv in (2, 1):
            for mask in MASKS:
                add(causal=causal, h_kv=h_kv, mask=mask)
                add(causal=causal, h_kv=h_kv, mask=mask, env=packed0)
            for mask in ("none", "rpad4", "dense"):
                for d in (128, 80):
                    add(causal=causal, h_kv=h_kv, d=d, mask=mask)
                add(causal=causal, h_kv=h_kv, sq=48, mask=mask)
                add(causal=causal, h_kv=h_kv, sq=128, mask=mask)
                # a cache object keeps the layer off the packed path
                add(causal=causal, h_kv=h_kv, mask=mask, cache="empty")
                # attention dropout: active in training only
                for training in (True, False):
                    add(causal=causal, h_kv=h_kv, mask=mask, drop=0.1,
                        training=training)
            add(causal=causal, h_kv=h_kv, training=True)
            add(causal=causal, h_kv=h_kv, mask="rpad4", env=varlen0)
            add(causal=causal, h_kv=h_kv, mask="rpad4", env=gqa0)
            add(causal=causal, h_kv=h_kv, env=gqa0)
            add(causal=causal, h_kv=h_kv, drop=0.1, training=True,
                env={"FENGSHEN_FLASH_V3_DROP": "1"})
            # chunked prefill and single-token decode behind 64 cached tokens
            for sq in (64, 1):
                for mask in ("none", "rpad4"):
                    add(causal=causal, h_kv=h_kv, sq=sq, mask=mask,
                        cache="past")
    for h_kv in (2, 1):
        for ks, mask in (("alone", "none"), ("with", "lpad"),
                         ("with", "dense")):
            add(h_kv=h_kv, kstart=ks, mask=mask)
            add(h_kv=h_kv, kstart=ks, mask=mask, d=80)
            add(h_kv=h_kv, kstart=ks, mask=mask, cache="empty")
            add(h_kv=h_kv, kstart=ks, mask=mask, env=packed0)
            add(h_kv=h_kv, kstart=ks, mask=mask, env=varlen0)
            add(h_kv=h_kv, kstart=ks, mask=mask, env=gqa0)
            add(h_kv=h_kv, kstart=ks, mask=mask, drop=0.1, training=True)
        # refused: non-empty cache, bidirectional layer
        add(h_kv=h_kv, kstart="alone", cache="past")
        add(h_kv=h_kv, kstart="alone", causal=False)
        add(h_kv=h_kv, kstart="alone", causal=False, env=packed0)
    add(h=4, h_kv=2, mask="lpad")
    add(h=4, h_kv=2, mask="hole")
    return out


def make_mask(name, b, sq, sk, device):
    """True = masked.  Batch row 0 carries the pattern; further rows are
    unpadded where the form allows."""
    if name == "none":
        return None
    ar = torch.arange(sk, device=device)
    if name in ("rpad4", "rpad2", "lpad", "hole"):
        row = {"rpad4": ar >= sk - 5, "rpad2": ar >= sk - 5, "lpad": ar < 5,
               "hole": (ar == 3) | (ar >= sk - 5)}[name]
        m = torch.zeros(b, sk, dtype=torch.bool, device=device)
        m[0] = row
        return m if name == "rpad2" else m[:, None, None, :]
    i = torch.arange(sq, device=device).view(1, sq, 1) + (sk - sq)
    j = ar.view(1, 1, sk)
    if name == "docs":
        # packed documents: a second one starts at key sk // 2 + 3
        start = torch.where(i >= sk // 2 + 3, sk // 2 + 3, 0)
        return ((j > i) | (j < start)).expand(b, sq, sk)[:, None].contiguous()
    assert name == "dense"
    return (((i + 2 * j) % 7 == 0) & (j != i)).expand(b, sq, sk)[:, None] \
        .contiguous()


def make_kstart(b, s, device):
    """int32 [b, s], the key start of the "lpad" mask: row 0 is left-padded
    by 5 (a pad row sees only itself), the others are unpadded."""
    ar = torch.arange(s, dtype=torch.int32, device=device)
    ks = torch.zeros(b, s, dtype=torch.int32, device=device)
    ks[0] = torch.where(ar < 5, ar, 5)
    return ks


class _Cache:
    """The smallest KV cache the layer accepts."""

    def __init__(self, k=None, v=None):
        self.k, self.v = k, v

    def get_seq_length(self, layer_idx):
        return 0 if self.k is None else self.k.shape[-2]

    def update(self, k, v, layer_idx):
        if self.k is not None:
            k, v = torch.cat([self.k, k], 2), torch.cat([self.v, v], 2)
        self.k, self.v = k, v
        return k, v


@contextlib.contextmanager
def _environ(env):
    old = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@contextlib.contextmanager
def spies():
    """Call-through spies on the three forward entries and counters on the
    two mask conversions; yields (entries seen, conversion counts)."""
    from fengshen_amd.ops import flash, get_ext
    ext = get_ext()
    seen, counts = [], {"mask_to_kstart": 0, "mask_to_klens": 0}
    saved = [(ext, n, getattr(ext, n)) for n in ENTRIES] \
        + [(flash, n, getattr(flash, n)) for n in counts]

    def entry_spy(name, orig):
        klens_at = 6 if name.endswith("strided") else 5

        def spy(*a, **kw):
            seen.append({"entry": name, "klens": a[klens_at] is not None,
                         "kstart": kw.get("kstart") is not None,
                         "k_heads": a[1].shape[1]})
            return orig(*a, **kw)
        return spy

    def counter(name, orig):
        def counted(*a, **kw):
            counts[name] += 1
            return orig(*a, **kw)
        return counted

    try:
        for obj, name, orig in saved:
            setattr(obj, name, (entry_spy if obj is ext else counter)(
                name, orig))
        yield seen, counts
    finally:
        for obj, name, orig in saved:
            setattr(obj, name, orig)


def _call_fn(c, dev):
    from fengshen_amd.ops import functional as F_ops
    g = torch.Generator(device="cpu").manual_seed(1)
    q, k, v = [torch.randn(c["b"], n, s, c["d"], generator=g)
               .to(DTYPES[c["dtype"]]).to(dev)
               for n, s in ((c["h"], c["sq"]), (c["h_kv"], c["sk"]),
                            (c["h_kv"], c["sk"]))]
    mask = make_mask(c["mask"], c["b"], c["sq"], c["sk"], dev)
    ks = None if c["kstart"] == "none" else \
        make_kstart(c["b"], c["sq"], dev)
    F_ops.attention(q, k, v, causal=c["causal"], mask=mask,
                    dropout_p=c["drop"], training=c["training"], kstart=ks)


def _call_layer(c, dev):
    from fengshen_amd.models.layers import ParallelAttention
    b, h, h_kv, d, sq = c["b"], c["h"], c["h_kv"], c["d"], c["sq"]
    torch.manual_seed(3)
    layer = ParallelAttention(
        h * d, h, causal=c["causal"], rotary=True, max_positions=256,
        attention_dropout=c["drop"], bias=False, dtype=torch.bfloat16,
        num_kv_heads=h_kv).to(dev).train(c["training"])
    g = torch.Generator(device="cpu").manual_seed(2)
    x = torch.randn(b, sq, h * d, generator=g).to(torch.bfloat16).to(dev)
    cache, past = None, 0
    if c["cache"] == "past":
        past = 64
        cache = _Cache(*[torch.randn(b, h_kv, past, d, generator=g)
                         .to(torch.bfloat16).to(dev) for _ in range(2)])
    elif c["cache"] == "empty":
        cache = _Cache()
    mask = make_mask(c["mask"], b, sq, past + sq, dev)
    ks = None if c["kstart"] == "none" else make_kstart(b, sq, dev)
    layer(x, attention_mask=mask, cache=cache, kstart=ks)


def run_case(c, dev="cuda"):
    """Run one case under the spies; returns its record.  (On "cpu" every
    case is the eager bmm path: a rehearsal of the case list only.)"""
    rec = {"entry": "bmm", "klens": False, "kstart": False, "k_heads": None,
           "mask_to_kstart": 0, "mask_to_klens": 0, "raises": None}
    with _environ(c["env"]), spies() as (seen, counts), torch.no_grad():
        try:
            (_call_fn if c["kind"] == "fn" else _call_layer)(c, dev)
        except Exception as e:  # the type is the record
            if "HIP error" in str(e) or "illegal memory" in str(e):
                raise  # a device error is no refusal: stop here
            rec["raises"] = type(e).__name__
            rec["entry"] = None
        if dev == "cuda":
            torch.cuda.synchronize()
    assert len(seen) <= 1, (case_id(c), seen)
    if seen:
        rec.update(seen[0])
    rec.update(counts)
    return rec


def main():
    out = {}
    for c in fn_cases() + layer_cases():
        cid = case_id(c)
        assert cid not in out, cid
        out[cid] = r = run_case(c)
        print(cid, r["entry"], r["raises"] or "")
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
        "attn_routes_parent.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote", path, len(out), "cases")


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(
        os.path.abspath(__file__)), ".."))
    main()
