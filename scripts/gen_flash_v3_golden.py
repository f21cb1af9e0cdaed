"""Record SHA-256 digests of the flash v3 kernels' outputs.

    python scripts/gen_flash_v3_golden.py [out.json]

Run once on an MI355X with the build whose results are to be frozen; the
digests go to tests/golden/flash_v3_parent.json, and
tests/test_flash_v3_bitexact_gpu.py compares later builds with them.  Inputs
come from a CPU generator with a fixed seed, so the GPU RNG plays no part.
Only extension entry points are called; `run_case` is shared with the test.
"""
import hashlib
import json
import math
import os
import sys

import torch

B, H = 2, 3
NAMES = ("o", "lse", "dq", "dk", "dv")

# name -> (d, s, causal, klens, dropout_p, drop_seed, also_strided)
CASES = {
    "d128_causal_s64": (128, 64, True, None, 0.0, 0, True),
    "d128_causal_s320": (128, 320, True, None, 0.0, 0, True),
    "d128_causal_s512": (128, 512, True, None, 0.0, 0, True),
    "d128_full_s256": (128, 256, False, None, 0.0, 0, True),
    "d96_causal_s128": (96, 128, True, None, 0.0, 0, False),
    "d64_full_s128_klens": (64, 128, False, [128, 70], 0.0, 0, False),
    "d64_causal_s128_drop": (64, 128, True, None, 0.1, 1234, False),
}


def variants():
    """(case name, strided) pairs, smallest d128 case first."""
    for name, c in CASES.items():
        yield name, False
        if c[6]:
            yield name, True


def key(name, strided):
    return f"{name}/{'strided' if strided else 'contig'}"


def make_inputs(name):
    """q, k, v, dO as [B, H, s, d] bf16 CPU tensors, fixed per case."""
    d, s = CASES[name][:2]
    g = torch.Generator(device="cpu").manual_seed(
        1000 + sorted(CASES).index(name))
    return [torch.randn(B, H, s, d, generator=g, dtype=torch.float32)
            .to(torch.bfloat16) for _ in range(4)]


def _bhsd(x):
    """[b, s, H*d] -> [b, H, s, d] view."""
    return x.unflatten(2, (H, -1)).transpose(1, 2)


def _wide(width, s, fill=None):
    """[B, s, width] slice of a wider allocation (row stride width + 24,
    base offset 8 elements); returns (allocation, slice)."""
    full = torch.full((B, s, width + 24), float("nan") if fill is None
                      else fill, device="cuda", dtype=torch.bfloat16)
    return full, full[:, :, 8:8 + width]


def run_case(ext, name, strided):
    """Run forward + backward; returns {o, lse, dq, dk, dv} on the GPU,
    each [B, H, s, ...] (views for the strided entry)."""
    d, s, causal, klens, drop_p, drop_seed, _ = CASES[name]
    scale = 1.0 / math.sqrt(d)
    q, k, v, do = [t.cuda() for t in make_inputs(name)]
    kl = None if klens is None else torch.tensor(
        klens, device="cuda", dtype=torch.int32)
    if not strided:
        o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, causal, kl, drop_p,
                                       drop_seed)
        dq, dk, dv = ext.flash_attn_bwd_v3(q, k, v, o, do, lse, scale,
                                           causal, kl, drop_p, drop_seed)
        torch.cuda.synchronize()
        return dict(zip(NAMES, (o, lse, dq, dk, dv)))

    w = H * d
    _, qkv = _wide(3 * w, s, fill=0.0)
    qv, kv, vv = [_bhsd(qkv.narrow(2, i * w, w)) for i in range(3)]
    qv.copy_(q), kv.copy_(k), vv.copy_(v)
    _, do_p = _wide(w, s, fill=0.0)
    _bhsd(do_p).copy_(do)
    o_full, o_p = _wide(w, s)
    g_full, g_p = _wide(3 * w, s)
    lse = ext.flash_attn_fwd_v3_strided(qv, kv, vv, _bhsd(o_p), scale,
                                        causal, kl)
    dq, dk, dv = [_bhsd(g_p.narrow(2, i * w, w)) for i in range(3)]
    ext.flash_attn_bwd_v3_strided(qv, kv, vv, _bhsd(o_p), _bhsd(do_p), lse,
                                  dq, dk, dv, scale, causal, kl)
    torch.cuda.synchronize()
    for full, width in ((o_full, w), (g_full, 3 * w)):  # slice only
        assert full[:, :, :8].isnan().all(), "wrote in front of the slice"
        assert full[:, :, 8 + width:].isnan().all(), "wrote past the slice"
    return dict(zip(NAMES, (_bhsd(o_p), lse, dq, dk, dv)))


def digest(t):
    t = t.contiguous().cpu()
    raw = t.view(torch.int16) if t.dtype == torch.bfloat16 else t
    return hashlib.sha256(raw.numpy().tobytes()).hexdigest()


def main():
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    out = {}
    for name, strided in variants():
        res = run_case(ext, name, strided)
        for n in NAMES:
            assert not res[n].float().isnan().any(), (name, strided, n)
        out[key(name, strided)] = {n: digest(res[n]) for n in NAMES}
        print(key(name, strided), out[key(name, strided)]["o"][:16])
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(
        os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
        "flash_v3_parent.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(
        os.path.abspath(__file__)), ".."))
    main()
