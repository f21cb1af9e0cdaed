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


# Causal cases with a per-row key start and / or grouped KV heads, each run
# contiguous and strided.  A table of its own with its own seed base:
# make_inputs seeds CASES by sorted position, so a new name there would move
# the inputs of every recorded case.
# name -> (d, s, h, h_kv, kstart)
MASKED_CASES = {
    "d128_causal_s320_kstart": (128, 320, H, H, True),
    "d64_causal_s128_gqa": (64, 128, 4, 2, False),
    "d96_causal_s320_gqa_kstart": (96, 320, 4, 1, True),
}


def variants():
    """(case name, strided) pairs, smallest d128 case first."""
    for name, c in CASES.items():
        yield name, False
        if c[6]:
            yield name, True
    for name in MASKED_CASES:
        yield name, False
        yield name, True


def key(name, strided):
    return f"{name}/{'strided' if strided else 'contig'}"


def make_inputs(name):
    """q, k, v, dO as bf16 CPU tensors, fixed per case: q and dO
    [B, h, s, d], k and v [B, h_kv, s, d] (h = h_kv = H in CASES)."""
    if name in CASES:
        (d, s), h, h_kv = CASES[name][:2], H, H
        seed = 1000 + sorted(CASES).index(name)
    else:
        d, s, h, h_kv, _ = MASKED_CASES[name]
        seed = 2000 + sorted(MASKED_CASES).index(name)
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [torch.randn(B, n, s, d, generator=g, dtype=torch.float32)
            .to(torch.bfloat16) for n in (h, h_kv, h_kv, h)]


def make_kstart(s):
    """int32 [B, s]: row 0 is packed documents starting at 0, 70 and 200,
    row 1 is left-padded by 37 (a pad row sees only itself)."""
    ar = torch.arange(s, dtype=torch.int32)
    docs = 70 * (ar >= 70) + 130 * (ar >= 200)
    return torch.stack([docs.to(torch.int32), torch.where(ar < 37, ar, 37)])


def _bhsd(x, h=H):
    """[b, s, h*d] -> [b, h, s, d] view."""
    return x.unflatten(2, (h, -1)).transpose(1, 2)


def _wide(width, s, fill=None):
    """[B, s, width] slice of a wider allocation (row stride width + 24,
    base offset 8 elements); returns (allocation, slice)."""
    full = torch.full((B, s, width + 24), float("nan") if fill is None
                      else fill, device="cuda", dtype=torch.bfloat16)
    return full, full[:, :, 8:8 + width]


def run_case(ext, name, strided):
    """Run forward + backward; returns {o, lse, dq, dk, dv} on the GPU:
    o, dq [B, h, s, d], dk, dv [B, h_kv, s, d], lse [B, h, s] (views for
    the strided entry)."""
    if name in CASES:
        d, s, causal, klens, drop_p, drop_seed, _ = CASES[name]
        h, h_kv, masked = H, H, False
    else:
        d, s, h, h_kv, masked = MASKED_CASES[name]
        causal, klens, drop_p, drop_seed = True, None, 0.0, 0
    scale = 1.0 / math.sqrt(d)
    q, k, v, do = [t.cuda() for t in make_inputs(name)]
    kl = None if klens is None else torch.tensor(
        klens, device="cuda", dtype=torch.int32)
    ks = qe = None
    if masked:
        from fengshen_amd.ops.flash import kstart_qend
        ks = make_kstart(s).cuda()
        qe = kstart_qend(ks)
    if not strided:
        o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, causal, kl, drop_p,
                                       drop_seed, kstart=ks)
        dq, dk, dv = ext.flash_attn_bwd_v3(q, k, v, o, do, lse, scale,
                                           causal, kl, drop_p, drop_seed,
                                           kstart=ks, qend=qe)
        torch.cuda.synchronize()
        return dict(zip(NAMES, (o, lse, dq, dk, dv)))

    w, wkv = h * d, h_kv * d

    def parts(x):  # [q | k | v] thirds of a packed [B, s, w + 2*wkv] slice
        return (_bhsd(x.narrow(2, 0, w), h),
                _bhsd(x.narrow(2, w, wkv), h_kv),
                _bhsd(x.narrow(2, w + wkv, wkv), h_kv))

    _, qkv = _wide(w + 2 * wkv, s, fill=0.0)
    qv, kv, vv = parts(qkv)
    qv.copy_(q), kv.copy_(k), vv.copy_(v)
    _, do_p = _wide(w, s, fill=0.0)
    _bhsd(do_p, h).copy_(do)
    o_full, o_p = _wide(w, s)
    g_full, g_p = _wide(w + 2 * wkv, s)
    lse = ext.flash_attn_fwd_v3_strided(qv, kv, vv, _bhsd(o_p, h), scale,
                                        causal, kl, kstart=ks)
    dq, dk, dv = parts(g_p)
    ext.flash_attn_bwd_v3_strided(qv, kv, vv, _bhsd(o_p, h), _bhsd(do_p, h),
                                  lse, dq, dk, dv, scale, causal, kl,
                                  kstart=ks, qend=qe)
    torch.cuda.synchronize()
    for full, width in ((o_full, w), (g_full, w + 2 * wkv)):  # slice only
        assert full[:, :, :8].isnan().all(), "wrote in front of the slice"
        assert full[:, :, 8 + width:].isnan().all(), "wrote past the slice"
    return dict(zip(NAMES, (_bhsd(o_p, h), lse, dq, dk, dv)))


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
