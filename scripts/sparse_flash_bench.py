"""Block-sparse flash attention benchmark.

For each (layout, block, seq_len) times forward and forward+backward of
  kernel : SparseSelfAttention on the block-sparse flash kernels
  eager  : the same module with FENGSHEN_SPARSE_FLASH=0 (blockwise eager)
  dense  : dense causal flash attention on the same tensors
The three variants alternate inside every repeat, in one process, after a
warm-up; times come from device events.  Prints one JSON line per point
with the median and the min..max spread over the repeats, the layout
density, and the achieved FLOP/s of the kernel path counted over active
16x16 sub-tiles only.

Usage: python scripts/sparse_flash_bench.py [--quick] [--out FILE]
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, json, math, statistics
import torch
from fengshen_amd.ops.flash import flash_attention
from fengshen_amd.ops.sparse_attention import (
    BigBirdSparsityConfig, LocalSlidingWindowSparsityConfig,
    SparseSelfAttention)

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="s=4096 only, 2 repeats")
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-eager", action="store_true")
args = ap.parse_args()

b, h, d = 2, 16, 128
scale = 1 / math.sqrt(d)
seqs = (4096,) if args.quick else (4096, 8192)
repeats = 2 if args.quick else args.repeats


def make_cfg(name, block):
    if name == "bigbird":
        return BigBirdSparsityConfig(h, block=block)
    return LocalSlidingWindowSparsityConfig(h, block=block)


def popcount_active(lists):
    m = lists.row_mask.cpu().to(torch.int64) & 0xFFFFFFFF
    n = 0
    for bit in range(32):
        n += int(((m >> bit) & 1).sum())
    return n * (h if lists.list_heads == 1 else 1)


def timed(fn, inner):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def run_point(name, block, s):
    cfg = make_cfg(name, block)
    attn = SparseSelfAttention(cfg)
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, gy = (torch.randn(b, h, s, d, generator=g, device="cuda")
                   .to(torch.bfloat16) for _ in range(4))
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    lists = attn.tile_lists(s, q.device)
    density = attn.density(s)
    sub_tiles = popcount_active(lists)
    fwd_flops = 2 * 2 * b * sub_tiles * 16 * 16 * d

    def env(val):
        if val is None:
            os.environ.pop("FENGSHEN_SPARSE_FLASH", None)
        else:
            os.environ["FENGSHEN_SPARSE_FLASH"] = val

    def kernel_fwd():
        env(None)
        with torch.no_grad():
            return attn(q, k, v)

    def eager_fwd():
        env("0")
        with torch.no_grad():
            out = attn(q, k, v)
        env(None)
        return out

    def dense_fwd():
        with torch.no_grad():
            return flash_attention(q, k, v, scale)

    def fb(fn):
        def run():
            for t in (qg, kg, vg):
                t.grad = None
            fn().backward(gy)
        return run

    def kernel_out():
        env(None)
        return attn(qg, kg, vg)

    def eager_out():
        env("0")
        out = attn(qg, kg, vg)
        env(None)
        return out

    variants = {
        "kernel": (kernel_fwd, fb(kernel_out), 5),
        "eager": (eager_fwd, fb(eager_out), 1),
        "dense": (dense_fwd, fb(lambda: flash_attention(qg, kg, vg, scale)), 5),
    }
    if args.no_eager:
        del variants["eager"]

    # spot check: kernel vs eager on this very point (first 2 heads)
    err = None
    if "eager" in variants:
        ok, oe = kernel_fwd(), eager_fwd()
        err = ((ok.float() - oe.float()).abs().max()
               / oe.float().abs().max().clamp(min=1.0)).item()
        del ok, oe

    times = {n: {"fwd": [], "fwd_bwd": []} for n in variants}
    for n, (f, fbk, _) in variants.items():      # warm-up
        f(); fbk()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for n, (f, fbk, inner) in variants.items():
            times[n]["fwd"].append(timed(f, inner))
        for n, (f, fbk, inner) in variants.items():
            times[n]["fwd_bwd"].append(timed(fbk, inner))

    rec = {"layout": name, "block": block, "s": s, "b": b, "h": h, "d": d,
           "density": round(density, 5), "active_sub_tiles": sub_tiles,
           "kernel_vs_eager_rel_err": err, "repeats": repeats}
    for n in variants:
        for ph in ("fwd", "fwd_bwd"):
            ts = times[n][ph]
            rec[f"{n}_{ph}_ms"] = {"median": round(statistics.median(ts), 4),
                                   "min": round(min(ts), 4),
                                   "max": round(max(ts), 4)}
    km = rec["kernel_fwd_ms"]["median"]
    kfb = rec["kernel_fwd_bwd_ms"]["median"]
    rec["kernel_fwd_tflops_active"] = round(fwd_flops / km / 1e9, 2)
    rec["kernel_fwd_bwd_tflops_active"] = round(3.5 * fwd_flops / kfb / 1e9, 2)
    return rec


lines = []
for s in seqs:
    for name in ("bigbird", "local"):
        for block in (16, 64):
            rec = run_point(name, block, s)
            line = json.dumps(rec)
            print(line, flush=True)
            lines.append(line)
            if args.out:
                os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
                with open(args.out, "w") as f:
                    f.write("\n".join(lines) + "\n")
