"""Flash v3 kernel times at the flagship step's shape, by work distribution.

Times get_ext().flash_attn_fwd_v3 and flash_attn_bwd_v3 (delta + dq + dkv) at
b16 h40 d128 for three cases
  causal_s2048    : 8 blocks per (batch, head), work 1..8 by block x
  noncausal_s2048 : the same grid, every block streams all 32 key tiles
                    (a causal block streams 18 on average)
  causal_s1792    : 7 blocks per (batch, head): an odd count spreads the
                    blocks of one x over all XCDs by itself
If the chip hands a free CU the next block wherever it sits, non-causal takes
32 / 18 = 1.78 x the causal time; if every XCD only runs the blocks dealt to
it round-robin by linear block id, plain causal s2048 puts all blocks of one
x on one XCD and takes about as long as non-causal.  The cases alternate
inside every repeat, in one process, after a warm-up; times come from device
events.  Prints one JSON line per case with the median and min..max over the
repeats, and the rate over the flop the mask leaves (2 GEMMs of the 256 x 256
tiles on or below the diagonal forward, 5 backward).

Usage: python scripts/flash_xcd_bench.py [--repeats N] [--inner N] [--out FILE]
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, json, math, statistics
import torch
from fengshen_amd.ops import get_ext

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--inner", type=int, default=5)
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--heads", type=int, default=40)
ap.add_argument("--out", default=None)
args = ap.parse_args()

ext = get_ext()
b, h, d = args.batch, args.heads, 128
scale = 1 / math.sqrt(d)
cases = [("causal_s2048", 2048, True), ("noncausal_s2048", 2048, False),
         ("causal_s1792", 1792, True)]


def timed(fn, inner):
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / inner


def spread(ts):
    return {"median": round(statistics.median(ts), 4),
            "min": round(min(ts), 4), "max": round(max(ts), 4)}


def make(s, causal):
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, gy = (torch.randn(b, h, s, d, generator=g, device="cuda")
                   .to(torch.bfloat16) for _ in range(4))
    o, lse = ext.flash_attn_fwd_v3(q, k, v, scale, causal, None, 0.0, 0)

    def fwd():
        ext.flash_attn_fwd_v3(q, k, v, scale, causal, None, 0.0, 0)

    def bwd():
        ext.flash_attn_bwd_v3(q, k, v, o, gy, lse, scale, causal, None, 0.0, 0)
    return fwd, bwd


fns = {n: make(s, c) for n, s, c in cases}
times = {n: {"fwd": [], "bwd": []} for n in fns}
for f, bk in fns.values():                       # warm-up
    f(); bk()
torch.cuda.synchronize()
for _ in range(args.repeats):
    for n, (f, bk) in fns.items():
        times[n]["fwd"].append(timed(f, args.inner))
    for n, (f, bk) in fns.items():
        times[n]["bwd"].append(timed(bk, args.inner))

lines = []
for n, s, causal in cases:
    nx = s // 256
    # 256 x 256 score tiles a (batch, head) needs: the causal triangle with
    # its diagonal, or the full square
    tiles = nx * (nx + 1) // 2 if causal else nx * nx
    tflop = b * h * tiles * 256 * 256 * d * 2 / 1e12   # one S-like GEMM
    rec = {"case": n, "b": b, "h": h, "s": s, "d": d, "causal": causal,
           "blocks_per_head": nx, "repeats": args.repeats,
           "fwd_ms": spread(times[n]["fwd"]),
           "bwd_ms": spread(times[n]["bwd"]),
           "fwd_TFs": round(2 * tflop / statistics.median(times[n]["fwd"])
                            * 1e3, 1),
           "bwd_TFs": round(5 * tflop / statistics.median(times[n]["bwd"])
                            * 1e3, 1)}
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)
base = statistics.median(times["causal_s2048"]["fwd"])
baseb = statistics.median(times["causal_s2048"]["bwd"])
line = json.dumps({
    "noncausal_over_causal_fwd": round(
        statistics.median(times["noncausal_s2048"]["fwd"]) / base, 3),
    "noncausal_over_causal_bwd": round(
        statistics.median(times["noncausal_s2048"]["bwd"]) / baseb, 3),
    "work_conserving_would_be": round(32 / 18, 3)})
print(line, flush=True)
lines.append(line)
if args.out:
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
