"""Grouped-query causal flash attention benchmark.

For each (h_kv, seq_len) at b2 h32 d128 times forward and forward+backward of
  native : flash_attention on k/v with h_kv heads (grouped-query v3 kernels)
  expand : K/V expanded to h heads (ops.flash.expand_kv) + the plain v3
           kernels + the group-sum of dK/dV that autograd adds: what a user
           has without the grouped-query kernels
  mha    : plain v3 kernels on an h-head K/V of the same size.  Same FLOPs,
           not the same function: the yardstick for what the extra indexing
           and the group loop of dkv cost
and the peak memory of forward+backward of native and expand.
The variants alternate inside every repeat, in one process, after a
warm-up; times come from device events.  Prints one JSON line per point
with the median and the min..max spread over the repeats.

--step instead times forward + backward of a LLaMA with the Llama-3-8B layer
shape (hidden 4096, 32 heads, 8 KV heads) at b4 s2048, with
FENGSHEN_GQA_FLASH=0 and =1 alternating: tokens/s and peak memory.

Usage: python scripts/flash_gqa_bench.py [--quick] [--step] [--out FILE]
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, json, math, statistics
import torch
from fengshen_amd.ops.flash import expand_kv, flash_attention

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="s=2048 only, 2 repeats")
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--step", action="store_true")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--batch", type=int, default=4)
args = ap.parse_args()

b, h, d = 2, 32, 128
scale = 1 / math.sqrt(d)
points = [(8, 2048), (1, 2048)] if args.quick else \
    [(8, 2048), (8, 8192), (1, 2048)]
repeats = 2 if args.quick else args.repeats


def env(val):
    if val is None:
        os.environ.pop("FENGSHEN_GQA_FLASH", None)
    else:
        os.environ["FENGSHEN_GQA_FLASH"] = val


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


def peak_of(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def run_point(h_kv, s):
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(heads):
        return torch.randn(b, heads, s, d, generator=g, device="cuda") \
            .to(torch.bfloat16)
    q, gy = rnd(h), rnd(h)
    k, v = rnd(h_kv), rnd(h_kv)
    kf, vf = rnd(h), rnd(h)          # the MHA yardstick's own K/V
    inner = 5

    def native(a, b_, c):
        return flash_attention(a, b_, c, scale)

    def expand(a, b_, c):
        return flash_attention(a, expand_kv(b_, h), expand_kv(c, h), scale)

    sets = {"native": (native, (q, k, v)), "expand": (expand, (q, k, v)),
            "mha": (native, (q, kf, vf))}
    variants = {}
    for n, (fn, ts) in sets.items():
        leaves = [t.clone().requires_grad_(True) for t in ts]

        def fwd(fn=fn, ts=ts):
            with torch.no_grad():
                return fn(*ts)

        def fb(fn=fn, leaves=leaves):
            for t in leaves:
                t.grad = None
            fn(*leaves).backward(gy)
        variants[n] = (fwd, fb)

    # spot check on this very point: same function, two routes
    on, oe = variants["native"][0](), variants["expand"][0]()
    same = bool(torch.equal(on, oe))
    del on, oe

    times = {n: {"fwd": [], "fwd_bwd": []} for n in variants}
    for n, (f, fbk) in variants.items():         # warm-up
        f(); fbk()
    torch.cuda.synchronize()
    peak = {n: peak_of(variants[n][1]) for n in ("native", "expand")}
    for _ in range(repeats):
        for n, (f, fbk) in variants.items():
            times[n]["fwd"].append(timed(f, inner))
        for n, (f, fbk) in variants.items():
            times[n]["fwd_bwd"].append(timed(fbk, inner))

    rec = {"s": s, "b": b, "h": h, "h_kv": h_kv, "d": d,
           "native_o_equals_expand_o": same, "repeats": repeats}
    for n in variants:
        for ph in ("fwd", "fwd_bwd"):
            rec[f"{n}_{ph}_ms"] = spread(times[n][ph])
    for n in peak:
        rec[f"{n}_fwd_bwd_peak_MiB"] = round(peak[n] / 2**20, 1)
    return rec


def train_step():
    from fengshen_amd.models.llama.configuration_llama import llama3_8b_config
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    s, bs = 2048, args.batch
    cfg = llama3_8b_config(num_hidden_layers=args.layers, vocab_size=32000,
                           max_position_embeddings=s)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().train()
    ids = torch.randint(3, cfg.vocab_size, (bs, s), device="cuda")

    def step():
        model.zero_grad(set_to_none=True)
        model(ids, labels=ids).loss.backward()

    rec = {"step": True, "layers": args.layers, "b": bs, "s": s,
           "hidden": cfg.hidden_size, "heads": cfg.num_attention_heads,
           "kv_heads": cfg.num_key_value_heads, "vocab": cfg.vocab_size,
           "repeats": repeats}
    times = {"0": [], "1": []}
    peak = {}
    for val in ("0", "1"):                       # warm-up + peak memory
        env(val)
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[val] = torch.cuda.max_memory_allocated()
    for _ in range(repeats):
        for val in ("0", "1"):
            env(val)
            times[val].append(timed(step, 2))
    env(None)
    for val, name in (("0", "expand"), ("1", "native")):
        rec[f"{name}_step_ms"] = spread(times[val])
        rec[f"{name}_tokens_per_s"] = round(
            bs * s / statistics.median(times[val]) * 1e3, 1)
        rec[f"{name}_peak_GiB"] = round(peak[val] / 2**30, 3)
    return rec


lines = []


def emit(rec):
    line = json.dumps(rec)
    print(line, flush=True)
    lines.append(line)
    if args.out:
        os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if args.step:
    emit(train_step())
else:
    for h_kv, s in points:
        emit(run_point(h_kv, s))
