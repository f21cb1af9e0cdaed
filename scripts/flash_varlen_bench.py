"""Causal flash attention with a per-row key start (kstart) benchmark.

For each (case, seq_len) times forward and forward+backward of
  kstart : flash_attention(..., kstart=...) on the kstart v3 kernels
  dense  : plain causal v3 flash attention on the same tensors (it ignores
           the mask: the cost yardstick, not the same function)
  bmm    : ops.functional.attention under the dense mask with
           FENGSHEN_VARLEN_FLASH=0 (bmm + masked softmax, what such a batch
           ran on before)
Cases: docs8 (8 equal documents, active area 1/8 of causal), one (kstart = 0:
what the extra load and compare cost), pad25 (25 % right padding).
The variants alternate inside every repeat, in one process, after a
warm-up; times come from device events.  Prints one JSON line per point
with the median and the min..max spread over the repeats.

--sft-step instead times one padded SFT training step (forward + backward,
25 % right padding) of a LLaMA with the Ziya-13B layer shape, with
FENGSHEN_VARLEN_FLASH=0 and =1 alternating: tokens/s and peak memory.

Usage: python scripts/flash_varlen_bench.py [--quick] [--sft-step] [--out FILE]
"""
import sys, os; sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import argparse, json, math, statistics
import torch
from fengshen_amd.ops import functional as F
from fengshen_amd.ops.flash import flash_attention, kstart_to_mask

ap = argparse.ArgumentParser()
ap.add_argument("--quick", action="store_true", help="s=2048 only, 2 repeats")
ap.add_argument("--out", default=None)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-bmm", action="store_true")
ap.add_argument("--sft-step", action="store_true")
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--batch", type=int, default=4)
args = ap.parse_args()

b, h, d = 2, 16, 128
scale = 1 / math.sqrt(d)
seqs = (2048,) if args.quick else (2048, 8192)
repeats = 2 if args.quick else args.repeats


def env(val):
    if val is None:
        os.environ.pop("FENGSHEN_VARLEN_FLASH", None)
    else:
        os.environ["FENGSHEN_VARLEN_FLASH"] = val


def make_kstart(case, s):
    ar = torch.arange(s, device="cuda", dtype=torch.int32)
    if case == "docs8":
        ks = ar // (s // 8) * (s // 8)
    elif case == "one":
        ks = torch.zeros_like(ar)
    else:  # pad25: real rows start at 0, pad rows see themselves
        ks = torch.where(ar < s - s // 4, torch.zeros_like(ar), ar)
    return ks.unsqueeze(0).repeat(b, 1).contiguous()


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


def run_point(case, s):
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, gy = (torch.randn(b, h, s, d, generator=g, device="cuda")
                   .to(torch.bfloat16) for _ in range(4))
    qg, kg, vg = (t.clone().requires_grad_(True) for t in (q, k, v))
    ks = make_kstart(case, s)
    mask = kstart_to_mask(ks)

    def bmm_out(a, b_, c):
        env("0")
        out = F.attention(a, b_, c, causal=True, mask=mask, scale=scale)
        env(None)
        return out

    def nograd(fn):
        def run():
            with torch.no_grad():
                return fn(q, k, v)
        return run

    def fb(fn):
        def run():
            for t in (qg, kg, vg):
                t.grad = None
            fn(qg, kg, vg).backward(gy)
        return run

    outs = {
        "kstart": (lambda a, b_, c: flash_attention(a, b_, c, scale,
                                                    kstart=ks), 5),
        "dense": (lambda a, b_, c: flash_attention(a, b_, c, scale), 5),
        "bmm": (bmm_out, 1),
    }
    if args.no_bmm:
        del outs["bmm"]
    variants = {n: (nograd(f), fb(f), inner) for n, (f, inner) in outs.items()}

    # spot check on this very point: kstart kernels vs the bmm path
    err = None
    if "bmm" in variants:
        ok, oe = variants["kstart"][0](), variants["bmm"][0]()
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

    rec = {"case": case, "s": s, "b": b, "h": h, "d": d,
           "kstart_vs_bmm_rel_err": err, "repeats": repeats}
    for n in variants:
        for ph in ("fwd", "fwd_bwd"):
            rec[f"{n}_{ph}_ms"] = spread(times[n][ph])
    return rec


def sft_step():
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    s, bs = 2048, args.batch
    cfg = LlamaConfig(vocab_size=39424, hidden_size=5120,
                      num_hidden_layers=args.layers, num_attention_heads=40,
                      intermediate_size=13824, max_position_embeddings=s)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().train()
    ids = torch.randint(3, 39424, (bs, s), device="cuda")
    am = torch.ones(bs, s, dtype=torch.long, device="cuda")
    am[:, s - s // 4:] = 0
    labels = ids.masked_fill(am == 0, -100)

    def step():
        model.zero_grad(set_to_none=True)
        model(ids, attention_mask=am, labels=labels).loss.backward()

    rec = {"sft_step": True, "layers": args.layers, "b": bs, "s": s,
           "hidden": 5120, "heads": 40, "pad": 0.25, "repeats": repeats}
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
    for val, name in (("0", "bmm"), ("1", "kstart")):
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


if args.sft_step:
    emit(sft_step())
else:
    for s in seqs:
        for case in ("docs8", "one", "pad25"):
            emit(run_point(case, s))
