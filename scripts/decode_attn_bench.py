"""decode_attn (one block per head, serial over the prefix) against
decode_attn_split (split-KV, grouped heads) on the same tensors and
decode_attn_split_q8 on their int8 quantisation (head dim 64 / 128), and the
end-to-end ms/token of GraphedDecoder with either kernel and, with
--kv-cache int8, with the int8 cache.

    python scripts/decode_attn_bench.py            # every step
    python scripts/decode_attn_bench.py --step 1   # one step, in-process
    python scripts/decode_attn_bench.py --tokens 4 8 16   # multi-token axis

--tokens T... replaces the tables above by those of the multi-token step
(decode_attn_split(..., tokens=T), decode_attn_mt.hip): per call at
MT_SHAPES, b in BATCHES, pos in MT_POSITIONS, one T-token call against one
tokens=1 call and against T of them, and end to end GraphedDecoder with
lookahead = the first T against lookahead = 1, once with the true
continuation as hint_ids and once without a hint on random tokens.

Every step runs in a child process of its own under a time limit; the first
step that fails ends the script.  Times are device events around ITERS
back-to-back calls; the kernels alternate inside each of 5 repeats after a
warm-up, and the table gives median [min, max] per call.  K/V GB/s counts
2 * (pos + 1) * h_kv * d * 2 * b bytes; the floor is those bytes at 6.3 TB/s.
The int8 kernel's GB/s counts what it reads, 2 * (pos + 1) * h_kv * (d + 4)
* b bytes (rows and their fp32 scales), and "% floor" is the time those bytes
take at 6.3 TB/s over the measured time.
"""
import argparse
import math
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

SHAPES = [(40, 40, 128), (32, 8, 128), (32, 1, 128), (36, 36, 96),
          (4, 4, 64)]
BATCHES = [1, 8]
POSITIONS = [511, 2047, 8191, 32767]
REPEATS, ITERS = 5, 20
HBM_BPS = 6.3e12
STEP_TIMEOUT = 240  # seconds per child
MT_SHAPES = [(40, 40, 128), (32, 8, 128)]
MT_POSITIONS = [2047, 8191]


def _time(fn):
    import torch
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(ITERS):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / ITERS  # us per call


def _fmt(ts):
    return f"{statistics.median(ts):8.1f} [{min(ts):7.1f}, {max(ts):7.1f}]"


def kernel_step(idx):
    import torch
    from fengshen_amd.ops import functional as F_ops
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d = SHAPES[idx]
    scale = 1 / math.sqrt(d)
    print(f"## h={h} h_kv={h_kv} d={d}   (us per call: median [min, max])")
    print("| b | pos | floor us | decode_attn | GB/s | decode_attn_split "
          "| GB/s | max abs diff | decode_attn_split_q8 | GB/s | % floor | "
          "max abs diff to split |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for b in BATCHES:
        for p in POSITIONS:
            L = p + 1
            torch.manual_seed(p + b)
            qkv = (torch.randn(b, (h + 2 * h_kv) * d, device="cuda")
                   * 0.5).bfloat16()
            kc = (torch.randn(b, h_kv, L, d, device="cuda") * 0.5).bfloat16()
            vc = (torch.randn(b, h_kv, L, d, device="cuda") * 0.5).bfloat16()
            cos, sin = F_ops.build_rope_cache(L, d)
            cos, sin = cos.cuda(), sin.cuda()
            pos1 = torch.tensor([p], device="cuda")
            posb = torch.full((b,), p, device="cuda")
            nbytes = 2 * (p + 1) * h_kv * d * 2 * b

            def new():
                return ext.decode_attn_split(qkv, kc, vc, cos, sin, posb,
                                             scale, True)

            def old():
                return ext.decode_attn(qkv, kc, vc, cos, sin, pos1, scale,
                                       True)
            has_old = d in (64, 128)  # and the int8 kernel
            diff = diff8 = float("nan")
            if has_old:
                kq, ks = ext.kv_quantize_int8(kc)
                vq, vs = ext.kv_quantize_int8(vc)
                nbytes8 = 2 * (p + 1) * h_kv * (d + 4) * b

                def q8():
                    return ext.decode_attn_split_q8(qkv, kq, ks, vq, vs, cos,
                                                    sin, posb, scale, True)
                diff = float((old().float() - new().float()).abs().max())
                diff8 = float((q8().float() - new().float()).abs().max())
                _time(old)
                _time(q8)
            _time(new)
            t_old, t_new, t_q8 = [], [], []
            for _ in range(REPEATS):
                if has_old:
                    t_old.append(_time(old))
                    t_q8.append(_time(q8))
                t_new.append(_time(new))
            o = (f"{_fmt(t_old)} | "
                 f"{nbytes / statistics.median(t_old) / 1e3:6.0f}"
                 if has_old else "- | -")
            print(f"| {b} | {p} | {nbytes / HBM_BPS * 1e6:6.1f} | {o} | "
                  f"{_fmt(t_new)} | "
                  f"{nbytes / statistics.median(t_new) / 1e3:6.0f} | "
                  f"{diff:.4f} | " + (
                      f"{_fmt(t_q8)} | "
                      f"{nbytes8 / statistics.median(t_q8) / 1e3:6.0f} | "
                      f"{nbytes8 / HBM_BPS * 1e8 / statistics.median(t_q8):4.0f}"
                      f" | {diff8:.4f} |" if has_old else "- | - | - | - |"),
                  flush=True)
            del qkv, kc, vc


def e2e_step(kv_cache="bf16", batch=1):
    """4 layers of the Ziya-13B layer shape, max_len 8192, 4096-token prompt:
    ms/token of the captured step with FENGSHEN_DECODE_SPLIT=0 and =1, and
    with kv_cache "int8" a third decoder with the int8 cache, alternating."""
    import torch
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=39424, hidden_size=5120,
                      num_hidden_layers=4, num_attention_heads=40,
                      intermediate_size=13824, max_position_embeddings=8192)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().eval()
    ids = torch.randint(3, 39424, (batch, 4096), device="cuda")
    decs = {}
    runs = [("0", "bf16"), ("1", "bf16")]
    if kv_cache == "int8":
        runs.append(("1", "int8"))
    for split, kv in runs:
        os.environ["FENGSHEN_DECODE_SPLIT"] = split
        mode = f"{split} kv_cache={kv}"
        decs[mode] = GraphedDecoder(model, batch=batch, max_len=8192,
                                    max_new_tokens=64, kv_cache=kv)
        decs[mode].generate(ids, max_new_tokens=8)  # capture + warm-up
    times = {mode: [] for mode in decs}
    for _ in range(REPEATS):
        for mode, dec in decs.items():
            dec._prefill(ids)
            beg = torch.cuda.Event(enable_timing=True)
            end = torch.cuda.Event(enable_timing=True)
            beg.record()
            for _ in range(48):
                dec._graph.replay()
            end.record()
            end.synchronize()
            times[mode].append(beg.elapsed_time(end) / 48)
    for mode, ts in times.items():
        dec = decs[mode]
        cache = dec.k_cache + dec.v_cache + (
            dec.k_scale + dec.v_scale if dec.kv_cache == "int8" else [])
        print(f"GraphedDecoder 4 layers, batch {batch}, pos 4096.., "
              f"FENGSHEN_DECODE_SPLIT={mode}: {statistics.median(ts):.3f} "
              f"ms/token [{min(ts):.3f}, {max(ts):.3f}], cache "
              f"{sum(t.numel() * t.element_size() for t in cache) / 2**20:.0f}"
              " MiB", flush=True)


def multitok_step(idx, tokens):
    """One T-token call against one tokens=1 call and against T of them (at
    pos .. pos+T-1, what T single steps would run), alternating."""
    import torch
    from fengshen_amd.ops import functional as F_ops
    from fengshen_amd.ops import get_ext
    ext = get_ext()
    h, h_kv, d = MT_SHAPES[idx]
    scale = 1 / math.sqrt(d)
    print(f"## h={h} h_kv={h_kv} d={d}   (us per call: median [min, max])")
    print("| b | pos | T | tokens=1 | T x tokens=1 | tokens=T | "
          "T singles / one T call | max abs diff |")
    print("|---|---|---|---|---|---|---|---|")
    for b in BATCHES:
        for p in MT_POSITIONS:
            for T in tokens:
                L = p + T
                torch.manual_seed(p + b)
                qkv = (torch.randn(b, T, (h + 2 * h_kv) * d, device="cuda")
                       * 0.5).bfloat16()
                kc = (torch.randn(b, h_kv, L, d, device="cuda")
                      * 0.5).bfloat16()
                vc = (torch.randn(b, h_kv, L, d, device="cuda")
                      * 0.5).bfloat16()
                cos, sin = F_ops.build_rope_cache(L, d)
                cos, sin = cos.cuda(), sin.cuda()
                post = [torch.full((b,), p + t, device="cuda")
                        for t in range(T)]
                rows = [qkv[:, t].contiguous() for t in range(T)]

                def one():
                    return ext.decode_attn_split(rows[0], kc, vc, cos, sin,
                                                 post[0], scale, True)

                def singles():
                    return [ext.decode_attn_split(rows[t], kc, vc, cos, sin,
                                                  post[t], scale, True)
                            for t in range(T)]

                def multi():
                    return ext.decode_attn_split(qkv, kc, vc, cos, sin,
                                                 post[0], scale, True,
                                                 tokens=T)
                diff = float((torch.stack(singles(), 1).float()
                              - multi().float()).abs().max())
                for fn in (one, singles, multi):
                    _time(fn)
                t_one, t_sing, t_mt = [], [], []
                for _ in range(REPEATS):
                    t_one.append(_time(one))
                    t_sing.append(_time(singles))
                    t_mt.append(_time(multi))
                ratio = statistics.median(t_sing) / statistics.median(t_mt)
                print(f"| {b} | {p} | {T} | {_fmt(t_one)} | {_fmt(t_sing)} | "
                      f"{_fmt(t_mt)} | {ratio:.2f} | {diff:.4f} |", flush=True)
                del qkv, kc, vc


def lookahead_step(T, batch=1, n=64):
    """4 layers of the Ziya-13B layer shape, max_len 8192, 4096-token random
    prompt: host-clock ms per generated token of the replay loop (prefill
    excluded, n - 1 tokens) with lookahead=1 and lookahead=T, alternating;
    lookahead=T once with its own continuation as the hint and once
    without a hint."""
    import time

    import torch
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=39424, hidden_size=5120,
                      num_hidden_layers=4, num_attention_heads=40,
                      intermediate_size=13824, max_position_embeddings=8192)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().eval()
    ids = torch.randint(3, 39424, (batch, 4096), device="cuda")
    os.environ["FENGSHEN_DECODE_SPLIT"] = "1"
    base = GraphedDecoder(model, batch=batch, max_len=8192, max_new_tokens=n)
    look = GraphedDecoder(model, batch=batch, max_len=8192, max_new_tokens=n,
                          lookahead=T)
    want = base.generate(ids)[:, 4096:]
    got = look.generate(ids)[:, 4096:]
    agree = int((want == got).long().cumprod(1).sum(1).min())
    print(f"lookahead={T} and lookahead=1 agree on the first {agree} of {n} "
          "tokens (bf16, random weights: near-ties may flip)", flush=True)
    hint = got  # the continuation this decoder takes

    def run(mode):
        if mode == "lookahead=1":
            base._prefill(ids)
        else:
            look._start_lookahead(ids, None,
                                  hint if "true hint" in mode else None)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if mode == "lookahead=1":
            for _ in range(n - 1):
                base._graph.replay()
            reps = n - 1
        else:
            look._run_lookahead(n)
            reps = look.last_replays
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / (n - 1), reps
    modes = ["lookahead=1", f"lookahead={T}, true hint",
             f"lookahead={T}, no hint"]
    times = {m: [] for m in modes}
    reps = {}
    for _ in range(REPEATS):
        for m in modes:
            t, reps[m] = run(m)
            times[m].append(t)
    for m in modes:
        ts = times[m]
        print(f"GraphedDecoder 4 layers, batch {batch}, pos 4096.., {m}: "
              f"{statistics.median(ts):.3f} ms/token [{min(ts):.3f}, "
              f"{max(ts):.3f}], {reps[m]} replays for {n - 1} tokens, "
              f"{statistics.median(ts) * (n - 1) / reps[m]:.3f} ms/replay",
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", type=int, default=None,
                    help="0..4: kernel table of SHAPES[step]; 5: end to end")
    ap.add_argument("--kv-cache", choices=["bf16", "int8"], default="bf16",
                    help="end to end: int8 adds a decoder with the int8 cache")
    ap.add_argument("--batch", type=int, default=1, help="end to end batch")
    ap.add_argument("--tokens", type=int, nargs="+", default=None,
                    help="multi-token step: T values of the kernel tables "
                         "(steps 0..1); step 2 is end to end with "
                         "lookahead = the first of them")
    args = ap.parse_args()
    if args.tokens is not None:
        if not all(2 <= t <= 16 for t in args.tokens):
            ap.error("--tokens values must be in 2..16")
        if args.step is not None:
            if args.step == len(MT_SHAPES):
                lookahead_step(args.tokens[0], args.batch)
            else:
                multitok_step(args.step, args.tokens)
            return 0
        for step in range(len(MT_SHAPES) + 1):
            rc = subprocess.run(
                [sys.executable, os.path.abspath(__file__), "--step",
                 str(step), "--batch", str(args.batch), "--tokens"]
                + [str(t) for t in args.tokens],
                timeout=STEP_TIMEOUT).returncode
            if rc != 0:
                print(f"step {step} failed with exit status {rc}; stopping")
                return rc
        return 0
    if args.step is not None:
        if args.step == len(SHAPES):
            e2e_step(args.kv_cache, args.batch)
        else:
            kernel_step(args.step)
        return 0
    for step in range(len(SHAPES) + 1):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__),
                             "--step", str(step), "--kv-cache", args.kv_cache,
                             "--batch", str(args.batch)],
                            timeout=STEP_TIMEOUT).returncode
        if rc != 0:
            print(f"step {step} failed with exit status {rc}; stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
