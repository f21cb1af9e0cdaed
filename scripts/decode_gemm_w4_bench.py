"""decode_gemm_w4 (split-K MFMA GEMM for int4 weights) against the int8 path
for the same call (w8_gemv at 1 row, decode_gemm above) at the five 13B
projection shapes, both tiles-per-wave builds.

    python scripts/decode_gemm_w4_bench.py             # the kernel table
    python scripts/decode_gemm_w4_bench.py --decoder   # ... and ms/token
    python scripts/decode_gemm_w4_bench.py --step 0    # one step, in-process

Every step runs in a child process of its own under a time limit; the first
step that fails ends the script.  Times are device events around ITERS
back-to-back calls; the paths alternate inside each of 5 repeats after a
warm-up, and the tables give median [min, max] in us per call.  GB/s counts
the weight bytes (int4: nibbles plus bf16 group scales); the floor is those
bytes at 6.3 TB/s.
"""
import argparse
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

SHAPES = [(15360, 5120), (5120, 5120), (27648, 5120), (5120, 13824),
          (39424, 5120)]  # out x K: qkv, out_proj, gate_up, down, lm_head
ROWS = [1, 2, 4, 8, 16]
REPEATS, ITERS = 5, 20
HBM_BPS = 6.3e12
STEPS = ["kernel", "decoder-1", "decoder-8"]
STEP_TIMEOUT = 280  # seconds per child


def _time(fn, iters=ITERS):
    import torch
    beg = torch.cuda.Event(enable_timing=True)
    end = torch.cuda.Event(enable_timing=True)
    beg.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return beg.elapsed_time(end) * 1e3 / iters  # us per call


def _fmt(ts):
    return f"{statistics.median(ts):6.1f} [{min(ts):5.1f}, {max(ts):5.1f}]"


def _verdict(new, old):
    return ("yes" if max(new) < min(old) else
            "no" if min(new) > max(old) else "within spread")


def kernel_step():
    import torch
    from fengshen_amd.ops import get_ext
    from fengshen_amd.utils.quantize import W4Linear, W8Linear
    ext = get_ext()
    print("## int4 against int8 weights   (us per call: median [min, max])")
    print("| out x K | rows | int8 floor | int8 | GB/s | int4 floor | "
          "int4 tw=1 | GB/s | int4 tw=2 | GB/s | tw=1 wins | tw=2 wins | "
          "max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    for out, K in SHAPES:
        torch.manual_seed(out + K)
        w = (torch.randn(out, K, device="cuda") * 0.05).bfloat16()
        q8, q4 = W8Linear(w), W4Linear(w)
        s8 = q8.scale.view(-1)
        del w
        b8 = q8.qweight.numel()
        b4 = q4.qweight.numel() + 2 * q4.scales.numel()
        for rows in ROWS:
            x = torch.randn(rows, K, device="cuda").bfloat16()

            def old():
                if rows == 1:
                    return ext.w8_gemv(q8.qweight, s8, x)
                return ext.decode_gemm(q8.qweight, x, s8)

            def new1():
                return ext.decode_gemm_w4(q4.qweight, q4.scales, x, out, 0, 1)

            def new2():
                return ext.decode_gemm_w4(q4.qweight, q4.scales, x, out, 0, 2)
            diff = float((new1().float() - new2().float()).abs().max())
            fns = (old, new1, new2)
            for f in fns:
                _time(f)
            ts = ([], [], [])
            for _ in range(REPEATS):
                for f, t in zip(fns, ts):
                    t.append(_time(f))
            print(f"| {out} x {K} | {rows} | {b8 / HBM_BPS * 1e6:5.1f} | "
                  f"{_fmt(ts[0])} | "
                  f"{b8 / statistics.median(ts[0]) / 1e3:5.0f} | "
                  f"{b4 / HBM_BPS * 1e6:5.1f} | {_fmt(ts[1])} | "
                  f"{b4 / statistics.median(ts[1]) / 1e3:5.0f} | "
                  f"{_fmt(ts[2])} | "
                  f"{b4 / statistics.median(ts[2]) / 1e3:5.0f} | "
                  f"{_verdict(ts[1], ts[0])} | {_verdict(ts[2], ts[0])} | "
                  f"{diff:.4f} |", flush=True)
        del q8, q4


def decoder_step(batch):
    """4 layers of the Ziya-13B layer shape in GraphedDecoder, max_len 2048,
    512-token prompt: ms/token of the captured step with int8 and with int4
    weights (FENGSHEN_DECODE_GEMM=auto), a model, a decoder and a graph per
    format, alternating in each repeat."""
    import torch
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    from fengshen_amd.utils.quantize import (
        quantize_model_int4, quantize_model_int8)
    cfg = LlamaConfig(vocab_size=39424, hidden_size=5120,
                      num_hidden_layers=4, num_attention_heads=40,
                      intermediate_size=13824, max_position_embeddings=2048)
    ids = torch.randint(3, 39424, (batch, 512), device="cuda")
    decs = {}
    for name, quant in (("int8", quantize_model_int8),
                        ("int4", quantize_model_int4)):
        torch.manual_seed(0)
        model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().eval()
        decs[name] = GraphedDecoder(quant(model), batch=batch, max_len=2048,
                                    max_new_tokens=64)
        decs[name].generate(ids, max_new_tokens=8)  # capture + warm-up
    times = {name: [] for name in decs}
    for _ in range(REPEATS):
        for name, dec in decs.items():
            dec._prefill(ids)
            times[name].append(_time(dec._graph.replay, 48) / 1e3)
    for name, ts in times.items():
        print(f"GraphedDecoder 4 layers, batch {batch}, {name}: "
              f"{statistics.median(ts):.3f} ms/token "
              f"[{min(ts):.3f}, {max(ts):.3f}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decoder", action="store_true",
                    help="also run the end-to-end GraphedDecoder steps")
    ap.add_argument("--step", type=int, default=None,
                    help=f"run one of {STEPS} in this process")
    args = ap.parse_args()
    if args.step is not None:
        import torch
        if not torch.cuda.is_available():
            sys.exit("decode_gemm_w4_bench needs a GPU")
        name = STEPS[args.step]
        if name == "kernel":
            kernel_step()
        else:
            decoder_step(int(name.split("-")[1]))
        return 0
    for step in range(len(STEPS) if args.decoder else 1):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__),
                             "--step", str(step)],
                            timeout=STEP_TIMEOUT).returncode
        if rc != 0:
            print(f"step {STEPS[step]} failed with exit status {rc}; stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
