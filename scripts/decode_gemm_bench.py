"""decode_gemm (MFMA weight-streaming GEMM for 2..16 rows) against what
FENGSHEN_DECODE_GEMM=0 runs for the same call: F.linear (hipBLASLt) for bf16
weights, w8_gemv for int8 weights, at the five 13B projection shapes.

    python scripts/decode_gemm_bench.py             # both kernel tables
    python scripts/decode_gemm_bench.py --decoder   # ... and ms/token
    python scripts/decode_gemm_bench.py --step 0    # one step, in-process

Every step runs in a child process of its own under a time limit; the first
step that fails ends the script.  Times are device events around ITERS
back-to-back calls; the two paths alternate inside each of 5 repeats after a
warm-up, and the tables give median [min, max] in us per call.  GB/s counts
the weight bytes; the floor is those bytes at 6.3 TB/s.
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
ROWS = [2, 4, 8, 16]
REPEATS, ITERS = 5, 20
HBM_BPS = 6.3e12
STEPS = ["bf16", "int8", "decoder-bf16", "decoder-int8"]
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
    return f"{statistics.median(ts):7.1f} [{min(ts):6.1f}, {max(ts):6.1f}]"


def kernel_step(w8):
    import torch
    from fengshen_amd.ops import get_ext
    from fengshen_amd.utils.quantize import W8Linear
    ext = get_ext()
    old_name = "w8_gemv" if w8 else "F.linear"
    print(f"## {'int8' if w8 else 'bf16'} weights   (us per call: median "
          "[min, max])")
    print(f"| out x K | rows | floor us | {old_name} | GB/s | decode_gemm | "
          "GB/s | wins | max abs diff |")
    print("|---|---|---|---|---|---|---|---|---|")
    for out, K in SHAPES:
        torch.manual_seed(out + K)
        w = (torch.randn(out, K, device="cuda") * 0.05).bfloat16()
        scale = None
        if w8:
            q = W8Linear(w)
            w, scale = q.qweight, q.scale.view(-1)
        nbytes = w.numel() * w.element_size()
        for rows in ROWS:
            x = torch.randn(rows, K, device="cuda").bfloat16()

            def new():
                return ext.decode_gemm(w, x, scale)

            def old():
                if w8:
                    return ext.w8_gemv(w, scale, x)
                return torch.nn.functional.linear(x, w)
            diff = float((old().float() - new().float()).abs().max())
            _time(old)
            _time(new)
            t_old, t_new = [], []
            for _ in range(REPEATS):
                t_old.append(_time(old))
                t_new.append(_time(new))
            wins = ("yes" if max(t_new) < min(t_old) else
                    "no" if min(t_new) > max(t_old) else "within spread")
            print(f"| {out} x {K} | {rows} | {nbytes / HBM_BPS * 1e6:5.1f} | "
                  f"{_fmt(t_old)} | "
                  f"{nbytes / statistics.median(t_old) / 1e3:5.0f} | "
                  f"{_fmt(t_new)} | "
                  f"{nbytes / statistics.median(t_new) / 1e3:5.0f} | {wins} | "
                  f"{diff:.4f} |", flush=True)
        del w


def decoder_step(w8):
    """4 layers of the Ziya-13B layer shape in GraphedDecoder, batch 8,
    max_len 2048: ms/token of the captured step with FENGSHEN_DECODE_GEMM=0
    and =1, a fresh decoder (and graph) per setting."""
    import torch
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    from fengshen_amd.serving.graphed_decode import GraphedDecoder
    from fengshen_amd.utils.quantize import quantize_model_int8
    torch.manual_seed(0)
    cfg = LlamaConfig(vocab_size=39424, hidden_size=5120,
                      num_hidden_layers=4, num_attention_heads=40,
                      intermediate_size=13824, max_position_embeddings=2048)
    model = LlamaForCausalLM(cfg).to(torch.bfloat16).cuda().eval()
    if w8:
        model = quantize_model_int8(model)
    ids = torch.randint(3, 39424, (8, 512), device="cuda")
    decs = {}
    for mode in ("0", "1"):
        os.environ["FENGSHEN_DECODE_GEMM"] = mode
        decs[mode] = GraphedDecoder(model, batch=8, max_len=2048,
                                    max_new_tokens=64)
        decs[mode].generate(ids, max_new_tokens=8)  # capture + warm-up
    times = {"0": [], "1": []}
    for _ in range(REPEATS):
        for mode, dec in decs.items():
            os.environ["FENGSHEN_DECODE_GEMM"] = mode  # the eager prefill
            dec._prefill(ids)
            times[mode].append(_time(dec._graph.replay, 48) / 1e3)
    for mode, ts in times.items():
        print(f"GraphedDecoder 4 layers, batch 8, "
              f"{'int8' if w8 else 'bf16'}, FENGSHEN_DECODE_GEMM={mode}: "
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
            sys.exit("decode_gemm_bench needs a GPU")
        name = STEPS[args.step]
        (decoder_step if name.startswith("decoder") else kernel_step)(
            name.endswith("int8"))
        return 0
    for step in range(len(STEPS) if args.decoder else 2):
        rc = subprocess.run([sys.executable, os.path.abspath(__file__),
                             "--step", str(step)],
                            timeout=STEP_TIMEOUT).returncode
        if rc != 0:
            print(f"step {STEPS[step]} failed with exit status {rc}; stopping")
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
