#!/usr/bin/env python3
"""Flagship benchmark: Ziya-LLaMA-13B causal-LM training step, bf16, native
ZeRO over RCCL, synthetic data, random-init weights (BASELINE.json metric:
"tokens/sec Ziya-LLaMA-13B ZeRO-3 @1/2/4/8 GPU", weak scaling).

Driver contract:
  python bench.py --gpus N --steps K --warmup W
(N>1 launched via torch.distributed.run, one rank per GPU over RCCL.)
W untimed warmup steps, then EXACTLY K timed steps bracketed by
barrier + torch.cuda.synchronize on both sides; time is MAX over ranks;
rank 0 prints ONE JSON line.
--dump-outputs DIR additionally saves the last timed step's loss and a
seeded sample of its logits as DIR/<name>.npy; inputs and weights are
seeded, so two builds can be compared output for output.  --full is where
secondary measurements belong; there are none today.
"""
import argparse
import json
import os
import time

# expandable segments avoid fragmentation OOM with selective activation
# checkpointing (large transient recompute allocations); must be set
# before the first allocation.
os.environ.setdefault("PYTORCH_HIP_ALLOC_CONF", "expandable_segments:True")

import torch


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", type=str, default="ziya-llama-13b",
                   choices=["ziya-llama-13b", "wenzhong-gpt2-3.5b",
                            "erlangshen-1.3b", "llama-tiny", "taiyi-sd"])
    p.add_argument("--image_size", type=int, default=512)
    # None -> per-model BASELINE config defaults (resolved below); the
    # driver's flagless invocation keeps the 13B b16 s2048 headline config
    p.add_argument("--seq_len", type=int, default=None)
    p.add_argument("--micro_batch", type=int, default=None)
    p.add_argument("--zero_stage", type=int, default=3)
    p.add_argument("--tensor_model_parallel_size", "--tp", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-5)
    p.add_argument("--ckpt_skip", type=int, default=-1,
                   help="selective act-ckpt: every k-th layer skips "
                        "recompute (0 = checkpoint all layers, -1 = auto "
                        "from free HBM after optimizer init)")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed "
                        "step's forward returned (loss, logits) to "
                        "DIR/<name>.npy as float32; large arrays are "
                        "reduced to a fixed seeded sample")
    p.add_argument("--full", action="store_true",
                   help="also run every secondary measurement; this "
                        "benchmark has none beyond the headline figure, so "
                        "a full run does the same work as a plain one")
    return p.parse_args()


# at most this many elements of each dumped array (4 MiB as float32)
_DUMP_MAX_ELEMS = 1 << 20


def sample_outputs(out) -> dict:
    """Tensors a caller of the model's forward receives, flattened to
    float32.  An array above _DUMP_MAX_ELEMS is reduced to the elements at
    a fixed seeded set of flat indices, so two builds sample the same
    positions."""
    kept = {}
    for name in ("loss", "logits", "prediction_logits",
                 "seq_relationship_logits"):
        t = getattr(out, name, None)
        if not torch.is_tensor(t):
            continue
        flat = t.detach().reshape(-1)
        if flat.numel() > _DUMP_MAX_ELEMS:
            g = torch.Generator(device="cpu").manual_seed(2024)
            idx = torch.randint(0, flat.numel(), (_DUMP_MAX_ELEMS,),
                                generator=g).sort().values
            flat = flat[idx.to(flat.device)]
        kept[name] = flat.float()
    return kept


def write_outputs(out_dir: str, kept: dict) -> None:
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    for name, t in kept.items():
        np.save(os.path.join(out_dir, f"{name}.npy"),
                t.cpu().numpy().astype(np.float32, copy=False))


_REPO = os.path.dirname(os.path.abspath(__file__))


def setup_tunableop(model: str, local_rank: int) -> str:
    """hipBLASLt GEMM algorithm selection via PyTorch TunableOp.

    Replay mode (default): load the committed per-model tuning cache from
    profiles/tunableop/<model>.csv so every hot GEMM shape runs its
    offline-selected fastest hipBLASLt solution.
    Tune mode (FENGSHEN_TUNE=1): search algorithms online and write the
    cache to gpurun_out/tunableop_<model>_<rank>.csv for committing.
    FENGSHEN_TUNABLEOP=0 disables both.
    """
    mode = "off"
    if os.environ.get("FENGSHEN_TUNABLEOP", "1") == "0" \
            or not torch.cuda.is_available():
        return mode
    import torch.cuda.tunable as tunable
    cache = os.path.join(_REPO, "profiles", "tunableop", f"{model}.csv")
    if os.environ.get("FENGSHEN_TUNE", "0") == "1":
        out_dir = os.path.join(_REPO, "gpurun_out")
        os.makedirs(out_dir, exist_ok=True)
        tunable.enable(True)
        tunable.tuning_enable(True)
        tunable.set_filename(
            os.path.join(out_dir, f"tunableop_{model}_{local_rank}.csv"))
        mode = "tune"
    elif os.path.exists(cache):
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.read_file(cache)
        mode = "replay"
    return mode


class _TaiyiSDTrainStep(torch.nn.Module):
    """Taiyi-SD-1B finetune step (BASELINE config 5): frozen VAE encode ->
    noise/timestep -> BERT text encode -> SD-1 UNet -> mse.  Trains UNet +
    text encoder (the bilingual stage-2 recipe)."""

    def __init__(self):
        super().__init__()
        from fengshen_amd.models.megatron_bert.configuration_megatron_bert \
            import bert_tiny_config
        from fengshen_amd.models.megatron_bert.modeling_megatron_bert \
            import MegatronBertModel
        from fengshen_amd.models.taiyi_sd import (
            AutoencoderKL, DDPMScheduler, UNet2DConditionModel)
        from fengshen_amd.models.taiyi_sd.unet import taiyi_sd_1b_config
        self.text_encoder = MegatronBertModel(
            bert_tiny_config(hidden_size=768, num_hidden_layers=12,
                             num_attention_heads=12,
                             intermediate_size=3072,
                             max_position_embeddings=512),
            add_pooling_layer=False)
        self.vae = AutoencoderKL()
        for p in self.vae.parameters():
            p.requires_grad = False
        self.unet = UNet2DConditionModel(taiyi_sd_1b_config())
        self.noise_scheduler = DDPMScheduler()

    class _Out:
        def __init__(self, loss):
            self.loss = loss

    @property
    def config(self):
        return self.unet.config

    def gradient_checkpointing_enable(self, **_kw):
        self.unet.gradient_checkpointing_enable()

    def forward(self, pixel_values, input_ids):
        with torch.no_grad():
            latents = self.vae.encode(pixel_values.to(
                self.unet.conv_in.weight.dtype))
        noise = torch.randn_like(latents)
        t = torch.randint(0, self.noise_scheduler.num_train_timesteps,
                          (latents.shape[0],), device=latents.device)
        noisy = self.noise_scheduler.add_noise(latents, noise, t)
        ctx = self.text_encoder(input_ids).last_hidden_state
        pred = self.unet(noisy, t, ctx)
        loss = torch.nn.functional.mse_loss(pred.float(), noise.float())
        return self._Out(loss)


def build_model(name: str, seq_len: int):
    if name == "taiyi-sd":
        m = _TaiyiSDTrainStep()
        return m, m.text_encoder.config.vocab_size, "Taiyi-SD-1B"
    if name == "ziya-llama-13b":
        from fengshen_amd.models.llama.configuration_llama import (
            ziya_llama_13b_config)
        from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
        cfg = ziya_llama_13b_config(max_position_embeddings=max(seq_len, 2048))
        return LlamaForCausalLM(cfg), cfg.vocab_size, "Ziya-LLaMA-13B"
    if name == "wenzhong-gpt2-3.5b":
        from fengshen_amd.models.gpt2.configuration_gpt2 import (
            wenzhong_gpt2_3b5_config)
        from fengshen_amd.models.gpt2.modeling_gpt2 import GPT2LMHeadModel
        cfg = wenzhong_gpt2_3b5_config(
            max_position_embeddings=max(seq_len, 1024))
        return GPT2LMHeadModel(cfg), cfg.vocab_size, "Wenzhong-GPT2-3.5B"
    if name == "erlangshen-1.3b":
        from fengshen_amd.models.megatron_bert.configuration_megatron_bert import (
            erlangshen_1b3_config)
        from fengshen_amd.models.megatron_bert.modeling_megatron_bert import (
            MegatronBertForPreTraining)
        # pos table must cover seq_len: out-of-range position ids fault
        # the embedding gather on-device
        cfg = erlangshen_1b3_config(
            max_position_embeddings=max(seq_len, 512))
        return MegatronBertForPreTraining(cfg), cfg.vocab_size, \
            "Erlangshen-MegatronBert-1.3B"
    from fengshen_amd.models.llama.configuration_llama import LlamaConfig
    from fengshen_amd.models.llama.modeling_llama import LlamaForCausalLM
    cfg = LlamaConfig(vocab_size=2048, hidden_size=512, num_hidden_layers=4,
                      num_attention_heads=8, intermediate_size=1408,
                      max_position_embeddings=max(seq_len, 512))
    return LlamaForCausalLM(cfg), cfg.vocab_size, "llama-tiny"


# (micro_batch, seq_len) of each model's BASELINE.json config
_MODEL_DEFAULTS = {"ziya-llama-13b": (16, 2048),
                   "wenzhong-gpt2-3.5b": (16, 1024),
                   "erlangshen-1.3b": (128, 512),
                   "taiyi-sd": (16, 77),
                   "llama-tiny": (4, 256)}


def main():
    args = parse_args()
    d_mb, d_sl = _MODEL_DEFAULTS[args.model]
    if args.micro_batch is None:
        args.micro_batch = d_mb
    if args.seq_len is None:
        args.seq_len = d_sl
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # FENGSHEN_BENCH_CPU=1: gloo/CPU smoke of the multi-rank path only —
    # numbers from this mode are NOT benchmark results.
    cpu_smoke = os.environ.get("FENGSHEN_BENCH_CPU") == "1"
    if cpu_smoke:
        device = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench.py requires a GPU"
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)

    import torch.distributed as dist
    from fengshen_amd.parallel.groups import init_distributed
    from fengshen_amd.parallel.zero import ZeroOptimizer
    if not cpu_smoke:
        from fengshen_amd.ops import has_ext
        assert has_ext(), \
            "HIP extension must be built (python -m fengshen_amd.ops.build)"

    tunable_mode = setup_tunableop(args.model, local_rank)

    if world > 1 or args.tensor_model_parallel_size > 1:
        init_distributed(backend="gloo" if cpu_smoke else "nccl")
    if args.tensor_model_parallel_size > 1:
        from fengshen_amd.parallel.groups import initialize_model_parallel
        initialize_model_parallel(args.tensor_model_parallel_size)

    torch.manual_seed(1234)
    # construct directly on the GPU in bf16: 8 ranks x fp32-on-CPU would
    # exhaust host RAM for 13B, and GPU-side init is much faster
    # cpu_smoke stays fp32 (CPU group_norm/conv kernels lack bf16 paths)
    bench_dtype = torch.float32 if cpu_smoke else torch.bfloat16
    torch.set_default_dtype(bench_dtype)
    with device:
        model, vocab, model_name = build_model(args.model, args.seq_len)
    torch.set_default_dtype(torch.float32)
    model = model.to(bench_dtype).to(device)
    if hasattr(model, "gradient_checkpointing_enable") \
            and args.model != "taiyi-sd":
        try:
            model.gradient_checkpointing_enable(
                skip_interval=max(args.ckpt_skip, 0))
        except TypeError:
            model.gradient_checkpointing_enable()
    model.train()
    n_params = sum(p.numel() for p in model.parameters())

    if args.zero_stage == 3:
        from fengshen_amd.parallel.zero3 import Zero3Engine
        opt = Zero3Engine(model, lr=args.lr, betas=(0.9, 0.95), eps=1e-8,
                          weight_decay=0.1)
    else:
        opt = ZeroOptimizer(model.parameters(), stage=args.zero_stage,
                            lr=args.lr, betas=(0.9, 0.95), eps=1e-8,
                            weight_decay=0.1)

    from fengshen_amd.parallel import groups as pgroups
    dp_rank = pgroups.get_data_parallel_rank()
    dp_world = pgroups.get_data_parallel_world_size()

    # Selective activation checkpointing: spend spare HBM3E to skip
    # recompute on every k-th layer (measured +5.4% at skip=4 on 1 GPU;
    # with dp-sharded optimizer states at N=8 far more memory is free, so
    # size k from what is actually available AFTER optimizer-state alloc).
    # kept-activation bytes per non-recomputed layer, in units of
    # hidden * b * s * 2 (bf16): ~21.2 for SwiGLU llama, ~21 gpt2, ~19 bert
    _ACT_MULT = {"ziya-llama-13b": 21.2, "llama-tiny": 21.2,
                 "wenzhong-gpt2-3.5b": 21.0, "erlangshen-1.3b": 19.0}
    skip = max(args.ckpt_skip, 0)
    if args.model == "taiyi-sd":
        skip = 0  # conv UNet at 512^2 fits 288 GB HBM without recompute
    elif args.ckpt_skip < 0 and torch.cuda.is_available():
        free_b, _total = torch.cuda.mem_get_info()
        L = model.config.num_hidden_layers
        act = _ACT_MULT[args.model] * model.config.hidden_size \
            * args.micro_batch * args.seq_len * 2
        n_store = int(free_b * 0.8 / act)
        if n_store >= L:
            skip = 1          # store everything: no recompute at all
        elif n_store >= 2:
            skip = max(2, -(-L // n_store))
        else:
            skip = 0
        if skip > 1 and args.model == "ziya-llama-13b" \
                and pgroups.get_data_parallel_world_size() == 1:
            skip = max(skip, 4)  # skip<4 validated OOM at 13B dp1
    if skip:
        try:
            model.gradient_checkpointing_enable(skip_interval=skip)
        except TypeError:
            skip = 0

    is_bert = args.model == "erlangshen-1.3b"
    is_sd = args.model == "taiyi-sd"
    b, s = args.micro_batch, args.seq_len
    if is_sd:
        s = 77  # CLIP-style caption length
    # TP ranks must see identical batches: seed by DP rank
    g = torch.Generator(device="cpu").manual_seed(42 + dp_rank)
    # one fresh synthetic batch per step (a fixed 4-batch cycle lets a 13B
    # memorize them and prints a meaningless ~0 loss)
    batches = []
    for _ in range(args.warmup + args.steps):
        ids = torch.randint(3, vocab, (b, s), generator=g).to(device)
        if is_sd:
            px = torch.randn(b, 3, args.image_size, args.image_size,
                             generator=g).to(device)
            batches.append(dict(pixel_values=px, input_ids=ids))
        elif is_bert:
            labels = ids.clone()
            mask_pos = torch.rand(b, s, generator=g) < 0.15
            labels[~mask_pos.to(device)] = -100
            sop = torch.randint(0, 2, (b,), generator=g).to(device)
            batches.append(dict(input_ids=ids, labels=labels,
                                next_sentence_label=sop,
                                attention_mask=torch.ones_like(ids)))
        else:
            batches.append(dict(input_ids=ids, labels=ids))

    step_idx = [0]
    dumped = {}

    def step(keep=False):
        batch = batches[step_idx[0] % len(batches)]
        step_idx[0] += 1
        out = model(**batch)
        if keep:
            # sampled before backward frees the logits; stays on the device
            # so the timed region gains no host synchronisation
            dumped.update(sample_outputs(out))
        opt.zero_grad()
        out.loss.backward()
        opt.step()
        return out.loss

    # Warmup doubles as an OOM self-check for the auto ckpt-skip estimate:
    # the heuristic can overshoot on topologies we could not measure
    # (e.g. dp8 shards optimizer state 8x, freeing HBM the activation
    # model then over-claims).  Warmup steps are untimed, so on OOM we
    # tighten the skip and retry instead of failing the whole run.
    warm_left = args.warmup
    while warm_left > 0:
        try:
            loss = step()
            warm_left -= 1
        except torch.OutOfMemoryError:
            # skip semantics: 0 = checkpoint all (min memory), 1 = store
            # all (max memory), k>=2 = store every k-th layer
            if args.ckpt_skip >= 0 or skip == 0:
                raise  # user-pinned or already at minimum memory
            skip = 2 if skip == 1 else (
                skip + 1 if skip < model.config.num_hidden_layers else 0)
            opt.zero_grad()
            torch.cuda.empty_cache()
            model.gradient_checkpointing_enable(skip_interval=skip)
            if rank == 0:
                print(f"[bench] OOM in warmup; ckpt_skip -> {skip}",
                      flush=True)

    if world > 1:
        dist.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = step(keep=args.dump_outputs is not None
                    and i == args.steps - 1)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    elapsed = time.perf_counter() - t0

    # MAX over ranks
    if world > 1:
        t = torch.tensor([elapsed], device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = t.item()

    tokens_per_step = b * s * dp_world
    samples_per_step = b * dp_world
    value = (samples_per_step if (is_bert or is_sd) else tokens_per_step) \
        * args.steps / elapsed
    ms_per_step = elapsed / args.steps * 1000.0

    # model-FLOPs utilisation (PaLM convention: no recompute counted):
    # 6*N per token dense + 12*L*h*s^2*b attention (fwd 4bs^2h + bwd 8bs^2h)
    # n_params was captured before ZeRO-3 sharded the param storage.
    L = getattr(model.config, "num_hidden_layers", 0)
    h = getattr(model.config, "hidden_size", 0)
    flops_step = 6.0 * n_params * b * s + 12.0 * L * h * s * s * b
    tflops_per_gpu = flops_step * args.steps / elapsed / 1e12
    mfu = tflops_per_gpu / 2500.0  # MI355X dense bf16 peak ~2.5 PF/s
    if is_sd:  # token-based MFU formula does not apply to the conv UNet
        tflops_per_gpu, mfu = None, None

    if rank == 0 and args.dump_outputs is not None:
        write_outputs(args.dump_outputs, dumped)

    if rank == 0:
        print(json.dumps({
            "metric": ("samples/sec/node pretrain Erlangshen-1.3B"
                       if is_bert
                       else "samples/sec Taiyi-SD-1B 512x512 finetune"
                       if is_sd
                       else f"tokens/sec Ziya-LLaMA-13B ZeRO-{args.zero_stage}"
                       if args.model == "ziya-llama-13b"
                       else f"tokens/sec {model_name}"),
            "value": round(value, 2),
            "unit": "samples/s" if (is_bert or is_sd) else "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "loss": round(float(loss.item()), 4),
            "tflops_per_gpu": (round(tflops_per_gpu, 1)
                               if tflops_per_gpu is not None else None),
            "mfu": round(mfu, 4) if mfu is not None else None,
            "tunableop": tunable_mode,
            "config": {
                "model": model_name,
                "global_batch": b * world,
                "micro_batch": b,
                "seq_len": s,
                **({"image_size": args.image_size} if is_sd else {}),
                "parallelism": (
                    f"zero{args.zero_stage}_dp{dp_world}"
                    + (f"_tp{args.tensor_model_parallel_size}"
                       if args.tensor_model_parallel_size > 1 else "")),
                "activation_checkpointing": True,
                "ckpt_skip_interval": skip,
            },
        }), flush=True)

    if tunable_mode == "tune":
        import torch.cuda.tunable as tunable
        tunable.write_file()

    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
