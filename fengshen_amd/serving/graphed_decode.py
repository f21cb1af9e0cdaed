"""hipGraph-captured decode for LLaMA serving (greedy or sampled).

Eager decode of a 13B model launches ~400 kernels per token (40 layers x
~10 ops); at ~8 us a launch that is several ms of pure launch overhead on
a path that is otherwise weight-bandwidth-bound.  This engine captures ONE
self-advancing decode step into a hipGraph (torch.cuda.CUDAGraph is
hipGraph on ROCm) and replays it per token:

- static KV cache [b, kv_heads, max_len, hd] per layer (kv_heads <
  heads under grouped-query attention), position driven by a
  device tensor (no host sync anywhere in the loop);
- inside the graph the hot path is hand-written HIP (kernels.hip):
  bf16_gemv (weights streamed at 5.7-6.8 TB/s vs hipBLASLt's ~2.5-3 at
  M=1), decode_attn (rope + cache write + online-softmax attention in one
  launch per layer) and add_rms_norm (residual add fused into the norm);
  eager torch fallback when the extension/dtype/head-dim doesn't fit;
- decode_attn_split (decode_attn.hip) is the second attention kernel: the
  key prefix is split over blocks, a block serves the query heads of one KV
  head together, and every sequence has its own position.  It serves head
  dim 96 and ragged prompt batches (generate(..., prompt_lens=...)), which
  decode_attn cannot, and long windows; FENGSHEN_DECODE_SPLIT = auto | 0 | 1
  picks between the two (see _SPLIT_MIN_LEN);
- with a batch of 2..16 the projections and the LM head can run decode_gemm
  (decode_gemm.hip), an MFMA kernel that streams the weights once and gets
  the reuse of x across the batch from the matrix instruction;
  FENGSHEN_DECODE_GEMM = auto | 0 | 1, read per call by
  ops.functional.decode_linear_route.  auto takes it for int8 weights
  (W8Linear) from 4 rows, where it replaces w8_gemv, whose cost grows with
  the batch; bf16 weights keep hipBLASLt, which measured faster;
- int4 weights (W4Linear, utils.quantize.quantize_model_int4) run
  decode_gemm_w4 (decode_gemm_w4.hip) for any batch of 1..16: a split-K
  MFMA kernel that stages x in LDS once per block and streams 4-bit
  weights with a bf16 scale per 128 input features; its partial-sum buffer
  comes from the stream's allocator, so the step captures like the others;
- kv_cache="int8" keeps K and V as int8 with one fp32 scale per cached row
  (k_scale / v_scale [b, kv_heads, max_len]) and runs decode_attn_split_q8
  (decode_attn_q8.hip), the split kernel reading half the bytes; prefill
  quantises its K/V with kv_quantize_int8, each step quantises its own row
  and attends to the quantised values.  Head dim 64 or 128, max_len a
  multiple of 4, the split kernel only; anything else raises ValueError,
  there is no fallback to a bf16 cache.  Per-row scales do not isolate the
  per-channel outliers K has in real models;
- lookahead=T (2..16) makes the captured step a T-token verify step of
  greedy lookahead decoding: the last accepted token and T-1 drafts go
  through the layers as [b, T, H] rows, attention is one
  decode_attn_split(..., tokens=T) launch per layer (decode_attn_mt.hip,
  the T tokens share one pass over the cache), and the longest prefix of
  drafts that equals the model's own argmax is accepted, so a replay emits
  1..T tokens per sequence and the output is the greedy output.  Drafts are
  a bigram lookup over the sequence's own tokens (generate(hint_ids=...)
  puts a guess of the continuation in front of them); no draft model.
  bf16 cache, greedy and the split kernel only;
- greedy argmax — or gumbel-max top-k/top-p sampling over a pre-generated
  seeded noise buffer indexed by the step tensor — feeds the token buffer
  consumed by the NEXT replay, so a whole max_new_tokens decode is just N
  graph replays with zero host round-trips.

Measured (13B, 1x MI355X): 5.92 ms/token bf16, 5.06 int8, 0.99
ms/seq/token at batch 8 (profiles/decode_kernels_r2.md).

Ref context: examples/ziya_inference (the reference's only throughput
table) and PERF_ROADMAP item 5 (hipGraph capture of the decode loop).
"""
from __future__ import annotations

import math
from typing import Optional

import torch

from fengshen_amd.ops import functional as F_ops


def filter_logits(logits: torch.Tensor, temperature: torch.Tensor,
                  top_k: int, top_p: torch.Tensor) -> torch.Tensor:
    """HF-convention sampling filter, graph-safe (static shapes only).

    temperature / top_p are device scalars so they can be retuned between
    generates without recapturing; top_k is shape-affecting and fixed at
    capture.  Order matches the reference's sample_sequence helpers
    (fengshen/utils/transfo_xl_utils.py top_k_logits): temperature, then
    top-k, then nucleus.
    """
    # NOTE: no torch.tensor(..., device=...) here — an H2D copy is
    # hipErrorStreamCaptureUnsupported inside graph capture; masked_fill
    # with a python scalar lowers to a capture-safe fill kernel.
    lg = logits.float() / temperature
    if top_k > 0:
        kth = lg.topk(top_k, dim=-1).values[..., -1:]
        lg = lg.masked_fill(lg < kth, float("-inf"))
    # nucleus: drop tokens once the cumulative prob BEFORE them >= top_p
    # (the top-1 token always survives).  top_p >= 1 keeps everything.
    srt, idx = lg.sort(dim=-1, descending=True)
    probs = torch.softmax(srt, dim=-1)
    shifted_cum = probs.cumsum(dim=-1) - probs
    srt = srt.masked_fill(shifted_cum >= top_p, float("-inf"))
    return torch.full_like(lg, float("-inf")).scatter(-1, idx, srt)


# FENGSHEN_DECODE_SPLIT=auto: windows of at least this many positions run
# decode_attn_split, shorter ones decode_attn.  At b1 h40 d128 the split
# kernel wins from the smallest measured window, 512 (docs/KERNELS.md,
# "split-KV decode"); the constant is never set below 513, so a decoder
# with the default max_len = 512 keeps decode_attn.
_SPLIT_MIN_LEN = 513


class GraphedDecoder:
    def __init__(self, model, batch: int = 1, max_len: int = 512,
                 max_new_tokens: int = 256, do_sample: bool = False,
                 top_k: int = 0, top_p: float = 1.0,
                 temperature: float = 1.0, kv_cache: str = "bf16",
                 lookahead: int = 1):
        if kv_cache not in ("bf16", "int8"):
            raise ValueError(
                f"kv_cache must be 'bf16' or 'int8', got {kv_cache!r}")
        self.kv_cache = kv_cache
        self.model = model.eval()
        cfg = model.config
        dev = next(model.parameters()).device
        dt = next(model.parameters()).dtype
        self.dev, self.dt = dev, dt
        self.batch = batch
        self.max_len = max_len
        self.max_new = max_new_tokens
        L = cfg.num_hidden_layers
        nh = cfg.num_attention_heads
        hd = cfg.hidden_size // nh
        # grouped-query attention: the caches hold the KV heads only
        nkv = getattr(cfg, "num_key_value_heads", None) or nh
        self.nh, self.nkv, self.hd = nh, nkv, hd
        self.scale = 1.0 / math.sqrt(hd)

        # static state; kv_cache="int8": int8 rows and one fp32 scale per row
        cdt = torch.int8 if kv_cache == "int8" else dt
        self.k_cache = [torch.zeros(batch, nkv, max_len, hd, device=dev,
                                    dtype=cdt) for _ in range(L)]
        self.v_cache = [torch.zeros(batch, nkv, max_len, hd, device=dev,
                                    dtype=cdt) for _ in range(L)]
        if kv_cache == "int8":
            self.k_scale = [torch.zeros(batch, nkv, max_len, device=dev)
                            for _ in range(L)]
            self.v_scale = [torch.zeros(batch, nkv, max_len, device=dev)
                            for _ in range(L)]
        if not 1 <= lookahead <= 16:
            raise ValueError(f"lookahead must be in [1, 16], got {lookahead}")
        self.lookahead = lookahead
        self.last_replays = 0  # graph replays of the last generate()
        # the last accepted token, then lookahead - 1 drafts
        self.tok = torch.zeros(batch, lookahead, device=dev,
                               dtype=torch.long)
        # one position per sequence; decode_attn and the eager step share
        # one position and read the [1] view self.pos[:1]
        self.pos = torch.zeros(batch, device=dev, dtype=torch.long)
        self.step_i = torch.zeros(1, device=dev, dtype=torch.long)
        # a lookahead step writes all its T predictions at the row's count
        self.out_tokens = torch.zeros(
            batch, max_new_tokens + (lookahead if lookahead > 1 else 0),
            device=dev, dtype=torch.long)
        if lookahead > 1:
            # tokens emitted per sequence; the draft corpus of a row is
            # [hint | prompt | accepted tokens], sequence position p at
            # column hint_n + p, so it ends at column hint_n + pos
            self.count = torch.zeros(batch, device=dev, dtype=torch.long)
            self.corpus = torch.zeros(batch, 2 * max_len, device=dev,
                                      dtype=torch.long)
            self.hint_n = torch.zeros(1, device=dev, dtype=torch.long)
            self.ar_t = torch.arange(lookahead, device=dev)
            self.ar_c = torch.arange(2 * max_len, device=dev)
        self.ar = torch.arange(max_len, device=dev)
        cos, sin = F_ops.build_rope_cache(
            max_len, hd, base=getattr(cfg, "rotary_emb_base",
                                      getattr(cfg, "rope_base", 10000.0)))
        self.cos = cos.to(dev)
        self.sin = sin.to(dev)
        # sampling state: gumbel-max with a pre-generated noise buffer
        # indexed by step_i — no RNG state inside the graph, and a fixed
        # torch seed gives reproducible samples.
        self.do_sample = do_sample
        self.top_k = top_k
        self.top_p = torch.tensor(float(top_p), device=dev)
        self.temperature = torch.tensor(float(temperature), device=dev)
        if do_sample:
            self.gumbel = torch.zeros(max_new_tokens, batch,
                                      cfg.vocab_size, device=dev)
        # fused rope+cache+attention kernel (one launch per layer instead
        # of ~10 eager ops); requires bf16 and head dim 64/128 (decode_attn)
        # or 64/96/128 (decode_attn_split)
        from fengshen_amd.ops import get_ext
        import os
        self._ext = get_ext() if dev.type == "cuda" else None
        self._split_mode = os.environ.get("FENGSHEN_DECODE_SPLIT", "auto")
        if self._split_mode not in ("auto", "0", "1"):
            raise ValueError("FENGSHEN_DECODE_SPLIT must be auto, 0 or 1, "
                             f"got {self._split_mode!r}")
        self._use_split = self._split_mode == "1" or (
            self._split_mode == "auto"
            and (hd == 96 or max_len >= _SPLIT_MIN_LEN))
        self._fused_attn = (
            self._ext is not None
            and (hd in (64, 128) or (hd == 96 and self._use_split))
            and dt == torch.bfloat16
            and os.environ.get("FENGSHEN_AMD_FORCE_EAGER") != "1"
            and os.environ.get("FENGSHEN_DECODE_FUSED", "1") == "1")
        if kv_cache == "int8":
            if not self._fused_attn or self._split_mode == "0":
                raise ValueError(
                    "kv_cache='int8' needs the fused decode_attn_split_q8 "
                    "kernel: a GPU, bf16 weights, the HIP extension, "
                    "FENGSHEN_DECODE_FUSED not 0 and FENGSHEN_DECODE_SPLIT "
                    "not 0")
            if hd not in (64, 128) or max_len % 4:
                raise ValueError(
                    "kv_cache='int8' serves head dim 64 or 128 and a max_len "
                    f"that is a multiple of 4, got {hd} and {max_len}")
            self._use_split = True
        if lookahead > 1:
            if not self._fused_attn or self._split_mode == "0":
                raise ValueError(
                    "lookahead > 1 needs the fused decode_attn_split kernel: "
                    "a GPU, bf16 weights, head dim 64/96/128, the HIP "
                    "extension, FENGSHEN_DECODE_FUSED not 0 and "
                    "FENGSHEN_DECODE_SPLIT not 0")
            if kv_cache != "bf16":
                raise ValueError("lookahead > 1 needs kv_cache='bf16': the "
                                 "multi-token kernel reads bf16 caches only")
            if do_sample:
                raise ValueError("lookahead > 1 needs do_sample=False: "
                                 "drafts are verified against the argmax")
            self._use_split = True  # forced, as ragged prompts force it
        self._graph: Optional[torch.cuda.CUDAGraph] = None

    @property
    def supports_ragged(self) -> bool:
        """Whether generate(..., prompt_lens=...) can run: it needs the
        decode_attn_split kernel (per-sequence positions)."""
        return self._fused_attn and self._split_mode != "0"

    # ------------------------------------------------------------------
    @staticmethod
    def _rot_half(x):
        x1, x2 = x.chunk(2, dim=-1)
        return torch.cat((-x2, x1), dim=-1)

    def _add_norm(self, a, b_, norm):
        """(a + b_, norm(a + b_)) — fused into one kernel when norm is an
        RMSNorm on the HIP path (the 13B decode graph has 81 such pairs
        per token)."""
        if self._fused_attn and type(norm).__name__ == "RMSNorm":
            s, y = self._ext.add_rms_norm(a.contiguous(), b_.contiguous(),
                                          norm.weight, norm.eps)
            return s.view_as(a), y.view_as(a)
        s = a + b_
        return s, norm(s)

    def _step(self):
        """Graph-safe decode step; advances tok/pos/step_i (lookahead > 1:
        tok/pos/count by the tokens it accepted)."""
        m = self.model.model
        b, nh, nkv, hd = self.batch, self.nh, self.nkv, self.hd
        T = self.lookahead
        # per-sequence positions for decode_attn_split, else the shared one
        split = self._fused_attn and self._use_split
        pos = self.pos if split else self.pos[:1]
        attn = (self._ext.decode_attn_split if split
                else self._ext.decode_attn) if self._fused_attn else None
        h = m.embed_tokens(self.tok)  # [b, T, H]
        if not self._fused_attn:
            c = self.cos.index_select(0, pos).to(self.dt)  # [1, hd]
            s = self.sin.index_select(0, pos).to(self.dt)
            # additive mask over the static window: visible iff idx <= pos
            amask = torch.where(self.ar <= pos,
                                torch.zeros((), device=self.dev),
                                torch.full((), float("-inf"),
                                           device=self.dev))
        if self._fused_attn:
            # residual adds ride the next norm's kernel (add_rms_norm),
            # including across layer boundaries and into the final norm
            pend = None  # (residual, branch) awaiting add+norm
            for i, layer in enumerate(m.layers):
                if pend is None:
                    x = layer.input_norm(h)
                else:
                    h, x = self._add_norm(pend[0], pend[1],
                                          layer.input_norm)
                qkv = layer.attention.qkv_proj(x)
                if isinstance(qkv, tuple):
                    qkv = qkv[0]
                if self.kv_cache == "int8":
                    ctx = self._ext.decode_attn_split_q8(
                        qkv.view(b, (nh + 2 * nkv) * hd), self.k_cache[i],
                        self.k_scale[i], self.v_cache[i], self.v_scale[i],
                        self.cos, self.sin, pos, self.scale,
                        bool(layer.attention.rotary))
                elif T > 1:
                    ctx = attn(
                        qkv.view(b, T, (nh + 2 * nkv) * hd), self.k_cache[i],
                        self.v_cache[i], self.cos, self.sin, pos,
                        self.scale, bool(layer.attention.rotary), tokens=T)
                else:
                    ctx = attn(
                        qkv.view(b, (nh + 2 * nkv) * hd), self.k_cache[i],
                        self.v_cache[i], self.cos, self.sin, pos,
                        self.scale, bool(layer.attention.rotary))
                out = layer.attention.out_proj(ctx.view(b, T, nh * hd))
                if isinstance(out, tuple):
                    out = out[0]
                h, x = self._add_norm(h, out, layer.post_attention_norm)
                mlp = layer.mlp(x)
                if isinstance(mlp, tuple):
                    mlp = mlp[0]
                pend = (h, mlp)
            _, h = self._add_norm(pend[0], pend[1], m.norm)
            if T > 1:
                self._emit_lookahead(h)
            else:
                self._emit(h)
            return
        for i, layer in enumerate(m.layers):
            res = h
            x = layer.input_norm(h)
            qkv = layer.attention.qkv_proj(x)
            if isinstance(qkv, tuple):
                qkv = qkv[0]
            q, k, v = qkv.split([nh * hd, nkv * hd, nkv * hd], dim=-1)
            q = q.view(b, 1, nh, hd).transpose(1, 2)  # [b, nh, 1, hd]
            k = k.view(b, 1, nkv, hd).transpose(1, 2)
            v = v.view(b, 1, nkv, hd).transpose(1, 2)
            if layer.attention.rotary:
                q = q * c + self._rot_half(q) * s
                k = k * c + self._rot_half(k) * s
            self.k_cache[i].index_copy_(2, pos, k)
            self.v_cache[i].index_copy_(2, pos, v)
            kfull, vfull = self.k_cache[i], self.v_cache[i]
            if nkv != nh:  # eager fallback: expand the cache to nh heads
                from fengshen_amd.ops.flash import expand_kv
                kfull, vfull = expand_kv(kfull, nh), expand_kv(vfull, nh)
            scores = (q.float() @
                      kfull.float().transpose(-1, -2)) * self.scale
            probs = torch.softmax(scores + amask, dim=-1)
            ctx = (probs.to(self.dt) @ vfull)  # [b, nh, 1, hd]
            ctx = ctx.transpose(1, 2).reshape(b, 1, nh * hd)
            out = layer.attention.out_proj(ctx)
            if isinstance(out, tuple):
                out = out[0]
            h = res + out
            res = h
            x = layer.post_attention_norm(h)
            mlp = layer.mlp(x)
            if isinstance(mlp, tuple):
                mlp = mlp[0]
            h = res + mlp
        h = m.norm(h)
        self._emit(h)

    def _emit(self, h):
        """lm_head -> pick -> record token and advance pos/step_i."""
        logits = self.model.lm_head(h)
        if isinstance(logits, tuple):
            logits = logits[0]
        nxt = self._pick(logits[:, -1, :], self.step_i)  # [b, 1]
        self.out_tokens.index_copy_(1, self.step_i, nxt)
        self.tok.copy_(nxt)
        self.pos.add_(1)
        self.step_i.add_(1)

    def _draft(self):
        """tok[:, 1:] = the T - 1 tokens that followed the most recent earlier
        occurrence of the row's last two tokens in its corpus, or token 0
        where there is none.  Torch ops on static shapes: graph-safe."""
        end = (self.hint_n + self.pos)[:, None]  # column of the last token
        last = self.corpus.gather(1, torch.cat([end - 1, end], 1))
        hit = ((self.corpus == last[:, 1:])
               & (self.corpus.roll(1, 1) == last[:, :1])
               & (self.ar_c >= 1) & (self.ar_c < end))
        at = (hit * self.ar_c).amax(1, keepdim=True)  # 0: no occurrence
        # columns past the end hold junk of earlier steps; as drafts they
        # are merely wrong
        nxt = self.corpus.gather(
            1, (at + self.ar_t[1:]).clamp(max=self.corpus.shape[1] - 1))
        self.tok[:, 1:] = nxt * (at > 0)

    def _emit_lookahead(self, h):
        """lm_head over the T rows -> accept the longest prefix of drafts
        that equals the predictions -> record n_acc + 1 tokens per sequence,
        advance pos/count by as many, draft for the next step."""
        T = self.lookahead
        logits = self.model.lm_head(h)
        if isinstance(logits, tuple):
            logits = logits[0]
        pred = logits.argmax(dim=-1)  # [b, T]: the token after tok[:, t]
        ok = (self.tok[:, 1:] == pred[:, :-1]).long().cumprod(1).sum(1)
        # never past max_new tokens: keeps pos inside the window while the
        # other sequences finish
        adv = torch.minimum(ok + 1, self.max_new - self.count)
        # all T predictions go out; those past adv lie at and above the new
        # count / corpus end and the next step overwrites them
        self.out_tokens.scatter_(1, self.count[:, None] + self.ar_t, pred)
        self.corpus.scatter_(
            1, (self.hint_n + self.pos + 1)[:, None] + self.ar_t, pred)
        self.tok[:, :1] = pred.gather(1, (adv - 1).clamp(min=0)[:, None])
        self.pos.add_(adv)
        self.count.add_(adv)
        self._draft()

    def _pick(self, last_logits: torch.Tensor,
              step: torch.Tensor) -> torch.Tensor:
        """Greedy argmax, or gumbel-max sample over the filtered logits.
        `step` indexes the pre-generated noise buffer; graph-safe."""
        if not self.do_sample:
            return last_logits.argmax(dim=-1, keepdim=True)
        lg = filter_logits(last_logits, self.temperature,
                           self.top_k, self.top_p)
        # clamp: warmup/capture advance step_i past the real range
        g = self.gumbel.index_select(
            0, step.clamp(max=self.max_new - 1)).squeeze(0)  # [b, vocab]
        return (lg + g).argmax(dim=-1, keepdim=True)

    # ------------------------------------------------------------------
    @torch.no_grad()
    def _prefill(self, prompt_ids: torch.Tensor,
                 prompt_lens: Optional[torch.Tensor] = None):
        """Eager prefill through the model's normal cache path, then copy
        the per-layer K/V into the static buffers.  With prompt_lens the
        prompts are right-padded: under the causal mask a real token never
        sees a pad, the cache rows at and above a row's length hold pad
        junk, and decode_attn_split never reads rows above its position."""
        from transformers.cache_utils import DynamicCache
        assert prompt_ids.shape[0] == self.batch, (
            f"decoder captured for batch {self.batch}, "
            f"got {prompt_ids.shape[0]}")
        plen = prompt_ids.shape[1]
        assert plen + self.max_new <= self.max_len, "window too small"
        if prompt_lens is not None:
            prompt_lens = prompt_lens.to(self.dev, torch.long).view(-1)
            assert prompt_lens.numel() == self.batch, "one length per prompt"
            assert int(prompt_lens.min()) >= 1 and \
                int(prompt_lens.max()) <= plen, "prompt_lens outside [1, plen]"
        cache = DynamicCache()
        out = self.model(input_ids=prompt_ids.to(self.dev),
                         past_key_values=cache, use_cache=True)
        for i in range(len(self.k_cache)):
            layer_cache = cache.layers[i]  # transformers >= 5 DynamicCache
            k, v = layer_cache.keys, layer_cache.values
            if self.kv_cache == "int8":
                self._fill_int8(i, k, v, prompt_lens)
                continue
            self.k_cache[i][:, :, :plen].copy_(k)
            self.v_cache[i][:, :, :plen].copy_(v)
            self.k_cache[i][:, :, plen:].zero_()
            self.v_cache[i][:, :, plen:].zero_()
        self.step_i.zero_()
        if prompt_lens is None:
            self.pos.fill_(plen)
            last = out.logits[:, -1, :]
        else:
            self.pos.copy_(prompt_lens)
            last = out.logits[torch.arange(self.batch, device=self.dev),
                              prompt_lens - 1]
        self.tok.copy_(self._pick(last, self.step_i))

    def _fill_int8(self, i, k, v, prompt_lens):
        """Quantise the prefilled K/V [b, nkv, plen, hd] of layer i into the
        int8 cache; rows at and above a sequence's prompt length get zero
        int8 and zero scale."""
        plen = k.shape[2]
        lens = (prompt_lens if prompt_lens is not None
                else self.pos.new_full((self.batch,), plen))
        keep = (self.ar[:plen] < lens[:, None])[:, None]  # [b, 1, plen]
        for x, cache, scale in ((k, self.k_cache[i], self.k_scale[i]),
                                (v, self.v_cache[i], self.v_scale[i])):
            q, s = self._ext.kv_quantize_int8(x.contiguous())
            cache.zero_()
            scale.zero_()
            cache[:, :, :plen].copy_(q * keep[..., None])
            scale[:, :, :plen].copy_(s * keep)

    def _capture(self):
        # warm up twice on a side stream (allocator + kernels), then capture
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            for _ in range(2):
                self._step()
        torch.cuda.current_stream().wait_stream(st)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        self._graph = g

    # ------------------------------------------------------------------
    @torch.no_grad()
    def generate(self, prompt_ids: torch.Tensor,
                 max_new_tokens: Optional[int] = None,
                 eos_token_id: Optional[int] = None,
                 prompt_lens: Optional[torch.Tensor] = None,
                 hint_ids: Optional[torch.Tensor] = None):
        """Greedy (or sampled) decode via graph replays.

        Without prompt_lens all prompts have the length of prompt_ids and
        the result is a tensor [b, plen + n]: prompt, then n new tokens.

        With prompt_lens (int [b]) the prompts are right-padded to plen and
        row i holds prompt_lens[i] real tokens.  The result is then a list
        of b 1-D tensors, row i being its prompt_lens[i] prompt tokens
        followed by its n new tokens, with no padding in between.  This
        needs the decode_attn_split kernel (per-sequence positions).

        With lookahead > 1 a replay emits 1..lookahead tokens per sequence
        and the call replays until every sequence has its n tokens
        (last_replays says how often); the result is the same.  hint_ids
        [b, n_hint] (n_hint <= max_len) is a guess of the continuation, a
        previous answer or the text being edited: it only seeds the draft
        lookup and cannot change the result."""
        n = min(max_new_tokens or self.max_new, self.max_new)
        if hint_ids is not None and self.lookahead == 1:
            raise ValueError("hint_ids needs lookahead > 1")
        if self.lookahead > 1:
            return self._generate_lookahead(prompt_ids, n, eos_token_id,
                                            prompt_lens, hint_ids)
        if prompt_lens is not None:
            prompt_lens = torch.as_tensor(prompt_lens)
        if prompt_lens is not None and not (self._fused_attn
                                            and self._use_split):
            if not self.supports_ragged:
                raise RuntimeError(
                    "prompt_lens (prompts of unequal length) needs the fused "
                    "decode_attn_split kernel: bf16 weights, head dim "
                    "64/96/128, the HIP extension and FENGSHEN_DECODE_SPLIT "
                    "not 0")
            # auto mode on a short window: switch kernels, capture again
            self._use_split = True
            self._graph = None
        if self.do_sample:
            # fresh Gumbel(0,1) noise per call: -log(Exp(1)); seeded via
            # torch.manual_seed for reproducible sampling.
            self.gumbel.exponential_().log_().neg_()
        if self._graph is None:
            # capture against scratch state, then restore via real prefill.
            # The 2 warmup steps + capture step advance pos by 3 total, so
            # start low enough that every scratch write stays inside the
            # static window even for tiny max_new_tokens.
            self.pos.fill_(min(prompt_ids.shape[1], self.max_len - 3))
            self._capture()
        self._prefill(prompt_ids, prompt_lens)
        # first generated token came from prefill logits
        self.out_tokens.index_copy_(
            1, self.step_i, self.tok)
        self.step_i.add_(1)
        for _ in range(n - 1):
            self._graph.replay()
        self.last_replays = n - 1
        return self._result(prompt_ids, n, eos_token_id, prompt_lens)

    def _generate_lookahead(self, prompt_ids, n, eos_token_id, prompt_lens,
                            hint_ids):
        if prompt_lens is not None:
            prompt_lens = torch.as_tensor(prompt_lens)
        self._start_lookahead(prompt_ids, prompt_lens, hint_ids)
        self._run_lookahead(n)
        return self._result(prompt_ids, n, eos_token_id, prompt_lens)

    def _start_lookahead(self, prompt_ids, prompt_lens=None, hint_ids=None):
        """Capture if needed, prefill, seed the corpus and the first drafts;
        leaves one emitted token per sequence (the prefill's)."""
        T, plen = self.lookahead, prompt_ids.shape[1]
        assert plen + self.max_new + T <= self.max_len, "window too small"
        if hint_ids is not None:
            assert hint_ids.dim() == 2 and \
                hint_ids.shape[0] == self.batch and \
                hint_ids.shape[1] <= self.max_len, "hint_ids not [b, <= max_len]"
        if self._graph is None:
            # scratch state for the 2 warm-up steps and the capture: each
            # advances pos by at most T
            self.pos.fill_(max(0, min(plen, self.max_len - 4 * T)))
            self.count.zero_()
            self.hint_n.zero_()
            self._capture()
        self._prefill(prompt_ids, prompt_lens)  # tok = the first new token
        nh = 0 if hint_ids is None else hint_ids.shape[1]
        self.hint_n.fill_(nh)
        self.corpus.zero_()
        if nh:
            self.corpus[:, :nh] = hint_ids.to(self.dev)
        self.corpus[:, nh:nh + plen] = prompt_ids.to(self.dev)
        self.corpus.scatter_(1, (self.hint_n + self.pos)[:, None],
                             self.tok[:, :1])
        self.out_tokens[:, :1] = self.tok[:, :1]
        self.count.fill_(1)
        self._draft()

    def _run_lookahead(self, n):
        """Replay until every sequence has n tokens.  A replay emits at most
        T tokens per sequence, so the slowest sequence needs at least
        ceil(missing / T) more: that many are replayed between two host
        reads of the counts.  No replay is wasted, and the reads are few
        when drafts are accepted."""
        T = self.lookahead
        self.last_replays = 0
        while True:
            missing = n - int(self.count.min())
            if missing <= 0:
                break
            for _ in range((missing + T - 1) // T):
                self._graph.replay()
                self.last_replays += 1

    def _result(self, prompt_ids, n, eos_token_id, prompt_lens):
        toks = self.out_tokens[:, :n].clone()
        if eos_token_id is not None:
            # trim after the first EOS per row (host-side, post hoc)
            done = (toks == eos_token_id).cumsum(dim=1) > 0
            toks = toks.masked_fill(done, eos_token_id)
        prompt_ids = prompt_ids.to(self.dev)
        if prompt_lens is None:
            return torch.cat([prompt_ids, toks], dim=1)
        return [torch.cat([prompt_ids[i, :int(ln)], toks[i]])
                for i, ln in enumerate(prompt_lens.tolist())]
