"""Greedy decode loop with a static KV cache and ONE captured hipGraph per decode step (the reference's
`HFGenerator`, hqq/utils/generation_hf.py:117-540, does the same with torch.compile + CUDA graphs).

At batch 1 every fused dequant-GEMV is a few microseconds, i.e. comparable to an eager launch from Python; replaying the whole
step — all decoder layers, attention, sampling argmax — as one graph removes the host from the loop.  The HIP kernels are
capturable by construction (no allocation, no host sync, stream passed in)."""
from __future__ import annotations

import gc

import torch
from torch import Tensor

from .. import ops


def kv_bucket(p: int, attention: str, max_cache_len: int) -> int:
    """the cache bucket a fused step at position p attends over (GraphedGreedyDecoder._kv_len's rule): "sdpa" 64, then multiples of 128 up to 1024,
    then multiples of 512; "hip" (the kernel attention only changes its launch shape beyond 1024 visible keys) 1024, then powers of two; at most the cache"""
    n = p + 1
    if attention == "hip":
        b = 1024
        while b < n:
            b *= 2
    elif n <= 64:                 # SDPA over 64 / 128 / 256 / 512 keys: 6.4 / 9.0 / 14.4 / 24.8 us per block
        b = 64
    elif n <= 1024:
        b = -(-n // 128) * 128
    else:
        b = -(-n // 512) * 512
    return min(b, max_cache_len)


def batch_kv_bucket(positions, attention: str, max_cache_len: int) -> int:
    """the bucket of a batched step: that of the LARGEST row position (every row attends within it, each masked beyond its own position)"""
    return kv_bucket(max(int(p) for p in positions), attention, max_cache_len)


def check_batch_lengths(lengths, max_new_tokens: int, max_cache_len: int) -> None:
    """every prompt of a batch must leave room for max_new_tokens in the cache: T_b + n <= max_cache_len (ValueError naming the first row that does not)"""
    if max_new_tokens < 1:
        raise ValueError("hqq_amd: max_new_tokens must be >= 1")
    for b, T in enumerate(lengths):
        if T < 1 or T + max_new_tokens > max_cache_len:
            raise ValueError(f"hqq_amd: prompt {b} ({T} tokens) + {max_new_tokens} new tokens does not fit a cache of {max_cache_len} positions")


def eos_lengths(rows, eos_token_id, n: int) -> list:
    """per row of generated tokens (lists of ints), how many to keep: up to and including the row's first eos_token_id, else n (generate()'s rule, per row)"""
    out = []
    for r in rows:
        r = list(r)[:n]
        out.append(r.index(eos_token_id) + 1 if eos_token_id is not None and eos_token_id in r else len(r))
    return out


def check_gqa_attention(gqa_attention) -> None:
    """the decoders' gqa_attention keyword: "heads" or "group" (ValueError otherwise)"""
    if isinstance(gqa_attention, bool) or gqa_attention not in ("heads", "group"):
        raise ValueError("gqa_attention: 'heads' or 'group'")


def check_prefill_attention(prefill_attention) -> None:
    """the decoders' prefill_attention keyword: "model" or "hip" (ValueError otherwise)"""
    if isinstance(prefill_attention, bool) or prefill_attention not in ("model", "hip"):
        raise ValueError("prefill_attention: 'model' or 'hip'")


def check_speculation(speculate, draft_rows, ngram_max, do_sample, verify_attention="rows") -> None:
    """the speculative-decoding keywords of GraphedGreedyDecoder and HFGenerator: speculate None or "ngram", draft_rows an integer in 2 .. ops.SPEC_MAX_ROWS,
    ngram_max an integer in 0 .. ops.SPEC_MAX_NGRAM, no sampling with speculation (acceptance is the greedy rule), verify_attention "rows" or "tile" and "tile"
    only with speculation (it names the verify step's attention kernel); ValueError naming the first that is not"""
    if speculate not in (None, "ngram"):
        raise ValueError("speculate: None or 'ngram'")
    for name, value, lo, hi in (("draft_rows", draft_rows, 2, ops.SPEC_MAX_ROWS), ("ngram_max", ngram_max, 0, ops.SPEC_MAX_NGRAM)):
        if isinstance(value, bool) or not isinstance(value, int) or not lo <= value <= hi:
            raise ValueError(f"{name}: an integer in {lo} .. {hi}")
    if speculate is not None and do_sample:
        raise ValueError("speculate: greedy decoding only (do_sample=True draws tokens the n-gram drafts cannot be verified against)")
    if isinstance(verify_attention, bool) or verify_attention not in ("rows", "tile"):
        raise ValueError("verify_attention: 'rows' or 'tile'")
    if verify_attention == "tile" and speculate is None:
        raise ValueError("verify_attention: 'tile' is the speculative verify step's attention kernel (speculate='ngram')")


def check_adapters(bank, adapters, B: int) -> list:
    """the `adapter` / `adapters` keyword of generate() / generate_batch() as one bank index per prompt: None — every prompt decodes on the base model (-1) when
    there is a bank, and nothing is asked when there is none; otherwise a bank is needed and every entry is an int in [-1, bank.n) (-1: the base model).  Returns the
    list (empty without a bank); anything else is a ValueError"""
    if bank is None:
        if adapters is not None:
            raise ValueError("hqq_amd: adapter / adapters pick from a LoRABank: the decoder was built without one (lora_bank=)")
        return []
    if adapters is None:
        return [-1] * B
    adapters = list(adapters)
    if len(adapters) != B:
        raise ValueError(f"hqq_amd: {len(adapters)} adapters for {B} prompts")
    for a in adapters:
        if isinstance(a, bool) or not isinstance(a, int) or not -1 <= a < bank.n:
            raise ValueError(f"hqq_amd: adapter {a!r} is not an index into the bank (-1 .. {bank.n - 1}; -1: the base model)")
    return adapters


def opt_ins(**keywords) -> set:
    """the decode-step opt-in keywords of GraphedGreedyDecoder and HFGenerator (axis0, qk_norm, qkv_bias, lora, moe), each "model" or "fused": the names of those
    set to "fused" (what llama_fused.resolve takes); ValueError naming the first keyword with another value"""
    for name, value in keywords.items():
        if value not in ("model", "fused"):
            raise ValueError(f"{name}: 'model' or 'fused'")
    return {name for name, value in keywords.items() if value == "fused"}


class GraphedGreedyDecoder:
    """fused=True (default): a Llama-shaped model whose decoder linears are HQQLinearHIP layers decodes through hqq_amd.utils.llama_fused —
    RMSNorm (+ the residual adds), rotary + KV-cache write and SiLU * up as one HIP kernel each around the grouped GEMVs, HF's own attention
    function on HF's cache: the same tokens in a third of the launches; since round 5 (glue="auto") the RMSNorms, the residual adds and SiLU * up
    ride inside the GEMV launches themselves: 5 launches + attention per decoder block.  Any other model, or fused=False: the model's own forward.
    axis0: what a model quantised along AXIS 0 decodes through.  "model" (default): the model's own forward, as before.  "fused" (opt-in): where
    llama_fused.supports_axis0 accepts the model, the fused step with q|k|v and gate|up (+ SiLU * up) as one grouped axis-0 launch each
    (`fused_axis0`; `fused` stays the axis-1 flag), and generate_batch's batched step where supports_axis0_batch accepts the batch.
    qk_norm: what a Qwen3 model (per-head q_norm / k_norm in front of the rotary embedding) decodes through.  "model" (default): the model's own forward, as
    before.  "fused" (opt-in): where llama_fused.supports_qk_norm accepts the model, the fused step with ops.qknorm_rope_cache_batched in rope_cache's place
    (`fused_qk_norm`; `fused` stays the Llama flag), and generate_batch's batched step where supports_qk_norm_batch accepts the batch.
    qkv_bias: what a Qwen2 / Qwen2.5 model (biases on q_proj / k_proj / v_proj) decodes through.  "model" (default): the model's own forward, as before.
    "fused" (opt-in): where llama_fused.supports_qkv_bias accepts the model, the fused step with bias-free q|k|v launches and ops.bias_rope_cache_batched in
    rope_cache's place (`fused_qkv_bias`; `fused` stays the Llama flag), and generate_batch's batched step where supports_qkv_bias_batch accepts the batch.
    lora: what a model whose decoder linears still carry LoRA adapters (HQQLinearLoRA wrappers around HQQLinearHIP layers) decodes through.  "model"
    (default): the model's own forward, as before.  "fused" (opt-in): where llama_fused.supports_lora accepts the model, the fused step with one
    ops.lora_shrink + one ops.lora_expand behind each base launch that has adapted layers (`fused_lora`; `fused` stays the Llama flag), and
    generate_batch's batched step where supports_lora_batch accepts the batch.  An adapted model quantised along axis 0 needs axis0="fused" as well.
    lora_bank (opt-in): a core.peft.LoRABank stacked for the model — several adapters over the one quantised base.  generate(ids, n, adapter=i) and
    generate_batch(prompts, n, adapters=[...]) then decode each prompt under the adapter it names (-1 or None: the base model): the prefill of a prompt is
    bank.activate(model, i) followed by the model's own forward, and with lora="fused" the fused step reads the bank itself and picks row b's adapter on the device
    from step.slots (ops.lora_shrink_routed / ops.lora_expand_routed), so prompts under different adapters share one pass over the base weights.  The kept step and
    graphs depend on the bank's tensors, not on the wrappers': another adapter=, another mix of adapters= and bank.set(...) rebuild nothing.  Where the fused step is
    not taken (lora="model", a model or batch it refuses) the bank still serves: activate, then the existing route, prompt after prompt.  Either way the model's
    wrappers are LEFT HOLDING THE LAST ADAPTER ACTIVATED (the last prompt's), lora_B zeroed after a base-model prompt.  adapter / adapters without a bank, or an
    entry outside [-1, bank.n), is a ValueError.
    moe: what a Mixtral or Qwen3-MoE model whose experts are HQQExperts decodes through.  "model" (default): the model's own forward, as before.  "fused"
    (opt-in): where llama_fused.supports_moe accepts the model, the fused step with ops.moe_router, ops.moe_gate_up and ops.moe_down in the MLP's place
    (`fused_moe`; `fused` stays the Llama flag), and generate_batch's batched step where supports_moe_batch accepts the batch (otherwise the prompts decode one
    after another).  A Qwen3-MoE model needs qk_norm="fused" as well.
    Which of these the model gets is decided once, by llama_fused.resolve, and kept as `variant` (None: the model's own forward); the fused_* flags read it.
    generate() and generate_batch() prefill differently and keep different caches, but advance through the same routine (_advance) over a small state
    holder: the device tensors tok / next_tok / pos that the captured graphs read and write, the step (None: the model's own forward), the dictionary
    its graphs are kept in with the key of an attended length in it, and the rule for that length.
    kv_cache: None (default) — HF's dense StaticCache, the code path as before.  "q8" / "q4" (opt-in): generate() and generate_batch() build a
    kv_cache.QuantizedStaticCache (8 / 4 bits per element, rows of kv_group_size values — None: 64, or 32 when head_dim is 64 — quantised when they are
    written) where they build a StaticCache; the prefill is the model's own forward into it, so every attended key and value is the stored, dequantised one.  A
    Llama / Mistral model with attention="hip" then decodes through the fused step on the packed buffers (ops.rope_kvq_cache_batched,
    ops.attn_decode_kvq_batched); everything else through the model's own forward on that cache, which dequantises it per layer.  `kv_cache_bytes` is what the
    kept caches hold on the device.
    speculate: None (default) — one token per step, the code path as before.  "ngram" (opt-in; greedy only): generate() emits SEVERAL tokens per pass over the
    weights by prompt-lookup speculation.  One captured step is ops.spec_propose (the last committed token + draft_rows - 1 guesses: the continuation of the latest
    earlier occurrence of the sequence's last n-gram, n <= ngram_max), the verify step (llama_fused.FusedLlamaStep(batch=draft_rows, verify=True): the rows are
    consecutive positions of the one sequence on its batch-1 cache), the rows' argmax and ops.spec_accept (the guesses the model's own argmax confirms are
    committed: history, position, EOS flag and counters, all on the device).  The host replays `check_every` steps, then reads the position and the flag in one
    copy.  The tokens are the greedy tokens of the verify step's arithmetic (the R-row kernels round differently from the one-row kernels, as generate_batch's do).
    Served where that step is (`speculating`): a Llama / Mistral model, attention="hip", the dense cache, llama_fused.supports_speculation(model, draft_rows);
    everything else decodes as before.  `spec_stats` holds the last call's {"steps", "tokens"}; generate_batch is untouched.
    verify_attention: the verify step's attention kernel.  "rows" (default) — ops.attn_decode_shared, the code path as before.  "tile" (opt-in, with speculate) —
    ops.attn_decode_tiled, which reads each key once for all rows and holds its own contract (a derived band of float64 attention, not the one-row kernel's
    bits).  Where speculation is not served the keyword has no effect; assigning `decoder.verify_attention` rebuilds the kept state at the next generate().
    gqa_attention: the decode-attention kernel's grid with attention="hip".  "heads" (default) — one workgroup per query head, the code path as before.  "group"
    (opt-in) — one workgroup per KV-head group (ops.attn_decode_gqa_batched / ops.attn_decode_gqa_kvq_batched: each key read, and a packed key rebuilt, once for
    the query heads that share it; the tile kernel's contract, not the one-row kernel's bits).  It is passed to the plain and the batched fused steps where
    llama_fused.supports_gqa_attention(model) holds and attention == "hip" (`gqa_grouped` says whether); otherwise, and for the speculative verify step always,
    the keyword has no effect.  Assigning `decoder.gqa_attention` rebuilds the kept state at the next generate().
    prefill_attention: what the prefill's attention runs through.  "model" (default) — the model's own forward as before: HF's attention function on the whole static
    cache (max_cache_len positions under a [T, max_cache_len] mask; on a quantised cache a full-length dequantised copy per layer).  "hip" (opt-in) — every prefill
    this decoder runs (generate(), the speculative generate(), each prompt of generate_batch, behind bank.activate as well) is still the model's own forward, but its
    attention modules call ops.attn_prefill (ops.attn_prefill_kvq on a quantised cache, whose layers then dequantise nothing): only keys [0, t] are read for row t
    (utils/prefill_attn.py switches config._attn_implementation for the duration of that forward).  Its contract is the tile kernel's — within a derived band of
    float64 attention, NOT the bits of SDPA.  Served where llama_fused.supports_prefill_attention holds for the model and the cache (`prefill_hip` says whether);
    otherwise the prefill runs as before.  Independent of `attention`, which names the decode steps' attention."""

    def __init__(self, model, max_cache_len: int = 512, fused: bool = True, attention: str = "sdpa", bucket_cache: bool = True, glue: str = "auto",
                 do_sample: bool = False, temperature: float = 0.6, top_k: int | None = 5, axis0: str = "model", qk_norm: str = "model",
                 qkv_bias: str = "model", lora: str = "model", moe: str = "model", kv_cache: str | None = None, kv_group_size: int | None = None,
                 speculate: str | None = None, draft_rows: int = 8, ngram_max: int = 3, verify_attention: str = "rows", lora_bank=None,
                 gqa_attention: str = "heads", prefill_attention: str = "model"):
        from transformers import StaticCache
        from . import llama_fused
        from .kv_cache import check_kv_group_size, kv_cache_bits
        opted = opt_ins(axis0=axis0, qk_norm=qk_norm, qkv_bias=qkv_bias, lora=lora, moe=moe)
        check_speculation(speculate, draft_rows, ngram_max, do_sample, verify_attention)
        self._verify_attention = verify_attention
        check_gqa_attention(gqa_attention)
        self._gqa_attention = gqa_attention
        check_prefill_attention(prefill_attention)
        self.prefill_attention = prefill_attention
        self.kv_bits = kv_cache_bits(kv_cache)   # (None: the dense StaticCache)
        check_kv_group_size(kv_cache, kv_group_size)
        self.kv_cache, self.kv_group_size = kv_cache, kv_group_size
        self.model = model.eval()
        self.lora_bank = lora_bank
        self.axis0, self.qk_norm, self.qkv_bias, self.lora, self.moe = axis0, qk_norm, qkv_bias, lora, moe
        # the llama_fused.StepVariant this model decodes through (resolve's precedence among the opt-ins), or None: the model's own forward
        self.variant = llama_fused.resolve(model, opted) if fused else None
        self._fused_mod = llama_fused
        self.attention = attention   # "sdpa": HF's attention function (token-identical to model(...)); "hip": the decode-attention kernel (faster, within rounding)
        self.glue = glue             # "auto" / "folded": RMSNorm, residual adds and SiLU * up inside the GEMV launches (csrc/gemv_block.hip); "kernels": round 4's separate glue kernels
        # sampling (the reference's HFGenerator(do_sample=True, temperature=0.6, top_k=5), hqq/utils/generation_hf.py:250-311): applied to the logits ON THE
        # DEVICE inside the captured step — no host round trip, the generator's Philox offset advances per replay —; greedy argmax otherwise
        self.do_sample, self.temperature, self.top_k = bool(do_sample), float(temperature), (None if top_k is None else int(top_k))
        self.bucket_cache = bucket_cache   # attention="sdpa": attend over a bucket of the static cache just above the position (False: all of it)
        self.step = None
        self.device = next(p.device for p in model.parameters() if p.device.type == "cuda")
        self.max_cache_len = max_cache_len
        self._StaticCache = StaticCache
        self.graphs = {}       # attended cache length -> captured step
        self.cache = None      # HF StaticCache, kept between generate() calls (reset in place)
        self._state = None     # the state holder of generate(): its tok / next_tok / pos are self.tok / .next_tok / .pos, its step self.step, its graphs self.graphs
        self._batch = {}       # B -> the state holder of generate_batch at B rows (with its B-row cache and its batch-1 prefill cache)
        self.batch_graphs = {} # (B, attended cache length) -> captured batched step
        # speculative decoding (opt-in): which route generate() takes is known here, as the fused_* flags are; a cache the verify step refuses turns it off in generate()
        self.speculate, self.draft_rows, self.ngram_max = speculate, int(draft_rows), int(ngram_max)
        self.speculating = bool(speculate is not None and self.fused and attention == "hip" and self.kv_bits is None and max_cache_len <= ops.KV_MAX_LEN
                                and llama_fused.supports_speculation(model, self.draft_rows))
        self._spec = None      # the state holder of the speculative route (its own cache, verify step, history, device scalars and graphs)
        self.spec_stats = {"steps": 0, "tokens": 0}
        # whether the prefills attend through ops.attn_prefill: asked for, and a model and cache the kernel covers (otherwise they run as before, without a message)
        self.prefill_hip = bool(prefill_attention == "hip" and llama_fused.supports_prefill_attention(model, max_cache_len, self.kv_bits, kv_group_size))

    @property
    def verify_attention(self) -> str:
        """the attention kernel of the verify step: "rows" or "tile" ("rows" and "tile" alike have no effect where `speculating` is False)"""
        return self._verify_attention

    @verify_attention.setter
    def verify_attention(self, value) -> None:
        check_speculation(self.speculate, self.draft_rows, self.ngram_max, self.do_sample, value)
        self._verify_attention = value   # (part of _fingerprint: the kept verify step and its graphs are rebuilt at the next generate())

    @property
    def gqa_attention(self) -> str:
        """the decode-attention kernel's grid: "heads" or "group" ("group" has an effect only where `gqa_grouped` is True)"""
        return self._gqa_attention

    @gqa_attention.setter
    def gqa_attention(self, value) -> None:
        check_gqa_attention(value)
        self._gqa_attention = value   # (part of _fingerprint: the kept steps and their graphs are rebuilt at the next generate())

    @property
    def gqa_grouped(self) -> bool:
        """whether the plain and the batched fused steps are built with gqa_attention="group": asked for, the kernel attention, and a model with KV groups to serve"""
        return bool(self._gqa_attention == "group" and self.attention == "hip" and self.variant is not None and self._fused_mod.supports_gqa_attention(self.model))

    # `variant` as flags (what bench.py, the tools and the tests read): `fused` is plain Llama's, the others are the opt-in variants, one true at most
    fused = property(lambda self: self.variant is not None and not any(self.variant.flags().values()))
    fused_axis0 = property(lambda self: self.variant is not None and self.variant.axis0 and not self.variant.lora)   # (an adapted axis-0 model is fused_lora's)
    fused_qk_norm = property(lambda self: self.variant is not None and self.variant.family == "qwen3")   # (a Qwen3-MoE model is fused_moe's)
    fused_qkv_bias = property(lambda self: self.variant is not None and self.variant.family == "qwen2")
    fused_lora = property(lambda self: self.variant is not None and self.variant.lora)
    fused_moe = property(lambda self: self.variant is not None and self.variant.flags().get("moe", False))

    def _new_cache(self):
        """the static cache generate() and generate_batch() decode on: HF's dense StaticCache, or (kv_cache="q8" / "q4") the quantised one"""
        if self.kv_bits is None:
            return self._StaticCache(config=self.model.config, max_cache_len=self.max_cache_len)
        from .kv_cache import QuantizedStaticCache
        return QuantizedStaticCache(self.model.config, self.max_cache_len, self.kv_bits, self.kv_group_size)

    def _prefill(self, ids: Tensor, cache):
        """the prompt ids [1, T] through the model's own forward into `cache` (reset by the caller: the rows stand at positions 0 .. T - 1); with `prefill_hip` its
        attention modules attend through ops.attn_prefill for the duration of this call"""
        T = ids.shape[1]
        if not self.prefill_hip:
            return self.model(ids, past_key_values=cache, cache_position=torch.arange(T, device=self.device), use_cache=True)
        from .prefill_attn import hip_prefill
        with hip_prefill(self.model, cache, 0):
            return self.model(ids, past_key_values=cache, cache_position=torch.arange(T, device=self.device), use_cache=True)

    def _step_keywords(self) -> dict:
        """what the fused steps are told about the cache (nothing with the dense one: their call is the one it was)"""
        kw = {} if self.kv_bits is None else {"kv_cache": self.kv_cache}
        if self.lora_bank is not None and self.fused_lora:   # (the other variants serve no adapters: with them the bank works through activate alone)
            kw["lora_bank"] = self.lora_bank
        if self.gqa_grouped:   # (absent otherwise: the steps' call is the one it was)
            kw["gqa_attention"] = "group"
        return kw

    @property
    def kv_cache_bytes(self) -> int:
        """the device bytes of the KV caches kept between calls: generate()'s, and generate_batch()'s B-row and batch-1 prefill caches"""
        def nbytes(c):
            if c is None:
                return 0
            if hasattr(c, "nbytes"):
                return c.nbytes
            return sum(t.numel() * t.element_size() for lay in c.layers for t in (lay.keys, lay.values) if isinstance(t, Tensor))
        return nbytes(self.cache) + sum(nbytes(st["cache"]) + nbytes(st["scratch"]) for st in self._batch.values()) + \
            (0 if self._spec is None else nbytes(self._spec["cache"]))   # (the speculative route decodes on a cache of its own)

    @property
    def graph(self):
        """the graph of the last generate() step that was replayed (None: none yet)"""
        return None if self._state is None else self._state["graph"]

    def _kv_len(self, p: int, fused: bool | None = None) -> int:
        """how much of the static cache a step at position p (a batched or verify step: its LARGEST row position — every row attends within the bucket, each
        masked beyond its own position) attends over; fused: whether a fused step runs it (None: generate()'s, self.step).  HF's attention function costs what it is
        given (the whole masked cache: 304 tok/s at 1024 positions, 119 at 4096, against 500 at 256), so the fused step hands it a bucket just above the position (64, then
        multiples of 128 to 1024, then multiples of 512) and keeps one captured graph per bucket; the kernel attention reads pos + 1 keys by itself and uses the bucket only to decide
        how many workgroups share a head's keys (one up to 1024 keys)"""
        if not (self.step is not None if fused is None else fused) or not self.bucket_cache:
            return self.max_cache_len
        return kv_bucket(p, self.attention, self.max_cache_len)

    def _holder(self, step, tok: Tensor, next_tok: Tensor, pos: Tensor, graphs: dict, key, argmax_advance: bool = True, **more) -> dict:
        """a state holder as _advance, _decode_once and _timed_steps read it: the step (None: the model's own forward), the device tensors the captured graphs
        read and write, the dictionary the graphs are kept in with `key` of an attended length in it, the rule for that length, the last graph replayed"""
        return {"step": step, "tok": tok, "next_tok": next_tok, "pos": pos, "graphs": graphs, "key": key, "kv_len": lambda p: self._kv_len(p, step is not None),
                "argmax_advance": argmax_advance, "graph": None, **more}

    def _pick(self, logits: Tensor) -> Tensor:
        """logits [B, vocab] -> the next tokens [B, 1].  Greedy: argmax.  do_sample: temperature, then the top_k cut, then one draw from the softmax by the
        exponential-race form of a categorical draw (argmax of p / e, e ~ Exp(1)): elementwise kernels + two reductions, nothing leaves the device"""
        if not self.do_sample:
            return logits.argmax(-1, keepdim=True)
        z = logits.float() / max(self.temperature, 1e-5)
        if self.top_k is not None:
            kth = torch.topk(z, min(self.top_k, z.shape[-1])).values[..., -1:]
            z = torch.where(z < kth, torch.full_like(z, float("-inf")), z)
        p = torch.softmax(z, dim=-1)
        return (p / torch.empty_like(p).exponential_(1.0)).argmax(-1, keepdim=True)

    @torch.no_grad()
    def _decode_once(self, st, kv_len=None) -> None:
        """one whole transition of every row: logits at pos -> next_tok, tok = next_tok, pos += 1 (all on the device, so the captured graph carries the loop state forward by itself)"""
        tok, next_tok, pos = st["tok"], st["next_tok"], st["pos"]
        if st.get("verify"):   # the speculative route: propose -> verify step -> row argmax -> accept; hist / p / done / the counters carry the loop forward
            ops.spec_propose(st["hist"], st["p"], tok, pos, self.ngram_max)
            ops.argmax_advance_batched(st["step"](tok, pos, kv_len), next_tok, None, None)
            ops.spec_accept(next_tok, tok, st["hist"], st["p"], st["last"], st["eos"], st["done"], st["steps"], st["tokens"])
            return
        if st["step"] is not None:
            logits = st["step"](tok, pos, kv_len)
            if st["argmax_advance"] and not self.do_sample and logits.dtype in (torch.float16, torch.bfloat16) and logits.is_contiguous():
                ops.argmax_advance_batched(logits, next_tok, tok, pos)   # per row: argmax + hand-over + position increment, one launch (csrc/block.hip)
                return
            next_tok.copy_(self._pick(logits))
        else:   # (generate() only)
            out = self.model(tok, past_key_values=self.cache, cache_position=pos, use_cache=True)
            next_tok.copy_(self._pick(out.logits[:, -1]))
        tok.copy_(next_tok)
        pos += 1

    def _fingerprint(self):
        """what the kept state was built from: identity, storage and version of every quantised layer's packed weights and scale, and the forward HQQLinear is
        bound to (set_backend rebinds it class-wide).  A re-quantised / re-loaded / re-patched model gives another tuple (round-5 advisor: the kept step and
        graphs silently decoded with stale copies).  In-place edits through .data bypass the version counters: call reset() after those."""
        from ..core.quantize import HQQLinear
        # (the verify step's attention kernel and the decode attention's grid are baked into the kept steps and their graphs)
        fp = [getattr(HQQLinear, "backend", None), self._verify_attention, self._gqa_attention]
        bank = self.lora_bank
        if bank is not None:   # the bank's tensors in the place of the wrappers' adapter tensors below (activate rewrites those; set / activate keep the bank's)
            fp.append(bank.pointers())
        for m in self.model.modules():
            W, meta = getattr(m, "W_q", None), getattr(m, "meta", None)
            if isinstance(W, Tensor):
                sc = meta.get("scale") if isinstance(meta, dict) else getattr(m, "scale", None)
                ver = lambda t: None if (t is None or t.is_inference()) else t._version   # noqa: E731
                fp.append((id(m), W.data_ptr(), ver(W), None if sc is None else sc.data_ptr(), ver(sc)))
            A, B = getattr(m, "lora_A", None), getattr(m, "lora_B", None)
            if isinstance(A, Tensor) and isinstance(B, Tensor) and hasattr(m, "linear_layer") and bank is None:
                # an adapter: load_lora_weights / cast replace .data (a kept step or graph would read freed tensors); `scaling` is baked into the step
                ver = lambda t: None if t.is_inference() else t._version   # noqa: E731
                sc = m._scaling_float() if hasattr(m, "_scaling_float") else getattr(m, "scaling", None)
                fp.append((id(m), A.data_ptr(), ver(A), B.data_ptr(), ver(B), sc if isinstance(sc, (int, float)) else id(sc)))
        return tuple(fp)

    def reset(self) -> None:
        """drop what generate() and generate_batch() keep between calls (the static caches, the fused steps with their re-laid-out layer copies, the captured graphs).  generate() calls it
        by itself when the model's quantised layers are no longer the ones the state was built from (_fingerprint)"""
        self.cache = None
        self.step = None
        self.graphs = {}
        self._state = None
        self._batch = {}
        self.batch_graphs = {}
        self._spec = None

    @torch.no_grad()
    def generate(self, input_ids: Tensor, max_new_tokens: int, use_graph: bool = True, eos_token_id: int | None = None, check_every: int = 16,
                 adapter: int | None = None) -> Tensor:
        """continuation of a single sequence [1, T] — greedy, or sampled when the decoder was built with do_sample=True; returns [1, T + n], n = max_new_tokens, or fewer
        when eos_token_id is given and was produced (the sequence then ends with it; the host looks at the tokens every `check_every` steps, never per token).
        The static cache, the fused step (its paired / rotary-paired layer copies) and the captured graphs are KEPT between calls: the next prompt resets the cache in
        place (StaticCache.reset keeps the tensors) and replays the same graphs — hqq/utils/generation_hf.py:190-207, :313-327 keep theirs the same way; reset() drops them.
        adapter (with lora_bank): the bank's adapter the sequence decodes under; None or -1: the base model.  The wrappers are left holding it."""
        assert input_ids.shape[0] == 1, "one sequence (the decode-shaped bs=1 path)"
        slot = check_adapters(self.lora_bank, None if adapter is None else [adapter], 1)
        if slot:
            self.lora_bank.activate(self.model, slot[0])
        T = input_ids.shape[1]
        assert T + max_new_tokens <= self.max_cache_len
        ids = input_ids.to(self.device)
        fp = self._fingerprint()
        if getattr(self, "_fp", None) != fp:   # other weights / layers / backend than the kept step and graphs were built from
            self.reset()
            self._fp = fp
        if self.speculating:
            out = self._generate_speculative(ids, max_new_tokens, use_graph, eos_token_id, check_every)
            if out is not None:   # (None: the verify step refused this cache — `speculating` is off from here on, the plain route below serves)
                return out
        kept = getattr(self, "cache", None) is not None and getattr(self, "_state", None) is not None
        if kept:
            self.cache.reset()
        else:
            self.cache = self._new_cache()
        out = self._prefill(ids, self.cache)
        first = self._pick(out.logits[:, -1])
        if kept:
            st = self._state   # (its tensors are the ones the captured graphs read and write)
            st["tok"].copy_(first)
            st["pos"].fill_(T)
        else:
            self.step = None
            if self.variant is not None:
                try:   # (the plain axis-0 variant takes the separate glue kernels whatever `glue` says; with adapters `glue` goes through, and "folded" is refused)
                    self.step = self._fused_mod.FusedLlamaStep(self.model, self.cache, self.max_cache_len, attention=self.attention,
                                                               glue="kernels" if self.fused_axis0 else self.glue, **self.variant.flags(), **self._step_keywords())
                except ValueError:   # a cache layout / attention configuration the fused step does not restate: the model's own forward serves
                    self.step = None
            self.graphs = {}
            # (glue="kernels" is the comparison leg with the separate front and back: its argmax, hand-over and increment stay torch ops)
            st = self._state = self._holder(self.step, first, torch.empty_like(first), torch.tensor([T], device=self.device), self.graphs, lambda kv: kv,
                                            argmax_advance=self.glue != "kernels")
        if slot and getattr(self.step, "slots", None) is not None:
            self.step.slots.fill_(slot[0])
        elif slot:
            # the composed route under a bank: a captured forward of the wrappers reads lora_A / lora_B in place (activate keeps their addresses) but holds
            # `scaling`, a Python float, as a constant — so its graphs are kept per set of scalings (adapters trained with one alpha / r share them)
            sk = self.lora_bank.scaling_key(slot[0])
            st["key"] = lambda kv: (sk, kv)
        self.tok, self.next_tok, self.pos = st["tok"], st["next_tok"], st["pos"]
        toks = [self.tok.clone()]
        done = 0        # tokens the host has looked at
        n = max_new_tokens
        for i in range(max_new_tokens - 1):
            self._advance(st, T + i, use_graph and (kept or i >= 1))   # (a fresh decoder's step 0 runs eagerly: lazy initialisation inside the model)
            toks.append(self.tok.clone())
            if eos_token_id is not None and (len(toks) - done >= check_every or i == max_new_tokens - 2):
                seen = torch.cat(toks[done:], dim=1)[0].tolist()   # one host read per check_every tokens
                if eos_token_id in seen:
                    n = done + seen.index(eos_token_id) + 1
                    break
                done = len(toks)
        if eos_token_id is not None and n == max_new_tokens and len(toks) == 1 and int(toks[0]) == eos_token_id:
            n = 1
        if self.step is not None:
            self.step.account_tokens(len(toks) - 1)
        return torch.cat([ids] + toks[:n], dim=1)

    def _snapshot(self, st):
        """what one _decode_once changes besides the cache slot it writes (and re-writes when repeated): the token and the positions — and, on the model's own
        forward, each StaticLayer's cumulative_length, the device counter StaticLayer.update takes its slot from and advances itself (a fused step never calls
        update: account_tokens keeps that counter, outside the captured step)"""
        lens = [] if st["step"] is not None or self.cache is None else \
            [lay.cumulative_length for lay in self.cache.layers if isinstance(getattr(lay, "cumulative_length", None), Tensor)]
        lens = lens + list(st.get("carried", ()))   # (the speculative route: the history, the device scalars — p, done, the counters — and the rows' argmax)
        return st["tok"].clone(), st["pos"].clone(), [(t, t.clone()) for t in lens]

    @staticmethod
    def _restore(st, snap) -> None:
        st["tok"].copy_(snap[0]); st["pos"].copy_(snap[1])
        for t, was in snap[2]:
            t.copy_(was)

    def _spec_state(self):
        """the kept state holder of the speculative route — a batch-1 cache of its own, the verify step on it, the token history, ONE int64 tensor with the
        device scalars (p, last, eos, done, steps, tokens: read back in one copy) and the rows' tok / pos / argmax — or None where the verify step refuses"""
        if self._spec is not None:
            return self._spec
        R, dev = self.draft_rows, self.device
        cfg = self.model.config
        cache = self._new_cache()
        cache.early_initialization(1, getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads, self._fused_mod.head_dim(cfg), self.model.model.norm.weight.dtype, dev)
        try:
            step = self._fused_mod.FusedLlamaStep(self.model, cache, self.max_cache_len, attention=self.attention, batch=R, verify=True,
                                                  verify_attention=self._verify_attention)   # (no `glue`: as the batched step)
        except ValueError:
            return None
        scal = torch.zeros(6, dtype=torch.int64, device=dev)
        st = self._holder(step, torch.zeros(R, 1, dtype=torch.int64, device=dev), torch.zeros(R, 1, dtype=torch.int64, device=dev), torch.zeros(R, dtype=torch.int64, device=dev),
                          {}, lambda kv: kv, verify=True, cache=cache, hist=torch.zeros(self.max_cache_len, dtype=torch.int64, device=dev), scalars=scal,
                          p=scal[0:1], last=scal[1:2], eos=scal[2:3], done=scal[3:4], steps=scal[4:5], tokens=scal[5:6], fresh=True)
        st["carried"] = (st["hist"], scal, st["next_tok"])
        self._spec = st
        return st

    @torch.no_grad()
    def _generate_speculative(self, ids: Tensor, max_new_tokens: int, use_graph: bool, eos_token_id, check_every: int):
        """generate() by prompt-lookup speculation (the class docstring): the prefill as on the plain route, then captured steps that each commit 1 .. draft_rows
        tokens on the device.  The host only replays: every `check_every` steps (fewer when fewer can still be needed: a live step commits at least one token) it
        reads the scalars in one copy and stops at done or p >= last.  The cache bucket of a step comes from the host's upper bound of p: the last value read,
        plus draft_rows per step since, plus draft_rows - 1 for the step's last row."""
        st = self._spec_state()
        if st is None:
            self.speculating = False
            return None
        R, T = self.draft_rows, ids.shape[1]
        cache = st["cache"]
        cache.reset()
        out = self._prefill(ids, cache)
        first = self._pick(out.logits[:, -1])
        last = T + max_new_tokens - 1   # the index of the last token to emit; the first one is hist[T]
        eos = -1 if eos_token_id is None else int(eos_token_id)
        st["hist"][:T].copy_(ids[0])
        st["hist"][T:T + 1].copy_(first.view(-1))
        ended = eos >= 0 and int(first) == eos   # (one host read per call, before the loop)
        st["scalars"].copy_(torch.tensor([T, last, eos, int(ended), 0, 0], dtype=torch.int64), non_blocking=False)
        p, done, since = T, ended, 0   # the host's copy of p as last read, and the steps replayed since
        while not done and p < last:
            for _ in range(max(1, min(int(check_every), last - p))):
                hi = min(p + since * R, last) + R - 1   # the largest position a row of this step can have
                self._advance(st, hi, use_graph and not st["fresh"])   # (a fresh state's first step runs eagerly, as generate()'s does)
                st["fresh"] = False
                since += 1
            vals = st["scalars"].tolist()   # one host read per check_every steps
            p, done, since = vals[0], bool(vals[3]), 0
        vals = st["scalars"].tolist()
        self.spec_stats = {"steps": vals[4], "tokens": vals[5]}
        st["step"].account_tokens(p - T)
        return torch.cat([ids, st["hist"][T:p + 1].view(1, -1)], dim=1)

    @torch.no_grad()
    def benchmark_speculative(self, input_ids: Tensor, steps: int = 64, warmup: int = 8) -> dict:
        """the captured speculative step's time at a context of T = input_ids.shape[1] positions: prefill, capture, then time `steps` replays of the step in the
        FROZEN state (last = p = T: propose, the verify step, the argmax and accept all run — rows at positions T .. T + draft_rows - 1 — and accept commits
        nothing, so every replay does the same work at the same context).  ms per step; what a step is worth in tokens is a property of the text, not measured here"""
        assert input_ids.shape[0] == 1 and self.speculating
        T = input_ids.shape[1]
        assert T + self.draft_rows + 2 <= self.max_cache_len
        self.generate(input_ids, 3, use_graph=True)
        st = self._spec
        assert st is not None and self.speculating
        st["scalars"].copy_(torch.tensor([T, T, -1, 0, 0, 0], dtype=torch.int64))
        hi = T + self.draft_rows - 1
        for _ in range(max(2, warmup)):
            self._advance(st, hi, True)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            self._advance(st, hi, True)
        e1.record()
        torch.cuda.synchronize()
        return {"ms_per_step": e0.elapsed_time(e1) / steps, "rows": self.draft_rows, "steps": steps, "prompt_tokens": T}

    @torch.no_grad()
    def _advance(self, st, p: int, use_graph: bool) -> None:
        """one decode step of the state holder st at position p (the host's copy of its LARGEST row position): replay the graph of p's cache bucket, capturing it first if need be"""
        kv = st["kv_len"](p)
        key = st["key"](kv)
        g = st["graphs"].get(key) if use_graph else None
        if use_graph and g is None:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                snap = self._snapshot(st)
                self._decode_once(st, kv)                # warm-up on the side stream (writes cache slot pos, re-written below)
                self._restore(st, snap)
            torch.cuda.current_stream().wait_stream(side)
            g = torch.cuda.CUDAGraph()
            # Python's cyclic collector is held off for the capture: a pass that starts inside it can free a dead decoder (a reference cycle: its state holder keeps
            # bound methods of it) with its captured graphs and cache tensors, and releasing those during a capture aborts the process.  torch.cuda.graph
            # collects before a capture only under torch.compiler.config.force_cudagraph_gc; the model's own forward allocates enough objects to start a pass.
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):
                    self._decode_once(st, kv)
            finally:
                if gc_was_on:
                    gc.enable()
            st["graphs"][key] = g                        # the capture itself does not execute: replay for this step
        if g is not None:
            g.replay()
            st["graph"] = g
        else:
            self._decode_once(st, kv)

    @torch.no_grad()
    def _timed_steps(self, st, p: int, new_tokens: int, warmup: int) -> float:
        """`warmup` steps of the state holder st from position p on (the host's copy of every row's position), then `new_tokens` timed ones (HIP events on
        the current stream; the argmax feeds the next step on the device, the host only replays): ms per step"""
        for _ in range(warmup):
            self._advance(st, p, True)
            p += 1
        for q in range(p, p + new_tokens):                    # buckets the timed steps will enter: captured before the clock starts
            if st["key"](st["kv_len"](q)) not in st["graphs"]:
                snap = self._snapshot(st)
                self._advance(st, q, True)
                self._restore(st, snap)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(new_tokens):
            self._advance(st, p, True)
            p += 1
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / new_tokens

    @torch.no_grad()
    def benchmark(self, input_ids: Tensor, new_tokens: int = 64, warmup: int = 8) -> dict:
        """end-to-end decode rate: prefill `input_ids`, capture the decode step, then time `new_tokens` replays of it (_timed_steps).  Returns tok/s and ms per token."""
        assert input_ids.shape[0] == 1
        T = input_ids.shape[1]
        assert T + warmup + new_tokens + 4 <= self.max_cache_len
        spec, self.speculating = self.speculating, False     # (the one-token step is what is timed here, whatever `speculate` says: benchmark_speculative times the other)
        try:
            self.generate(input_ids, 3, use_graph=True)      # prefill + eager step + captured step (leaves self.graphs, self.tok, self.pos)
        finally:
            self.speculating = spec
        assert self.graph is not None
        ms = self._timed_steps(self._state, T + 2, new_tokens, warmup)   # (T + 2: the host's copy of self.pos)
        return {"ms_per_token": ms, "tok_s": 1e3 / ms, "new_tokens": new_tokens, "prompt_tokens": T}

    # ---- a batch of prompts through ONE fused step per token (llama_fused.FusedLlamaStep with batch = B) ----------------------------------------------------------
    @torch.no_grad()
    def generate_batch(self, prompts, max_new_tokens: int, use_graph: bool = True, eos_token_id: int | None = None, check_every: int = 16,
                       adapters=None) -> list:
        """continuations of B prompts of any lengths (a list of 1-D or [1, T_b] int64 tensors), decoded together: each decode step runs the B sequences
        through one fused step (every linear launch takes the B rows at once, so the weights are streamed once per step for all of them) and is
        captured / replayed as generate()'s is, one graph per (B, cache bucket of the largest row position), kept across calls.  Returns one
        [1, T_b + n_b] tensor per prompt: n_b = max_new_tokens, or fewer when row b produced eos_token_id (it then ends with it; the host looks every
        `check_every` steps, and the loop ends once every row has ended).  Greedy unless the decoder was built with do_sample.
        Prefill: each prompt alone through the model on a kept batch-1 StaticCache (exactly generate()'s prefill, no padding), whose first T_b positions
        are copied into row b of a kept B-row StaticCache; row b's first token comes from its own prefill logits.  The B-row cache's cumulative_length
        is not meaningful (its rows have different lengths): only the fused step reads that cache.
        B == 1 is generate().  A model the batched step does not cover at B rows (llama_fused.supports_batch), or a cache / attention setting it refuses,
        decodes the prompts one after another through generate() instead: the same tokens, only slower.
        adapters (with lora_bank): one bank index per prompt (-1: the base model); None: the base model for all.  Prompt b is prefilled under its adapter
        (bank.activate, then the model's own forward) and row b of the batched step decodes under it (step.slots), in one pass over the base weights for all rows."""
        ids = [torch.as_tensor(p).view(1, -1).to(device=self.device, dtype=torch.int64) for p in prompts]
        B = len(ids)
        slots = check_adapters(self.lora_bank, adapters, B)
        if B == 0:
            return []
        lengths = [x.shape[1] for x in ids]
        check_batch_lengths(lengths, max_new_tokens, self.max_cache_len)
        if B == 1:
            return [self.generate(ids[0], max_new_tokens, use_graph=use_graph, eos_token_id=eos_token_id, check_every=check_every, adapter=slots[0] if slots else None)]
        fp = self._fingerprint()
        if getattr(self, "_fp", None) != fp:
            self.reset()
            self._fp = fp
        st = self._batch.get(B)
        kept = st is not None
        if not kept:
            st = self._batch_state(B)
            if st is None:   # not covered: one prompt after another
                return [self.generate(x, max_new_tokens, use_graph=use_graph, eos_token_id=eos_token_id, check_every=check_every, adapter=slots[b] if slots else None)
                        for b, x in enumerate(ids)]
        bc, scratch = st["cache"], st["scratch"]
        bc.reset()
        firsts = []
        for b, x in enumerate(ids):   # prefill: each prompt alone, then its first T_b key / value positions into row b
            scratch.reset()
            if slots:
                self.lora_bank.activate(self.model, slots[b])
            out = self._prefill(x, scratch)
            firsts.append(self._pick(out.logits[:, -1]))
            for dst, src in zip(bc.layers, scratch.layers):
                if self.kv_bits is not None:   # the six buffers of a quantised layer: rows are independent, so a copied row is the row a B-row prefill would have stored
                    dst.copy_row(b, src, lengths[b])
                    continue
                dst.keys[b, :, :lengths[b]].copy_(src.keys[0, :, :lengths[b]])
                dst.values[b, :, :lengths[b]].copy_(src.values[0, :, :lengths[b]])
        st["tok"].copy_(torch.cat(firsts, dim=0))
        st["pos"].copy_(torch.tensor(lengths, device=self.device))
        if slots and getattr(st["step"], "slots", None) is not None:
            st["step"].slots.copy_(torch.tensor(slots, dtype=torch.int64))
        toks = [st["tok"].clone()]
        done = 0
        n = max_new_tokens
        for i in range(max_new_tokens - 1):
            self._advance(st, max(lengths) + i, use_graph and (kept or i >= 1))   # (a fresh state's step 0 runs eagerly, as in generate())
            toks.append(st["tok"].clone())
            if eos_token_id is not None and (len(toks) - done >= check_every or i == max_new_tokens - 2):
                seen = torch.cat(toks, dim=1).tolist()   # one host read per check_every steps
                if all(eos_token_id in r for r in seen):
                    n = len(toks)
                    break
                done = len(toks)
        rows = torch.cat(toks[:n], dim=1)
        keep = eos_lengths(rows.tolist(), eos_token_id, n)
        return [torch.cat([ids[b], rows[b:b + 1, :keep[b]]], dim=1) for b in range(B)]

    def _batch_state(self, B: int):
        """the kept state holder of generate_batch at B rows, or None when the batched step does not serve the model there"""
        fm = self._fused_mod
        if self.variant is None or not fm.variant_supported(self.model, self.variant, B):
            return None
        cfg, dev = self.model.config, self.device
        cache = self._new_cache()   # (below: StaticLayer.lazy_initialization with batch B)
        cache.early_initialization(B, getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads, fm.head_dim(cfg), self.model.model.norm.weight.dtype, dev)
        try:   # (without the decoder's `glue`: the batched step has the one-launch front and back wherever they apply)
            step = fm.FusedLlamaBatchStep(self.model, cache, self.max_cache_len, B, attention=self.attention, **self.variant.flags(), **self._step_keywords())
        except ValueError:
            return None
        st = self._holder(step, torch.zeros(B, 1, dtype=torch.int64, device=dev), torch.zeros(B, 1, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int64, device=dev),
                          self.batch_graphs, lambda kv: (B, kv), B=B, cache=cache, scratch=self._new_cache())
        self._batch[B] = st
        return st

    @torch.no_grad()
    def benchmark_batch(self, input_ids: Tensor, new_tokens: int = 64, warmup: int = 8) -> dict:
        """benchmark() for a batch: prefill the B rows of input_ids [B, T], capture the batched step, time `new_tokens` replays of it (_timed_steps).
        Returns the step time and the aggregate rate (B tokens per step).  Needs a model the batched step covers at B rows."""
        B, T = input_ids.shape
        assert T + warmup + new_tokens + 4 <= self.max_cache_len
        if B == 1:
            r = self.benchmark(input_ids, new_tokens, warmup)
            return {"ms_per_step": r["ms_per_token"], "tok_s": r["tok_s"], "batch": 1, "new_tokens": new_tokens, "prompt_tokens": T}
        self.generate_batch(list(input_ids), 3, use_graph=True)
        st = self._batch.get(B)
        assert st is not None, "hqq_amd: the batched step does not serve this model at this batch (llama_fused.supports_batch)"
        ms = self._timed_steps(st, T + 2, new_tokens, warmup)
        return {"ms_per_step": ms, "tok_s": B * 1e3 / ms, "batch": B, "new_tokens": new_tokens, "prompt_tokens": T}


# prompts of different lengths for HFGenerator.warmup(): what matters is that the first cache buckets get their graphs captured, not what is asked
WARMUP_PROMPTS = ["Hello.", "Name three prime numbers and say why each one is prime.",
                  "Explain in two paragraphs how a key-value cache speeds up autoregressive decoding, and what it costs in memory."]


class HFGenerator:
    """The reference's generation front end (hqq/utils/generation_hf.py:117-540: HFGenerator(model, tokenizer, ...).generate(prompt) -> {"output_text", "output_tokens",
    "input_tokens"}) over GraphedGreedyDecoder: same constructor arguments, same methods a caller uses (warmup, generate, tokenize_prompt), same defaults
    (cache_size = the next power of two above max_new_tokens, greedy unless do_sample, temperature 0.6 / top_k 5, stop at the tokenizer's EOS).
    What `compile` means here: the reference compiles the decode step with torch.compile ("partial" / "full") and can wrap it in a CUDA graph; this loop has no tracing
    compiler — "partial" / "full" both select the captured-hipGraph step (one graph per token, kept across prompts), None the same step launched eagerly.
    `compile_options` / `patch_accelerate` are accepted and unused.  The decode step itself is hqq_amd.utils.llama_fused (HIP kernels) for Llama-shaped models whose
    linears went through prepare_for_inference(backend="hip"), the model's own forward otherwise.
    Differences a caller can see: EOS is looked for every 16 tokens on the host instead of after every token (no per-token synchronisation; the text returned is cut at
    the EOS all the same); "output_tokens" holds every generated token before the EOS (the reference's slice drops the last one it generated, generation_hf.py:493);
    a prompt that leaves less than max_new_tokens of cache generates what fits.
    speculate / draft_rows / ngram_max / verify_attention / gqa_attention / prefill_attention and attention are GraphedGreedyDecoder's keywords (defaults: no speculation, HF's attention function); speculation is served
    with attention="hip" only, and everything else decodes as before (`decoder.speculating` says which).
    lora_bank, and the adapter / adapters keywords of generate / generate_batch, are GraphedGreedyDecoder's: passed through."""

    def __init__(self, model, tokenizer, max_new_tokens: int = 1000, cache_size: int | None = None, do_sample: bool = False, temperature: float = 0.6, top_k: int = 5,
                 compile: str | None = None, compile_options: dict | None = None, patch_accelerate: bool = True, axis0: str = "model", qk_norm: str = "model",
                 qkv_bias: str = "model", lora: str = "model", moe: str = "model", kv_cache: str | None = None, kv_group_size: int | None = None,
                 speculate: str | None = None, draft_rows: int = 8, ngram_max: int = 3, attention: str = "sdpa", verify_attention: str = "rows", lora_bank=None,
                 gqa_attention: str = "heads", prefill_attention: str = "model"):
        if compile not in (None, "partial", "full"):
            raise ValueError("compile: None, 'partial' or 'full'")
        opt_ins(axis0=axis0, qk_norm=qk_norm, qkv_bias=qkv_bias, lora=lora, moe=moe)   # (GraphedGreedyDecoder's keywords, checked before anything is built)
        from .kv_cache import check_kv_group_size, kv_cache_bits
        kv_cache_bits(kv_cache)
        check_kv_group_size(kv_cache, kv_group_size)
        check_speculation(speculate, draft_rows, ngram_max, do_sample, verify_attention)
        check_gqa_attention(gqa_attention)
        check_prefill_attention(prefill_attention)
        self.model, self.tokenizer = model, tokenizer
        self.device = next(p.device for p in model.parameters() if p.device.type == "cuda")
        self.do_sample = bool(do_sample)
        self.temperature = temperature if self.do_sample else None
        self.top_k = top_k if self.do_sample else None
        self.max_new_tokens = int(max_new_tokens)
        self.cache_size = self.next_multiple(self.max_new_tokens) if cache_size is None else int(cache_size)
        self.max_new_tokens = min(self.max_new_tokens, self.cache_size)
        self.is_compiled = compile is not None
        self.use_graph = compile is not None
        self.compile_options = compile_options
        self.decoder = GraphedGreedyDecoder(model, max_cache_len=self.cache_size, do_sample=self.do_sample, temperature=temperature, top_k=top_k, axis0=axis0, qk_norm=qk_norm,
                                            qkv_bias=qkv_bias, lora=lora, moe=moe, kv_cache=kv_cache, kv_group_size=kv_group_size, speculate=speculate,
                                            draft_rows=draft_rows, ngram_max=ngram_max, attention=attention, verify_attention=verify_attention, lora_bank=lora_bank,
                                            gqa_attention=gqa_attention, prefill_attention=prefill_attention)
        self.init()

    @staticmethod
    def next_multiple(val: int) -> int:
        """the next power of two above val, from 32 (generation_hf.py:233-236)"""
        n = 32
        while n <= val:
            n *= 2
        return n

    def init(self) -> None:
        """inference-mode settings of tokenizer and model (generation_hf.py:238-247)"""
        tk = self.tokenizer
        for name in ("add_bos_token", "add_eos_token"):
            if hasattr(tk, name):
                setattr(tk, name, False)
        if getattr(tk, "pad_token", None) in (None, "") and hasattr(tk, "add_special_tokens"):
            tk.add_special_tokens({"pad_token": "<<[PAD]>>"})
        if hasattr(tk, "padding_side"):
            tk.padding_side = "right"
        self.model.eval()
        # (the reference also sets model.generation_config.cache_implementation = "static" here: its loop shares the model's own generate() settings.  This loop owns its
        #  StaticCache; the setting would only make every LATER model.generate() call of the caller compile the model — generate_() asks for the static cache itself)
        self.model.config.use_cache = True

    def reset(self) -> None:
        """drop the decoder's kept static cache, fused step and captured graphs (GraphedGreedyDecoder.reset; generate() also does it by itself when the model's
        quantised layers changed — call this after an in-place edit of weights that bypasses torch's version counters)"""
        self.decoder.reset()

    def warmup(self, max_samples: int = -1):
        """a few prompts through the loop: the fused step is built and the graphs of the first cache buckets captured before a caller's clock starts"""
        for prompt in WARMUP_PROMPTS[:max_samples if max_samples > 0 else len(WARMUP_PROMPTS)]:
            self.generate(prompt, verbose=False, print_tokens=False)
        return self

    def tokenize_prompt(self, prompt: str, use_chat_template: bool = True):
        if use_chat_template:
            prompt = self.tokenizer.apply_chat_template([{"role": "user", "content": prompt}], tokenize=False, add_generation_prompt=True)
        return self.tokenizer([prompt], return_tensors="pt").to(device=self.device)

    @torch.no_grad()   # (not inference_mode: graph capture updates generator state tensors in place, which inference tensors refuse outside that mode)
    def generate(self, prompt: str, use_chat_template: bool = True, verbose: bool = True, print_tokens: bool = False, adapter: int | None = None) -> dict:
        inputs = self.tokenize_prompt(prompt, use_chat_template=use_chat_template)
        ids = inputs["input_ids"].to(torch.int64)
        T = ids.shape[1]
        n = min(self.max_new_tokens, self.cache_size - T)
        if n < 1:
            raise ValueError(f"hqq_amd: the prompt ({T} tokens) leaves no room in a cache of {self.cache_size}")
        eos = getattr(self.tokenizer, "eos_token_id", None)
        out = self.decoder.generate(ids, n, use_graph=self.use_graph, eos_token_id=eos, **({} if adapter is None else {"adapter": adapter}))
        new = out[0, T:]
        if eos is not None and new.numel() and int(new[-1]) == eos:
            new = new[:-1]
        output_tokens = new.cpu()
        output_text = self.tokenizer.decode(output_tokens)
        if print_tokens:
            print(output_text, flush=True)
        return {"output_text": output_text, "output_tokens": output_tokens, "input_tokens": ids[0].cpu()}

    @torch.no_grad()
    def generate_batch(self, prompts, use_chat_template: bool = True, verbose: bool = True, print_tokens: bool = False, adapters=None) -> list:
        """generate() for several prompts decoded together (GraphedGreedyDecoder.generate_batch): one dict per prompt with generate()'s keys.  Every prompt gets
        the same number of new tokens: max_new_tokens, or what the longest prompt leaves of the cache"""
        ids = [self.tokenize_prompt(p, use_chat_template=use_chat_template)["input_ids"].to(torch.int64) for p in prompts]
        if not ids:
            return []
        T = max(x.shape[1] for x in ids)
        n = min(self.max_new_tokens, self.cache_size - T)
        if n < 1:
            raise ValueError(f"hqq_amd: the longest prompt ({T} tokens) leaves no room in a cache of {self.cache_size}")
        eos = getattr(self.tokenizer, "eos_token_id", None)
        outs = self.decoder.generate_batch(ids, n, use_graph=self.use_graph, eos_token_id=eos, **({} if adapters is None else {"adapters": adapters}))
        res = []
        for x, out in zip(ids, outs):
            new = out[0, x.shape[1]:]
            if eos is not None and new.numel() and int(new[-1]) == eos:
                new = new[:-1]
            output_tokens = new.cpu()
            output_text = self.tokenizer.decode(output_tokens)
            if print_tokens:
                print(output_text, flush=True)
            res.append({"output_text": output_text, "output_tokens": output_tokens, "input_tokens": x[0].cpu()})
        return res

    def generate_(self, prompt: str, use_chat_template: bool = True, verbose: bool = False, print_tokens: bool = False) -> dict:
        """HF's own generate with a static cache (generation_hf.py:515-527): the loop this class replaces, for comparison"""
        gen_out = self.model.generate(**self.tokenize_prompt(prompt, use_chat_template=use_chat_template), do_sample=self.do_sample, cache_implementation="static",
                                      max_new_tokens=self.max_new_tokens, pad_token_id=getattr(self.tokenizer, "pad_token_id", None),
                                      **({"temperature": self.temperature, "top_k": self.top_k} if self.do_sample else {}))[0]
        return {"output_text": self.tokenizer.decode(gen_out), "output_tokens": gen_out}
