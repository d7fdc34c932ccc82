"""One decode step of a Llama-type HF model whose decoder linears are HQQLinearHIP layers, with the steps either side of the fused
GEMVs fused too (the loop the reference's headline tok/s is measured on: hqq/utils/generation_hf.py:117-540, Readme.md:153).
ONE step class, FusedLlamaStep, serves a single sequence and a batch of B independent sequences: the batch size is a parameter (`batch`), every
buffer has B rows, every launch takes the B rows at once and the glue kernels are the *_batched entry points of csrc/block.hip (row b gives the bits
the batch-1 kernel gives for sequence b alone).

HF's decoder block around the seven linears is ~25 eager kernels per block at batch 1 (RMSNorm 5-6, rotary 8, cache update 2, SiLU * up 2,
residual adds 2, ...): 79 % of a token once the linears are fused.  Here a block is, with glue="kernels" (the only sequence at batch > 1, where the linears
run at M = B),
    add_rmsnorm -> q|k|v (one grouped GEMV) -> rope_cache -> attention (HF's own attention function on the static cache) -> o ->
    add_rmsnorm (the residual add of o rides in it) -> gate|up (one grouped GEMV) -> silu_mul -> down (its residual add rides in the next block's add_rmsnorm)
= 8 launches + the attention's; and with glue="folded" (one sequence, the default where csrc/gemv_block.hip covers the model)
    q|k|v with the RMSNorm in its prologue -> rope_cache -> attention -> o with the residual add in its epilogue ->
    ONE paired gate|up layer (RMSNorm prologue, SiLU * up epilogue) -> down with the residual add in its epilogue
where, with q / k in the rotary-paired row order (ops.rotary_pair_layout), rope_cache rides in the q|k|v launch's epilogue too = 4 launches + the attention's.
attention="hip" puts csrc/block.hip's decode-attention kernel in the attention function's place; in the Llama family it takes rope_cache into its launch.
The glue kernels restate the HF modules rounding for rounding and the attention is HF's function on HF's cache tensors, so the step emits the same tokens
as `model(...)` does on the same kernels — and as the same model under HQQBackend.PYTORCH_FORWARD does on the reference's arithmetic (tests/test_model_gpu.py).

That is the base sequence.  WHICH model gets which sequence is one value, a StepVariant (family, axis0, lora); eight exist, and each changes this much of it:

    variant               opt-in (decoder keyword)   what changes                                                                       per block, + attention
    llama                 -                          nothing                                                                            8 kernels / 4 folded
    llama + axis0         axis0                      q|k|v and gate|up through ops.gemv_axis0_grouped (SiLU * up in gate|up's reduce:   7, never folded
                                                     no silu_mul), o / down through ops.gemv_axis0, on the layers' own tensors
    qwen3                 qk_norm                    ops.qknorm_rope_cache_batched (per-head q_norm / k_norm, then rotary + cache) in   8 kernels / 5 folded
                                                     rope_cache's place; no rotary-paired q / k (the norm must see a whole head first)
    qwen2                 qkv_bias                   ops.bias_rope_cache_batched (q / k / v biases added, one rounding each, then       8 kernels / 5 folded
                                                     rotary + cache) in rope_cache's place, behind a bias-free q|k|v launch; no
                                                     rotary-paired q / k (their epilogue rotates before a bias could be added)
    llama + lora          lora                       behind each of the four base launches that has adapted layers, one                 8 + 2 per adapted
                                                     ops.lora_shrink + one ops.lora_expand; never folded                                group
                                                     (lora_bank=: ops.lora_shrink_routed + ops.lora_expand_routed in their place,
                                                     one adapter of a core.peft.LoRABank per row, picked on the device from step.slots)
    llama + lora + axis0  lora and axis0             both of the above; an adapted gate|up runs without SiLU in its reduce, then        7 or 8, + 2 per
                                                     silu_mul (the adapter terms come before SiLU)                                      adapted group
    mixtral               moe                        ops.moe_router (logits, softmax, top-k and renormalisation in one launch, into     8, never folded
                                                     per-block idx / weights), ops.moe_gate_up and ops.moe_down on the HQQExperts
                                                     stacks in the place of gate|up, silu_mul and down
    qwen3_moe             moe and qk_norm            mixtral's MLP half behind qwen3's attention half                                   8, never folded

FAMILIES says what each family asks of an architecture, variant_supported(model, variant, batch) is the one coverage rule behind every supports_*
function, and resolve() is the precedence by which the decoders pick a variant.  Nothing but plain llama is taken without being asked.

Only what the step needs is taken from the model: module weights and the HF StaticCache's tensors are used in place (nothing is copied).

Independently of the variant, FusedLlamaStep(kv_cache="q8" / "q4") (opt-in) runs on a kv_cache.QuantizedStaticCache: ops.rope_kvq_cache_batched and
ops.attn_decode_kvq_batched on the layers' six packed buffers take the place of the rotary-and-cache launch and the attention, with attention="hip" and for the
variants whose rotary launch is plain rope_cache; every other combination is refused, and the decoders then run the model's own forward on that cache.

FusedLlamaStep(batch=R, verify=True) (opt-in; speculative decoding, GraphedGreedyDecoder(speculate="ngram")) is the batched step whose R rows are R consecutive
positions of ONE sequence on a batch-1 cache: ops.rope_cache_shared and ops.attn_decode_shared take the place of the rotary-and-cache launch and the attention.
verify_attention="tile" (opt-in) puts ops.attn_decode_tiled — each key read once for all rows, a contract of its own — in ops.attn_decode_shared's place.
Plain llama with attention="hip" on the dense cache only (supports_speculation); every other combination is refused.

FusedLlamaStep(attention="hip", gqa_attention="group") (opt-in) attends with one workgroup per KV-HEAD GROUP (csrc/attn_gqa.hip): the family's rotary-and-cache
launch, then ops.attn_decode_gqa_batched (dense cache), or ops.rope_kvq_cache_batched, then ops.attn_decode_gqa_kvq_batched (quantised cache).  Every variant
and batch that attention="hip" serves, on models with 2 .. 16 query heads per KV head (supports_gqa_attention); not the verify step.  The same launches per block
as "heads", except in the Llama family on the dense cache: one more (9 kernels / 6 folded against 8 / 5), because "heads" attends inside its rotary launch there.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace

import torch
from torch import Tensor

from .. import ops
from ..backends.hip import HQQLinearHIP, _GroupedMember


def _hip(layer):
    return layer.layer if isinstance(layer, _GroupedMember) else layer


def _is_lora(layer) -> bool:
    from ..core.peft import is_hqq_lora_layer
    return is_hqq_lora_layer(layer)


def _unwrap(layer):
    """the quantised layer behind an HQQLinearLoRA wrapper (prepare_for_inference keeps the wrapper and patches its linear_layer), or the layer itself"""
    return _hip(layer.linear_layer) if _is_lora(layer) else _hip(layer)


def head_dim(cfg) -> int:
    """the attention head size of an HF config: its own head_dim where it names one (Qwen3's need not be hidden_size // num_attention_heads), else that quotient"""
    return getattr(cfg, "head_dim", None) or cfg.hidden_size // cfg.num_attention_heads


@dataclass(frozen=True)
class Family:
    """What one served model family asks of an architecture (_arch_ok walks a model once against it) and which step variants it admits."""
    name: str
    model_types: tuple    # config.model_type, an allow-list: models that merely LOOK like Llama (same attribute names) would decode wrong tokens without an error
    qk_norm: bool         # per-head q_norm / k_norm on every attention module: required (1-D, head_dim elements, the compute dtype, an epsilon) / forbidden
    qkv_bias: bool        # a bias on q_proj, k_proj and v_proj of every block and none on the other four linears: required / not looked at here (the config's
                          # attention_bias / mlp_bias are refused in every family, and _structure refuses a bias on any quantised layer)
    sliding: tuple        # which of the config's sliding-window signals refuse the model (a window on an attention MODULE refuses it in every family)
    axis0: bool           # admits models quantised along axis 0 (the axis-0 kernels have no head-norm or bias sequence)
    lora: bool            # admits un-merged LoRA adapters
    moe: bool = False     # the block's MLP is a routed mixture of experts: `mlp.gate` a dense top-k router, `mlp.experts` an HQQExperts, and nothing else


FAMILIES = {f.name: f for f in (
    # LlamaDecoderLayer (transformers models/llama, models/mistral).  Their configs have neither use_sliding_window nor layer_types; a Mistral with a
    # window says so in config.sliding_window, and that is the one signal looked at.
    Family("llama", ("llama", "mistral"), qk_norm=False, qkv_bias=False, sliding=("sliding_window",), axis0=True, lora=True),
    # Qwen3DecoderLayer (models/qwen3; not qwen3_moe): Llama's block with an RMSNorm over head_dim on every head of q and k before the rotary embedding.
    # All three signals refuse (Qwen3Config clears sliding_window itself unless use_sliding_window is on).
    Family("qwen3", ("qwen3",), qk_norm=True, qkv_bias=False, sliding=("sliding_window", "use_sliding_window", "layer_types"), axis0=False, lora=False),
    # Qwen2DecoderLayer (models/qwen2): Llama's block with a bias on q_proj / k_proj / v_proj.  ONLY layer_types is looked at: Qwen2 / Qwen2.5 checkpoints
    # carry a default config.sliding_window while use_sliding_window is off and every layer attends fully, so that field must not refuse them; and
    # use_sliding_window alone changes nothing until max_window_layers makes some layer_types entry a sliding one.
    Family("qwen2", ("qwen2",), qk_norm=False, qkv_bias=True, sliding=("layer_types",), axis0=False, lora=False),
    # MixtralDecoderLayer (models/mixtral): Mistral's block with MixtralSparseMoeBlock (a MixtralTopKRouter and fused experts) in the MLP's place.
    Family("mixtral", ("mixtral",), qk_norm=False, qkv_bias=False, sliding=("sliding_window",), axis0=False, lora=False, moe=True),
    # Qwen3MoeDecoderLayer (models/qwen3_moe) where every block is sparse: Qwen3's block with Qwen3MoeSparseMoeBlock in the MLP's place.  Dense blocks
    # (mlp_only_layers, decoder_sparse_step != 1) have no `experts` and refuse the model; so do shared experts (Qwen2-MoE, DeepSeek: other model types anyway).
    Family("qwen3_moe", ("qwen3_moe",), qk_norm=True, qkv_bias=False, sliding=("sliding_window", "use_sliding_window", "layer_types"), axis0=False, lora=False, moe=True),
)}

# the router class each MoE family's blocks carry (ops.moe_router restates exactly these two forwards)
_ROUTERS = {"mixtral": "MixtralTopKRouter", "qwen3_moe": "Qwen3MoeTopKRouter"}


def _moe_mlp_ok(mlp, family: Family, cfg, dt) -> bool:
    """an MoE family's question about a block's `mlp` (in the place of the dense families' SiLU check): its children are `gate` and `experts` and nothing
    else (no shared expert, no dense MLP); experts is a ready HQQExperts (SiLU by construction); gate is the family's router class with ONE parameter, a
    dense weight [E, H] of the compute dtype on the experts' device (no bias), an integer top_k in 1 .. 8 and, for Qwen3-MoE, a boolean norm_topk_prob"""
    from ..core.moe import HQQExperts
    if set(dict(mlp.named_children())) != {"gate", "experts"}:
        return False
    gate, ex = mlp.gate, mlp.experts
    if not isinstance(ex, HQQExperts) or not ex.ready or type(gate).__name__ != _ROUTERS[family.name]:
        return False
    if [n for n, _ in gate.named_parameters()] != ["weight"] or getattr(gate, "bias", None) is not None:
        return False
    w = gate.weight
    if w.dim() != 2 or tuple(w.shape) != (ex.num_experts, cfg.hidden_size) or w.dtype != dt or not w.is_contiguous() or w.device != ex.gate_W_q.device:
        return False
    if isinstance(gate.top_k, bool) or not isinstance(gate.top_k, int) or not 1 <= gate.top_k <= min(8, ex.num_experts):
        return False
    return family.name != "qwen3_moe" or isinstance(gate.norm_topk_prob, bool)


def _arch_ok(model, family: Family) -> bool:
    """The allow-list half of variant_supported(): whether `model` is of `family`, i.e. its decoder block is the arithmetic the step restates and nothing
    else.  Refused in every family: another model_type, soft-capping, config.attention_bias / mlp_bias, Granite-style multipliers (residual / embedding /
    logits / attention) other than 1, attention sinks or a qk_norm module, a sliding window on an attention module, an activation other than SiLU.
    What differs between the families is FAMILIES' fields; an MoE family asks _moe_mlp_ok of every block's mlp where the others ask for SiLU."""
    try:
        cfg = model.config
        if getattr(cfg, "model_type", None) not in family.model_types:
            return False
        if getattr(cfg, "attn_logit_softcapping", None) or getattr(cfg, "final_logit_softcapping", None):
            return False
        if getattr(cfg, "attention_bias", False) or getattr(cfg, "mlp_bias", False):
            return False
        if any(getattr(cfg, odd, None) not in (None, 1, 1.0) for odd in ("residual_multiplier", "embedding_multiplier", "logits_scaling", "attention_multiplier")):
            return False
        if any(getattr(cfg, sig, None) for sig in family.sliding if sig != "layer_types"):
            return False
        if "layer_types" in family.sliding and any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or ())):
            return False
        dt = model.model.norm.weight.dtype
        if family.qk_norm:
            hd = head_dim(cfg)
        for blk in model.model.layers:
            at = blk.self_attn
            if any(hasattr(at, n) for n in ("qk_norm", "sinks")) or getattr(at, "sliding_window", None):
                return False
            if family.qk_norm:
                for nrm in (at.q_norm, at.k_norm):
                    if nrm.weight.dim() != 1 or nrm.weight.shape[0] != hd or nrm.weight.dtype != dt or not isinstance(nrm.variance_epsilon, (int, float)):
                        return False
            elif hasattr(at, "q_norm") or hasattr(at, "k_norm"):
                return False
            if family.qkv_bias:
                if any(getattr(at, n).bias is None for n in ("q_proj", "k_proj", "v_proj")):
                    return False
                if at.o_proj.bias is not None or any(getattr(blk.mlp, n).bias is not None for n in ("gate_proj", "up_proj", "down_proj")):
                    return False
            if family.moe:
                if not _moe_mlp_ok(blk.mlp, family, cfg, dt):
                    return False
            elif type(getattr(blk.mlp, "act_fn", None)).__name__ not in ("SiLUActivation", "SiLU"):
                return False
        return True
    except (AttributeError, TypeError):
        return False


def arch_supported(model) -> bool:
    """a Llama / Mistral architecture (FAMILIES["llama"]): what the plain step, its axis-0 and its LoRA variants restate.  Qwen3 and Qwen2 are refused HERE —
    this predicate and the defaults built on it stay Llama's — and have predicates of their own"""
    return _arch_ok(model, FAMILIES["llama"])


def qk_norm_arch_supported(model) -> bool:
    """a Qwen3 architecture (FAMILIES["qwen3"]): what the step with qk_norm=True restates"""
    return _arch_ok(model, FAMILIES["qwen3"])


def qkv_bias_arch_supported(model) -> bool:
    """a Qwen2 / Qwen2.5 architecture (FAMILIES["qwen2"]): what the step with qkv_bias=True restates (what the biases must look like on the quantised
    layers is _structure's question)"""
    return _arch_ok(model, FAMILIES["qwen2"])


def moe_arch_supported(model) -> bool:
    """a Mixtral or an all-sparse Qwen3-MoE architecture (FAMILIES["mixtral"] / ["qwen3_moe"]) whose experts are HQQExperts: what the step with moe=True restates"""
    return _arch_ok(model, FAMILIES["mixtral"]) or _arch_ok(model, FAMILIES["qwen3_moe"])


def _no_variant(**flags) -> ValueError:
    return ValueError(f"hqq_amd: no fused decode step for {' with '.join(k + '=True' for k, on in flags.items() if on)}: axis0 and lora=True go with Llama / Mistral "
                      "models only (an axis-0 or adapted Qwen decodes through the model's own forward), no served architecture has both q/k/v biases and head norms, "
                      "and moe=True goes alone (Mixtral) or with qk_norm=True (Qwen3-MoE)")


@dataclass(frozen=True)
class StepVariant:
    """Which sequence of launches a model decodes through: its family, whether its linears are quantised along axis 0, whether they still carry LoRA
    adapters.  Eight exist (VARIANTS): only the Llama family admits axis 0 or adapters, and the two MoE families are variants by their family alone.  The step
    and the decoders each hold one; from_flags() / flags() translate from and to FusedLlamaStep's boolean keywords."""
    family: str = "llama"
    axis0: bool = False
    lora: bool = False

    def __post_init__(self):
        fam = FAMILIES.get(self.family)
        if fam is None:
            raise ValueError(f"hqq_amd: no family {self.family!r} ({', '.join(FAMILIES)})")
        if (self.axis0 and not fam.axis0) or (self.lora and not fam.lora):
            raise _no_variant(**self.flags())

    @classmethod
    def from_flags(cls, axis0: bool = False, qk_norm: bool = False, qkv_bias: bool = False, lora: bool = False, moe: bool = False) -> "StepVariant":
        """the variant FusedLlamaStep's keywords name; ValueError for the combinations that name none (ten without moe; with moe, everything but moe alone —
        Mixtral — and moe with qk_norm — Qwen3-MoE)"""
        if (qk_norm and qkv_bias) or (moe and (axis0 or qkv_bias or lora)):
            raise _no_variant(axis0=axis0, qk_norm=qk_norm, qkv_bias=qkv_bias, lora=lora, moe=moe)
        if moe:
            return cls("qwen3_moe" if qk_norm else "mixtral")
        return cls("qwen3" if qk_norm else "qwen2" if qkv_bias else "llama", bool(axis0), bool(lora))

    def flags(self) -> dict:
        """from_flags' inverse: the booleans as FusedLlamaStep's keywords — the four of the dense variants, and "moe": True in addition for the two MoE ones"""
        fam = FAMILIES[self.family]
        flags = {"axis0": self.axis0, "qk_norm": fam.qk_norm, "qkv_bias": fam.qkv_bias, "lora": self.lora}
        if fam.moe:
            flags["moe"] = True
        return flags


# every variant there is, in resolve()'s order of precedence
VARIANTS = (StepVariant(), StepVariant(axis0=True), StepVariant("qwen3"), StepVariant("qwen2"), StepVariant(lora=True), StepVariant(axis0=True, lora=True),
            StepVariant("mixtral"), StepVariant("qwen3_moe"))


def _decoder_linears(model, lora: bool = False, moe: bool = False):
    """the seven linears of every decoder block, q k v o gate up down, as HQQLinearHIP layers (lora: the layer behind an HQQLinearLoRA wrapper where there is one);
    moe: the four attention linears only (the MLP's place is taken by a router and an HQQExperts)"""
    get = _unwrap if lora else _hip
    return [[get(getattr(b.self_attn, n)) for n in ("q_proj", "k_proj", "v_proj", "o_proj")] +
            ([] if moe else [get(getattr(b.mlp, n)) for n in ("gate_proj", "up_proj", "down_proj")]) for b in model.model.layers]


def _decoder_wrappers(model):
    """beside _decoder_linears(model, lora=True): per block, the HQQLinearLoRA wrapper of each of the seven linears, or None where it is not adapted"""
    return [[(w if _is_lora(w) else None) for w in [getattr(b.self_attn, n) for n in ("q_proj", "k_proj", "v_proj", "o_proj")] +
             [getattr(b.mlp, n) for n in ("gate_proj", "up_proj", "down_proj")]] for b in model.model.layers]


def _bias_ok(L, dt, wanted: bool) -> bool:
    """a decoder linear's bias as _structure asks for it: none, or (wanted) a dense 1-D tensor of out_features elements in the compute dtype on the layer's device"""
    if not wanted:
        return L.bias is None
    b = L.bias
    return isinstance(b, Tensor) and b.dim() == 1 and b.shape[0] == L.out_features and b.is_contiguous() and b.dtype == dt and b.device == L.W_q.device


def _structure(model, variant: StepVariant):
    """The structural half of variant_supported(): an architecture of the variant's family (_arch_ok), fp16 or bf16, the rotary / embedding / lm_head modules
    the step calls, every decoder linear an HQQLinearHIP of the compute dtype, quantised along the variant's axis, on the GPU, and RMSNorm weights of that
    dtype with a multiple of 8 features.  Biases: no decoder linear may have one, except that in a family with qkv_bias q_proj, k_proj and v_proj must each
    HAVE one — 1-D, dense, out_features elements, the compute dtype, the layer's device.  With lora the checks apply to the layers behind HQQLinearLoRA
    wrappers (what the wrappers themselves must look like is _lora_wrappers_ok's question).
    An MoE family: the four attention linears only (what the router and the experts must look like is _arch_ok's question, which kernels cover them _moe_covers').
    Returns (dtype, _decoder_linears(model)), or None where the model is not of that shape; which kernels cover the layers is the caller's question."""
    family = FAMILIES[variant.family]
    if not _arch_ok(model, family):
        return None
    try:
        inner = model.model
        dt = inner.norm.weight.dtype
        if dt not in (torch.float16, torch.bfloat16):
            return None
        if not hasattr(inner, "rotary_emb") or not hasattr(inner, "embed_tokens") or not hasattr(model, "lm_head"):
            return None
        blocks = _decoder_linears(model, variant.lora, family.moe)
        for blk, lin in zip(inner.layers, blocks):
            if not all(isinstance(L, HQQLinearHIP) and L.compute_dtype == dt and L.W_q.is_cuda and L.axis == (0 if variant.axis0 else 1) for L in lin):
                return None
            if not all(_bias_ok(L, dt, family.qkv_bias and i < 3) for i, L in enumerate(lin)):
                return None
            for nrm in (blk.input_layernorm, blk.post_attention_layernorm):
                if nrm.weight.dtype != dt or nrm.weight.shape[0] % 8:
                    return None
        return dt, blocks
    except AttributeError:
        return None


def batch_covers(dtype, B: int, layers, opts: int = 0) -> bool:
    """whether the fused decode kernels serve every layer of `layers` — (N, K, group_size, nbits, w3s) each — at M = B activation rows (a pure
    function of the shapes: no device needed).  The grouped launch (hqq_hip_gemv_grouped) takes a group of layers at B rows where each of them is
    served on its own, so the rule is per layer: a decode route (ops.route, asked for the layer's layout)."""
    B = int(B)
    if B < 1:
        return False
    factored = bool(int(opts) & ops.OPT_FACTORED) and dtype == torch.float16
    for (N, K, gs, nbits, w3s) in set(layers):   # (a model repeats a few shapes)
        r = ops.route(dtype, B, (N,), K, gs, nbits, ops.OPT_W3S if w3s else 0)
        if r not in ops.DECODE_ROUTES:
            return False
        # a policy, not a kernel limit: FACTORED batches beyond 8 rows only on the skinny kernel (the row-per-wave kernel would serve them in launches of 8)
        if factored and B > 8 and r != ops.ROUTE_SKINNY:
            return False
    return True


# the four places of a decoder block where adapters are served, as slices of (q, k, v, o, gate, up, down): each is one base launch, followed by one
# lora_shrink + one lora_expand over the adapted layers among its members
LORA_GROUPS = (("qkv", 0, 3), ("o", 3, 4), ("gu", 4, 6), ("d", 6, 7))


def _lora_wrappers_ok(model, B: int) -> bool:
    """the wrapper half of variant_supported() for the lora variants: at least one decoder linear is an HQQLinearLoRA; every wrapper has no bias and does not
    train one, no active dropout, and lora_A [K, r] / lora_B [r, N] dense, of ONE dtype the kernels cover, on the layer's device; ops.lora_decode_covers
    holds for the adapted layers of each group at B rows"""
    from torch import nn
    try:
        dt = model.model.norm.weight.dtype
        found = False
        for lin, wrs in zip(_decoder_linears(model, True), _decoder_wrappers(model)):
            for L, w in zip(lin, wrs):
                if w is None:
                    continue
                found = True
                A, Bm = w.lora_A.data, w.lora_B.data
                if w.bias is not None or w.train_bias or not (isinstance(w.peft_drop, nn.Identity) or not w.training):
                    return False
                if A.dtype != Bm.dtype or A.dim() != 2 or Bm.dim() != 2 or tuple(A.shape) != (L.in_features, w.r) or tuple(Bm.shape) != (w.r, L.out_features):
                    return False
                if not (A.is_contiguous() and Bm.is_contiguous() and A.device == L.W_q.device and Bm.device == L.W_q.device):
                    return False
                w._scaling_float()
            for _, lo, hi in LORA_GROUPS:
                ad = [(L, w) for L, w in zip(lin[lo:hi], wrs[lo:hi]) if w is not None]
                if ad and (len({w.lora_A.dtype for _, w in ad}) != 1 or
                           not ops.lora_decode_covers(dt, ad[0][1].lora_A.dtype, B, [L.out_features for L, _ in ad], ad[0][0].in_features, [w.r for _, w in ad])):
                    return False
        return found
    except (AttributeError, TypeError, ValueError):
        return False


def _moe_covers(model, dt, B: int) -> bool:
    """the expert half of variant_supported() for the MoE families, at B rows: every block's HQQExperts in a layout the routed expert kernel reads (byte
    containers, no view_as_float, ONE packing and group size over gate / up / down, axis 1, stacks of the compute dtype on the GPU), ops.moe_covers and
    ops.moe_router_covers for its shapes.  ops.MOE_ROUTE_MAX_T is HQQExperts' own route policy and is not asked: the step has no composed alternative"""
    from ..core.moe import ROLES
    from ..core.quantize import Quantizer
    for blk in model.model.layers:
        ex, gate = blk.mlp.experts, blk.mlp.gate
        g = ex.layer_meta["gate"]
        if any(ex.layer_meta[r]["view_as_float"] or ex.layer_meta[r]["packing"] not in ("4bit_u8", "2bit_u8") or ex.layer_meta[r]["packing"] != g["packing"]
               or ex.layer_meta[r]["group_size"] != g["group_size"] or ex.layer_meta[r]["axis"] != 1 for r in ROLES):
            return False
        if not (ex.gate_W_q.is_cuda and gate.weight.is_cuda) or ex.gate_scale.dtype != dt:
            return False
        if not ops.moe_covers(dt, B, gate.top_k, ex.num_experts, ex.hidden_dim, ex.intermediate_dim, g["group_size"], Quantizer._packing_bits[g["packing"]], 1):
            return False
        if not ops.moe_router_covers(dt, B, gate.top_k, ex.num_experts, ex.hidden_dim):
            return False
    return True


def variant_supported(model, variant: StepVariant, batch: int | None = None) -> bool:
    """Whether the fused step of `variant` serves `model` — the one rule behind every supports_* function below.  batch=None asks about one sequence, an
    integer about that many rows, and the two are NOT the same question at 1: on axis 1 without adapters, one sequence asks only that q|k|v and gate|up can
    each share a grouped launch (the folded or grouped kernels then take the layers as they are), while B rows — 1 included — ask in addition for a decode
    route of every linear at M = B (batch_covers); the axis-0 and the lora variants have no other sequence than the B-row one, so for them None means 1.
    Everything else is common: _structure, then
      axis 1: q|k|v share (nbits, group_size, layout) and so do gate|up; q is one the decode kernels cover, or 3-bit stream; qwen3: a head_dim
      ops.qknorm_rope_cache_batched serves (64 / 128 / 256; ops.bias_rope_cache_batched serves any even one, so qwen2 asks for none);
      axis 0: 1 <= B <= ops.GEMV_MAX_M; q|k|v share (nbits, group_size) and gate|up share them with equal N, so that each group is ONE grouped launch
      (ops.axis0_grouped_covers, gate|up with BLOCK_SILU); o and down on the single-layer kernel (ops.decode_axis0_covers);
      lora: the wrappers as _lora_wrappers_ok asks for them, any subset of the seven linears adapted, with different ranks;
      mixtral / qwen3_moe: the axis-1 rule over q|k|v (there is no gate|up pair), B <= ops.MOE_MAX_T, and _moe_covers at B rows; qwen3_moe: qwen3's head_dim."""
    B = 1 if batch is None else int(batch)
    moe = FAMILIES[variant.family].moe
    if B < 1 or (variant.axis0 and B > ops.GEMV_MAX_M) or (variant.lora and not _lora_wrappers_ok(model, B)) or (moe and B > ops.MOE_MAX_T):
        return False
    found = _structure(model, variant)
    if found is None:
        return False
    dt, blocks = found
    if variant.axis0:
        for (q, k, v, o, g, u, d) in blocks:
            if len({(L.nbits, L.group_size, L.in_features) for L in (q, k, v)}) != 1 or len({(L.nbits, L.group_size, L.in_features, L.out_features) for L in (g, u)}) != 1:
                return False
            if not ops.axis0_grouped_covers(dt, B, [L.out_features for L in (q, k, v)], q.in_features, q.group_size, q.nbits) or \
                    not ops.axis0_grouped_covers(dt, B, [g.out_features, u.out_features], g.in_features, g.group_size, g.nbits, ops.BLOCK_SILU):
                return False
            if not all(ops.decode_axis0_covers(dt, B, L.out_features, L.in_features, L.group_size, L.nbits) for L in (o, d)):
                return False
        return True
    for lin in blocks:
        if len({(L.nbits, L.group_size, L.w3s) for L in lin[:3]}) != 1 or len({(L.nbits, L.group_size, L.w3s) for L in lin[4:6]}) > 1:   # (an MoE block has no gate|up pair)
            return False
        if not ops.decode_covers(dt, 1, lin[0].out_features, lin[0].in_features, lin[0].group_size, lin[0].nbits) and not lin[0].w3s:
            return False
    if moe and not _moe_covers(model, dt, B):
        return False
    if FAMILIES[variant.family].qk_norm and head_dim(model.config) not in (64, 128, 256):
        return False
    if batch is None and not variant.lora:
        return True
    return batch_covers(dt, B, [(L.out_features, L.in_features, L.group_size, L.nbits, L.w3s) for lin in blocks for L in lin], ops._default_opts)


def resolve(model, opted, batch: int | None = None) -> StepVariant | None:
    """The variant a decoder gives `model`: the first of VARIANTS — llama, then axis 0, then qwen3, then qwen2, then lora on axis 1, then lora on axis 0 — that
    is opted into and that variant_supported accepts (at `batch`), or None: the model's own forward; mixtral and qwen3_moe come last.  `opted` holds the
    opt-ins among "axis0", "qk_norm", "qkv_bias", "lora", "moe"; a variant is opted into when every flag it sets is (plain llama sets none: always; lora on
    axis 0 needs both, and so does qwen3_moe: qk_norm and moe)."""
    opted = set(opted)
    for variant in VARIANTS:
        if all(k in opted for k, on in variant.flags().items() if on) and variant_supported(model, variant, batch):
            return variant
    return None


def supports(model) -> bool:
    """one sequence of a Llama / Mistral model quantised along axis 1: what the decoders take by default"""
    return variant_supported(model, StepVariant())


def supports_batch(model, B: int) -> bool:
    return variant_supported(model, StepVariant(), B)


def supports_axis0(model) -> bool:
    """supports() for a model quantised along AXIS 0"""
    return variant_supported(model, StepVariant(axis0=True))


def supports_axis0_batch(model, B: int) -> bool:
    return variant_supported(model, StepVariant(axis0=True), B)


def supports_qk_norm(model) -> bool:
    """supports() for a Qwen3 model: what FusedLlamaStep(qk_norm=True) takes"""
    return variant_supported(model, StepVariant("qwen3"))


def supports_qk_norm_batch(model, B: int) -> bool:
    return variant_supported(model, StepVariant("qwen3"), B)


def supports_qkv_bias(model) -> bool:
    """supports() for a Qwen2 / Qwen2.5 model: what FusedLlamaStep(qkv_bias=True) takes"""
    return variant_supported(model, StepVariant("qwen2"))


def supports_qkv_bias_batch(model, B: int) -> bool:
    return variant_supported(model, StepVariant("qwen2"), B)


def supports_lora(model, axis0: bool | None = None) -> bool:
    """supports() / supports_axis0() for a model whose decoder linears still carry their LoRA adapters.  axis0: None — either axis; False / True — that one"""
    return supports_lora_batch(model, 1, axis0)


def supports_lora_batch(model, B: int, axis0: bool | None = None) -> bool:
    return any(variant_supported(model, StepVariant(axis0=a, lora=True), B) for a in (False, True) if axis0 in (None, a))


def supports_moe(model) -> bool:
    """supports() for a Mixtral or Qwen3-MoE model whose experts are HQQExperts: what FusedLlamaStep(moe=True) (with qk_norm=True for Qwen3-MoE) takes"""
    return any(variant_supported(model, StepVariant(f)) for f in _ROUTERS)


def supports_moe_batch(model, B: int) -> bool:
    return any(variant_supported(model, StepVariant(f), B) for f in _ROUTERS)


def supports_speculation(model, rows: int) -> bool:
    """the coverage rule of the verify step (FusedLlamaStep(batch=rows, verify=True)): 2 .. ops.SPEC_MAX_ROWS rows, a Llama / Mistral model on axis 1 without
    adapters that the batched step serves at that many rows (variant_supported(model, StepVariant(), rows)), and a head_dim the decode-attention kernel covers"""
    if isinstance(rows, bool) or not isinstance(rows, int) or not 2 <= rows <= ops.SPEC_MAX_ROWS or not variant_supported(model, StepVariant(), rows):
        return False
    return head_dim(model.config) in (64, 128, 256)


def supports_gqa_attention(model) -> bool:
    """whether FusedLlamaStep(..., attention="hip", gqa_attention="group") has a KV group to serve on this model: 2 .. 16 query heads per KV head
    (ops.attn_gqa_covers) of a head_dim the decode-attention kernels cover"""
    cfg = model.config
    n_heads = cfg.num_attention_heads
    n_kv = getattr(cfg, "num_key_value_heads", None) or n_heads
    return ops.attn_gqa_covers(n_heads, n_kv) and head_dim(cfg) in (64, 128, 256)


def supports_prefill_attention(model, max_cache_len: int | None = None, kv_bits: int | None = None, kv_group_size: int | None = None) -> bool:
    """the coverage rule of GraphedGreedyDecoder(prefill_attention="hip") (utils/prefill_attn.py; ops.attn_prefill / ops.attn_prefill_kvq attend ONE sequence's
    prompt): full attention in every layer — the sliding-window signals _arch_ok reads for the model's family (FAMILIES; every one of them for a model type no
    family names), and no window on an attention module —, no attention sinks, no soft-capping of the attention logits, keys and values of one head_dim of
    64 / 128 / 256, fp16 / bf16, query heads a multiple of the KV heads.  The hook sits behind the projections, the norms and the rotary embedding, so nothing
    else about the block is asked.  With max_cache_len also the cache the decoder would build: a dense StaticCache of up to ops.KV_MAX_LEN positions, or
    (kv_bits 8 / 4, kv_group_size None: ops.kv_group_size's default) a QuantizedStaticCache that ops.kv_covers serves."""
    try:
        cfg = model.config
        hd = head_dim(cfg)
        n_heads = cfg.num_attention_heads
        n_kv = getattr(cfg, "num_key_value_heads", None) or n_heads
        if hd not in (64, 128, 256) or n_heads % n_kv or getattr(cfg, "attn_logit_softcapping", None):
            return False
        if any(getattr(cfg, name, None) not in (None, hd) for name in ("v_head_dim", "qk_head_dim")):
            return False
        family = next((f for f in FAMILIES.values() if getattr(cfg, "model_type", None) in f.model_types), None)
        sliding = ("sliding_window", "use_sliding_window", "layer_types") if family is None else family.sliding
        if any(getattr(cfg, sig, None) for sig in sliding if sig != "layer_types"):
            return False
        if "layer_types" in sliding and any(t != "full_attention" for t in (getattr(cfg, "layer_types", None) or ())):
            return False
        dt = model.model.norm.weight.dtype
        if dt not in (torch.float16, torch.bfloat16):
            return False
        for blk in model.model.layers:
            at = blk.self_attn
            if hasattr(at, "sinks") or getattr(at, "sliding_window", None) or not isinstance(getattr(at, "layer_idx", None), int):
                return False
        if max_cache_len is None:
            return True
        if kv_bits is None:
            return 1 <= int(max_cache_len) <= ops.KV_MAX_LEN
        return ops.kv_covers(dt, kv_bits, hd, ops.kv_group_size(hd) if kv_group_size is None else kv_group_size, int(max_cache_len))
    except (AttributeError, TypeError):
        return False


def _rec(L):
    """a layer as ops.gemv_block and the re-layout functions take it"""
    return (L.W_q, L.scale, L.zero, L.out_features)


def _rec5(L):
    """a layer as the grouped launches take it (the bias slot stays None: where the model has biases, the rotary-and-cache launch adds them)"""
    return (L.W_q, L.scale, L.zero, None, L.out_features)


def _opts(scalable: bool, w3s: bool) -> int:
    return ops.layer_opts((ops.OPT_META_SCALABLE if scalable else 0) | (ops.OPT_W3S if w3s else 0))


def _gopts(Ls) -> int:
    return _opts(all(L.opts & ops.OPT_META_SCALABLE for L in Ls), Ls[0].w3s)


def _relaid_scalable(dt, t, L) -> bool:
    """whether t = (W_q, scale, zero, N), a re-laid-out copy of layer L's rows (rotary-paired, or paired with another layer's), takes the three-op rebuild: its
    condition depends on the slab a row sits in (J = 9 - the slab's bit offset) and the re-layout moves rows between slabs, so it is checked again on the
    copy's tensors, never inherited from the layers"""
    if dt != torch.float16:
        return False
    return ops.w3s_meta_scalable(t[1], t[2], t[3], L.in_features) if L.w3s else ops.meta_scalable(t[1], t[2], t[3], L.in_features, L.group_size, L.nbits)


# the rotary-and-cache launch of a family, by its (qk_norm, qkv_bias): the launch's name (looked up in ops at every call) and what it takes of block b between v and cos
_ROTARY = {
    (False, False): ("rope_cache_batched", lambda b: ()),
    # Qwen3 (and the attention half of Qwen3-MoE): the heads of q and k normalised, rotated and cached in one launch
    (True, False): ("qknorm_rope_cache_batched", lambda b: (b["attn"].q_norm.weight, b["attn"].k_norm.weight, b["attn"].q_norm.variance_epsilon, b["attn"].k_norm.variance_epsilon)),
    # Qwen2: the projections' biases added to the bias-free q|k|v, then rotated and cached, one launch
    (False, True): ("bias_rope_cache_batched", lambda b: b["qkv_bias"]),
}


class FusedLlamaStep:
    """decode step t of `batch` independent sequences -> logits of their tokens t + 1, on the model's own weights and an HF StaticCache of that batch
    that a prefill has filled (layer.keys / .values [batch, n_kv, max_cache_len, hd], used in place).  Each sequence has its own position; row b of
    every glue kernel gives the bits of the batch-1 kernel for sequence b alone, and the linears run at M = batch."""

    def __init__(self, model, cache, max_cache_len: int, attention: str = "sdpa", glue: str = "auto", axis0: bool = False, batch: int = 1,
                 qk_norm: bool = False, qkv_bias: bool = False, lora: bool = False, moe: bool = False, kv_cache: str | None = None, verify: bool = False,
                 verify_attention: str = "rows", lora_bank=None, gqa_attention: str = "heads"):
        """attention: "sdpa" — HF's own attention function on the cache tensors (the step then emits the tokens `model(...)` would);
        "hip" — csrc/block.hip's decode-attention kernel (one query per head, fp32 softmax): within rounding of SDPA, not bit-identical,
        3-4 us instead of 12-15 per block.
        glue: "folded" — RMSNorm in the q|k|v / gate|up launches' prologue, the residual adds in o's / down's epilogue, SiLU * up in the epilogue of ONE
        paired gate|up layer (csrc/gemv_block.hip: 4 launches + rotary / attention per block; costs a second copy of gate / up's packed levels in the
        paired layout); "kernels" — round 4's separate glue kernels (9 launches per block); "auto": folded where hqq_hip_gemv_block covers the model.
        batch: the number of sequences.  Beyond 1 the model must be one supports_batch (supports_axis0_batch with axis0) accepts at that many rows;
        the folded launches serve one activation row, so a batch takes the separate glue kernels whatever `glue` allows.
        axis0, qk_norm, qkv_bias, lora: together they name the StepVariant (self.variant) whose sequence the step runs — the table in the module's docstring;
        a combination that names none is a ValueError, and so is a model that variant_supported refuses for it at `batch` rows.  axis0 and lora take the
        separate glue kernels (the folded launches read axis-1 meta and serve no adapters: glue="folded" is refused); qk_norm and qkv_bias fold all but their
        rotary-and-cache launch, and with attention="hip" the kernel attends on that launch's rotated q_out (ops.attn_decode_batched).  lora: the adapter
        terms are added on the input the base launch read — o's on self.delta before the residual add, gate|up's before SiLU — and `scaling` is read once, here.
        moe (Mixtral; with qk_norm=True: Qwen3-MoE): the separate glue kernels (glue="folded" is refused), with ops.moe_router, ops.moe_gate_up and ops.moe_down
        on the HQQExperts stacks in the place of gate|up, silu_mul and down.  Per block, counted from the stages _choose picks: add_rmsnorm, q|k|v, the rotary-and-cache launch,
        o, add_rmsnorm, moe_router, moe_gate_up, moe_down = 8 launches + the attention's (9 with attention="sdpa", whose function is one SDPA launch here).  The
        router writes idx / weights into per-block buffers that the two expert launches read on the device: nothing is cast or copied in between.
        kv_cache: None — `cache` is an HF StaticCache, as above.  "q8" / "q4" (opt-in) — `cache` is a kv_cache.QuantizedStaticCache of that width, and per block the
        step launches q|k|v (RMSNorm folded where `glue` allows), ops.rope_kvq_cache_batched (rotary, then the new key and value quantised into the six buffers),
        ops.attn_decode_kvq_batched on the packed rows, o and the rest as above: no dense key / value tensor exists.  Only with attention="hip" (no SDPA runs on packed
        bytes), up to 16 rows, and for the variants whose rotary launch is plain rope_cache (the Llama family's, Mixtral); neither the rotary-paired q / k layout nor
        ops.rope_attn_decode_batched is used with it.  Everything else is a ValueError, which the decoders turn into the model's own forward on that cache.
        verify (opt-in; speculative decoding): the `batch` rows are `batch` CONSECUTIVE POSITIONS OF ONE SEQUENCE — the last committed token and batch - 1 guessed
        ones — on a batch-1 StaticCache (keys / values [1, n_kv, max_cache_len, hd]).  Per block the separate-glue sequence of the batched step runs with
        ops.rope_cache_shared + ops.attn_decode_shared in the place of the rotary-and-cache launch and the attention: every row's key and value are written first (a
        launch of its own: row i reads the keys rows < i write in the same step), then row i attends over keys [0, pos[i]].  Row i's logits are those of the
        sequence's token at pos[i] given the rows before it, so a caller that feeds the true continuation gets every next token in one pass over the weights.  Rows
        of rejected guesses leave finite stale keys and values beyond the committed length: nothing reads them, and the next step rewrites them before a row that
        could see them.  Served: the plain Llama / Mistral variant (no axis0 / qk_norm / qkv_bias / lora / moe keyword), attention="hip", the dense cache, 2 .. 16
        rows of a model supports_speculation accepts; everything else is a ValueError.
        verify_attention (with verify=True): "rows" (default) — ops.attn_decode_shared, every row bit-identical to the one-row kernel at its position, every key read
        once PER ROW.  "tile" (opt-in) — ops.attn_decode_tiled in its place: one workgroup per (head, split) reads each key once for ALL rows; deterministic, a row
        independent of the other rows' queries, within a derived band of float64 attention and NOT bit-identical to the one-row kernel (include/hqq_hip.h).  Any
        other value, and "tile" without verify=True, is a ValueError.
        lora_bank (opt-in, with lora=True): a core.peft.LoRABank stacked for this model.  The four adapter stages then call ops.lora_shrink_routed /
        ops.lora_expand_routed on the bank's tensors, and row b decodes under adapter self.slots[b] — int64 [batch] on the device at a static address, -1 (no
        adapter, the base model; the initial value) or an index into the bank.  The caller writes it with slots.copy_(...) between steps; a captured step follows
        it, as it follows bank.set(...).  The wrappers' own lora_A / lora_B / scaling are not read.  Row b's logits are the bits of the one-adapter step on the model
        with adapter slots[b] in its wrappers.  A bank without lora=True, with verify=True, whose layers are not exactly the model's decoder wrappers, or that
        ops.lora_routed_covers refuses for a group at `batch` rows, is a ValueError.
        gqa_attention (with attention="hip"): "heads" (default) — one workgroup per QUERY head (csrc/block.hip, csrc/kv_cache.hip), the code path as it was.  "group"
        (opt-in) — one workgroup per KV-HEAD GROUP (csrc/attn_gqa.hip): the family's rotary-and-cache launch, then ops.attn_decode_gqa_batched on the rotated qr
        (dense cache), or ops.rope_kvq_cache_batched, then ops.attn_decode_gqa_kvq_batched (quantised cache); each key is read, and a packed key rebuilt, once for
        the n_heads / n_kv_heads query heads that share it.  Its contract is the tile kernel's: deterministic, within a derived band of float64 attention, NOT
        bit-identical to "heads".  Launches per block against "heads": the same for the Qwen families, Mixtral and every quantised-cache step; ONE MORE for the
        Llama family on the dense cache, where "heads" rotates, caches and attends in the one rope_attn_decode_batched launch (with the separate glue kernels 9
        against 8, folded 6 against 5; a split launch adds its merging launch to either).  The split count comes from ops.attn_gqa_splits.  Served for every variant and batch that attention="hip" serves; refused
        (ValueError) with attention="sdpa", with verify=True (the verify step keeps verify_attention) and where ops.attn_gqa_covers is false (n_heads / n_kv_heads
        outside 2 .. 16).  Any other value is a ValueError."""
        from transformers.modeling_utils import ALL_ATTENTION_FUNCTIONS
        from transformers.models.llama.modeling_llama import eager_attention_forward
        self.variant = variant = StepVariant.from_flags(axis0=axis0, qk_norm=qk_norm, qkv_bias=qkv_bias, lora=lora, moe=moe)
        self.axis0, self.qk_norm, self.qkv_bias, self.lora = (variant.flags()[k] for k in ("axis0", "qk_norm", "qkv_bias", "lora"))
        self.moe = FAMILIES[variant.family].moe
        self.model, self.inner, cfg = model, model.model, model.config
        self.device = self.inner.embed_tokens.weight.device
        self.dt = self.inner.norm.weight.dtype   # fp16 or bf16 (supports())
        self.B = int(batch)
        self.n_heads = cfg.num_attention_heads
        self.n_kv = getattr(cfg, "num_key_value_heads", None) or cfg.num_attention_heads
        self.hd = head_dim(cfg)
        self.H, self.L = cfg.hidden_size, max_cache_len
        self.attn_fn = ALL_ATTENTION_FUNCTIONS.get_interface(cfg._attn_implementation, eager_attention_forward)
        self.attention, self.verify, self.verify_attention = attention, bool(verify), verify_attention
        self.gqa_attention = gqa_attention
        self._rope_cache, self._rope_extra = _ROTARY[FAMILIES[variant.family].qk_norm, FAMILIES[variant.family].qkv_bias]
        self.lora_bank = lora_bank
        if lora_bank is not None and (not lora or verify):
            raise ValueError("hqq_amd: lora_bank serves the lora=True variants of the decode step (and no verify step): " +
                             ("verify=True takes no bank" if verify else "it needs lora=True"))
        self.kv_bits = self._check(cache, glue, kv_cache)   # (None: the dense cache)
        self._verify_attn = ops.attn_decode_tiled if verify_attention == "tile" else ops.attn_decode_shared
        linears = [lin + [None] * (7 - len(lin)) for lin in _decoder_linears(model, self.lora, self.moe)]   # (an MoE block: q k v o, and no gate up down)
        wrappers = _decoder_wrappers(model) if self.lora else [[None] * 7 for _ in linears]
        if lora_bank is not None:
            self._check_bank(linears, wrappers)
        self.folded, self.extra_weight_bytes = self._fold(glue, linears)
        self.blocks = [self._block(blk, lin, wrs, cache.layers[li]) for li, (blk, lin, wrs) in enumerate(zip(self.inner.layers, linears, wrappers))]
        self._buffers(glue)

    def _check(self, cache, glue: str, kv_cache):
        """the constructor's refusals that need no look at a layer, in the order in which they win (the cache is only asked what it is);
        returns kv_cache's bit width, None for the dense cache"""
        from .kv_cache import QuantizedStaticCache, kv_cache_bits
        model, cfg, variant, attention, B = self.model, self.model.config, self.variant, self.attention, self.B
        if attention not in ("sdpa", "hip"):
            raise ValueError("attention: 'sdpa' or 'hip'")
        if attention == "hip" and (self.hd not in (64, 128, 256) or getattr(cfg, "sliding_window", None) or getattr(cfg, "attn_logit_softcapping", None)
                                   or self.L > 30000):
            raise ValueError("hqq_amd: the decode-attention kernel covers plain softmax attention with head_dim 64 / 128 / 256 and caches of <= 30000 positions")
        if self.verify_attention not in ("rows", "tile"):
            raise ValueError("verify_attention: 'rows' or 'tile'")
        if self.verify_attention == "tile" and not self.verify:
            raise ValueError("hqq_amd: verify_attention='tile' is the verify step's attention: it needs verify=True")
        if self.gqa_attention not in ("heads", "group"):
            raise ValueError("gqa_attention: 'heads' or 'group'")
        if self.gqa_attention == "group":
            if attention != "hip":
                raise ValueError("hqq_amd: gqa_attention='group' is a kernel attention: it needs attention='hip'")
            if self.verify:
                raise ValueError("hqq_amd: gqa_attention='group' serves the decode step; the verify step keeps verify_attention ('rows' / 'tile')")
            if not ops.attn_gqa_covers(self.n_heads, self.n_kv):
                raise ValueError(f"hqq_amd: gqa_attention='group' needs 2 .. {ops.ATTN_GQA_MAX_G} query heads per KV head (ops.attn_gqa_covers): this model has "
                                 f"{self.n_heads} / {self.n_kv}")
        if self.verify and (variant != StepVariant() or attention != "hip" or kv_cache is not None or not supports_speculation(model, B)):
            raise ValueError(f"hqq_amd: verify=True serves the plain Llama / Mistral step with attention='hip' on a dense cache, for 2 .. {ops.SPEC_MAX_ROWS} rows of a "
                             "model llama_fused.supports_speculation accepts")
        if glue not in ("auto", "folded", "kernels"):
            raise ValueError("glue: 'auto', 'folded' or 'kernels'")
        if glue == "folded" and (self.lora or self.axis0 or self.moe):
            raise ValueError("hqq_amd: glue='folded' reads axis-1 meta of seven dense linears and serves no adapters: "
                             f"{'lora=True' if self.lora else 'axis0=True' if self.axis0 else 'moe=True'} takes the separate glue kernels")
        # (a single sequence of an axis-1 Llama is not asked: its callers ask supports(), and models construct here that it refuses)
        if (variant != StepVariant() or B != 1) and not variant_supported(model, variant, None if B == 1 else B):
            on = [k for k, v in variant.flags().items() if v]
            fn = "supports" + ("_lora" if self.lora else "_moe" if self.moe else "_" + on[0] if on else "")
            raise ValueError(f"hqq_amd: {', '.join(k + '=True' for k in on) or 'a batch'} needs a model of the {variant.family} family whose decoder linears "
                             f"the fused decode kernels serve at {B} rows ({fn} / {fn}_batch)")
        kv_bits = kv_cache_bits(kv_cache)
        if kv_bits is not None:
            if attention != "hip" or self._rope_cache != "rope_cache_batched" or not 1 <= B <= 16:
                raise ValueError("hqq_amd: the fused step reads a quantised KV cache only with attention='hip', for 1 .. 16 rows of a variant whose rotary launch is "
                                 "rope_cache (Llama / Mistral / Mixtral); the model's own forward serves the rest on that cache")
            if not isinstance(cache, QuantizedStaticCache) or cache.nbits != kv_bits:
                raise ValueError(f"hqq_amd: kv_cache={kv_cache!r} needs a QuantizedStaticCache of {kv_bits} bits")
        elif isinstance(cache, QuantizedStaticCache):
            raise ValueError("hqq_amd: a QuantizedStaticCache needs the kv_cache keyword ('q8' / 'q4')")
        return kv_bits

    def _check_bank(self, linears, wrappers) -> None:
        """the constructor's refusals of a LoRABank: its layers are exactly the model's decoder wrappers, its tensors are where and what the routed kernels read"""
        bank = self.lora_bank
        named = {getattr(w, "name", None): (L, w) for lin, wrs in zip(linears, wrappers) for L, w in zip(lin, wrs) if w is not None}
        if None in named or sorted(named) != sorted(bank.names):
            raise ValueError("hqq_amd: the LoRABank's layers are not exactly the HQQLinearLoRA wrappers of the model's decoder linears")
        for name, (L, w) in named.items():
            A, Bm, sc = bank.layer(name)
            if tuple(A.shape) != (bank.n, L.in_features, w.r) or tuple(Bm.shape) != (bank.n, w.r, L.out_features) or A.dtype != Bm.dtype or \
                    not (A.is_contiguous() and Bm.is_contiguous()) or any(t.device != L.W_q.device for t in (A, Bm, sc)):
                raise ValueError(f"hqq_amd: the LoRABank's tensors for {name!r} are not the stacked [n, K, r] / [n, r, N] of that layer on its device")
        for lin, wrs in zip(linears, wrappers):
            for _, lo, hi in LORA_GROUPS:
                ad = [(L, bank.layer(w.name)[0]) for L, w in zip(lin[lo:hi], wrs[lo:hi]) if w is not None]
                if ad and (len({A.dtype for _, A in ad}) != 1 or
                           not ops.lora_routed_covers(self.dt, ad[0][1].dtype, bank.n, self.B, [L.out_features for L, _ in ad], ad[0][0].in_features,
                                                      [A.shape[2] for _, A in ad])):
                    raise ValueError(f"hqq_amd: the routed adapter kernels do not cover this LoRABank at {self.B} rows (ops.lora_routed_covers)")

    def _fold(self, glue: str, linears):
        """whether the step runs the folded launches, and the bytes of the layer copies they keep: (folded, extra_weight_bytes)"""
        can_fold = not self.lora and not self.moe and all(ops.block_covers(self.dt, L.in_features, L.group_size, L.nbits, L.w3s, norm=norm)
                       for (q, _, _, o, g, _, d) in linears for L, norm in ((q, True), (o, False), (g, True), (d, False))) and \
            all(g.out_features == u.out_features for (_, _, _, _, g, u, _) in linears) and not (ops._default_opts & ops.OPT_FACTORED) and not self.axis0 and self.B == 1
        if glue == "folded" and not can_fold:
            raise ValueError("hqq_amd: glue='folded' needs one sequence and fp16 / bf16 layers of 4 / 2 bits or the 3-bit stream layout, group_size 64, hidden size <= 8192")
        if not can_fold or glue == "kernels":
            return False, 0
        # The folded step keeps re-laid-out COPIES of q, k (rotary-paired rows) and of gate | up (one paired layer) beside the layers' own tensors: about
        # +60 % of the decoder's linear-weight bytes (7B at 4 bits: +1.9 GB).  glue="auto" takes them only when they fit with room to spare; a model that filled
        # the GPU before keeps round 4's separate glue kernels (no copy) instead of running out of memory here (round-5 advisor).  glue="folded" insists.
        need = sum(L.W_q.numel() * L.W_q.element_size() + 2 * L.scale.numel() * L.scale.element_size() for (q, k, _, _, g, u, _) in linears for L in (q, k, g, u))
        free_b = torch.cuda.mem_get_info(self.device)[0] if self.device.type == "cuda" else need * 4
        if glue == "auto" and free_b < need + need // 4 + (1 << 30):
            import warnings
            warnings.warn(f"hqq_amd: the folded decode step needs {need / 1e9:.2f} GB for its paired layer copies, {free_b / 1e9:.2f} GB are free: "
                          "falling back to the separate glue kernels (glue='kernels')")
            return False, 0
        return True, need

    def _choose(self, adapted_gu: bool) -> dict:
        """WHICH LAUNCHES A BLOCK OF THIS STEP RUNS — the one statement of the precedence among the step's modes.  A block is three stages; per stage the first rule
        that matches wins, and each rule is one method below, holding exactly its launches.  The constructor calls this once per block (adapted_gu: the block's
        gate | up carry an adapter), builds what the chosen stages ask for, and __call__ runs them; nothing else restates a condition.
          q|k|v          1  folded, the SDPA attention, the llama family, an even head_dim: gemv_block with BLOCK_NORM | BLOCK_ROPE on the rotary-paired copies of
                            q / k (which exist because of this rule: "qkv_rope"), writing the rotated q into qr and k / v into the caches                 _qkv_folded_rope
                         2  folded otherwise: gemv_block with BLOCK_NORM into q, k, v                                                                     _qkv_folded
                         3  else: add_rmsnorm(h, delta, n1), the grouped q|k|v launch (axis 0 or 1), the qkv adapters                                    _qkv_kernels
          rotary, cache  0  gqa_attention="group" (the kernel attention only; no verify step) — a quantised cache: rope_kvq_cache_batched,
          and attention     attn_decode_gqa_kvq_batched; the dense cache: the family's rotary-and-cache launch (_ROTARY), attn_decode_gqa_batched     _attend_kvq_gqa / _attend_rotary_gqa
                         1  a quantised cache: rope_kvq_cache_batched, attn_decode_kvq_batched                                                            _attend_kvq
                         2  the verify step: rope_cache_shared, then _verify_attn (attn_decode_shared or attn_decode_tiled)                               _attend_verify
                         3  the kernel attention in the llama family (its axis-0 and lora variants too): rope_attn_decode_batched, one launch             _attend_rope_attn
                         4  else the family's rotary-and-cache launch (_ROTARY) — unless q|k|v rule 1 has rotated and cached already —, then
                            attn_decode_batched ("hip") or self.attn_fn on the first kv_len positions ("sdpa")                     _attend_rotary_hip / _attend_rotary_sdpa / _attend_sdpa
          o and the MLP  1  folded: three gemv_block launches — o with BLOCK_RESID, the paired gate|up with BLOCK_NORM | BLOCK_SILU, down with BLOCK_RESID;
                            no delta is left for the next add_rmsnorm                                                                                     _mlp_folded
                         2  else the single-layer o launch, the o adapters, add_rmsnorm(h, delta, n2), then
                            an MoE family: moe_router, moe_gate_up, moe_down                                                                              _mlp_moe
                            axis 0 whose gate | up carry no adapter: ONE grouped launch with BLOCK_SILU, down, the down adapters                          _mlp_silu_in_reduce
                            otherwise: grouped gate|up, the gu adapters (they come before SiLU), silu_mul, down, the down adapters                        _mlp_kernels
        The grouped and single-layer launches themselves are the axis-0 or the axis-1 pair."""
        S, hip, llama = FusedLlamaStep, self.attention == "hip", self.variant.family == "llama"
        qkv = S._qkv_kernels if not self.folded else S._qkv_folded_rope if not hip and llama and self.hd % 2 == 0 else S._qkv_folded
        if self.gqa_attention == "group":   # (_check: attention="hip", no verify step)
            attend = S._attend_kvq_gqa if self.kv_bits is not None else S._attend_rotary_gqa
        elif self.kv_bits is not None:
            attend = S._attend_kvq
        elif self.verify:
            attend = S._attend_verify
        elif hip:
            attend = S._attend_rope_attn if llama else S._attend_rotary_hip
        else:
            attend = S._attend_sdpa if qkv is S._qkv_folded_rope else S._attend_rotary_sdpa
        mlp = S._mlp_folded if self.folded else S._mlp_moe if self.moe else S._mlp_silu_in_reduce if self.axis0 and not adapted_gu else S._mlp_kernels
        grouped, single = (S._grouped_axis0, S._single_axis0) if self.axis0 else (S._grouped_axis1, S._single_axis1)
        # (plain functions, called with the step: a record that held bound methods would tie the step and its layer copies into a reference cycle)
        return {"qkv_stage": qkv, "attend_stage": attend, "mlp_stage": mlp, "grouped": grouped, "single": single}

    def _block(self, blk, lin, wrs, lay) -> dict:
        """one block's record: its modules, launch records and output buffers, the cache tensors of `lay`, the adapters of `wrs`, the stages _choose picks and
        the re-laid-out layer copies those stages ask for"""
        q, k, v, o, g, u, d = lin
        B, dt, dev, S = self.B, self.dt, self.device, FusedLlamaStep
        cache_rows = 1 if self.verify else B   # (verify: the B rows share ONE sequence's cache)
        if self.kv_bits is not None:   # the six buffers in the place of keys / values (kv_cache.QuantizedStaticLayer)
            if not getattr(lay, "is_initialized", False) or tuple(lay.bufs[0].shape[:3]) != (B, self.n_kv, self.L) or lay.k_head_dim != self.hd or lay.dtype != dt:
                raise ValueError(f"hqq_amd: the fused decode step needs an initialised QuantizedStaticCache of batch {B} and {self.L} positions")
            kv = {"kvq": lay.bufs}
        elif not getattr(lay, "is_initialized", False) or tuple(lay.keys.shape) != (cache_rows, self.n_kv, self.L, self.hd) or \
                not lay.keys.is_contiguous() or not lay.values.is_contiguous():
            raise ValueError(f"hqq_amd: the fused decode step needs an initialised HF StaticCache of batch {cache_rows} and {self.L} positions")
        else:
            kv = {"kc": lay.keys, "vc": lay.values}
        b = {
            "attn": blk.self_attn, "n1": blk.input_layernorm, "n2": blk.post_attention_layernorm,
            "qkv": [_rec5(L) for L in (q, k, v)], "qkv_opts": _gopts((q, k, v)), "qkv_nbits": q.nbits, "qkv_gs": q.group_size,
            "o": o, **kv, "len": lay.cumulative_length,
            # outputs of the launches (static addresses: the step is captured in a hipGraph)
            "q": torch.empty(B, q.out_features, dtype=dt, device=dev), "k": torch.empty(B, k.out_features, dtype=dt, device=dev),
            "v": torch.empty(B, v.out_features, dtype=dt, device=dev), "qr": torch.empty(B, self.n_heads, 1, self.hd, dtype=dt, device=dev),
        }
        if self.moe:   # the router's weight and the experts' stacks in place; idx / weights / a are this block's own (static addresses under graph capture)
            from ..core.quantize import Quantizer
            gate, ex = blk.mlp.gate, blk.mlp.experts
            kk = int(gate.top_k)
            b.update({
                "router": gate.weight, "top_k": kk, "renorm": bool(getattr(gate, "norm_topk_prob", True)), "round_w": self.variant.family == "qwen3_moe",
                "ex": [(getattr(ex, r + "_W_q"), getattr(ex, r + "_scale"), getattr(ex, r + "_zero")) for r in ("gate", "up", "down")],
                "ex_dims": (ex.num_experts, ex.hidden_dim, ex.intermediate_dim, ex.layer_meta["gate"]["group_size"], Quantizer._packing_bits[ex.layer_meta["gate"]["packing"]]),
                "idx": torch.zeros(B, kk, dtype=torch.int64, device=dev), "w": torch.zeros(B, kk, dtype=torch.float32, device=dev),
                "a": torch.empty(B, kk, ex.intermediate_dim, dtype=dt, device=dev),
            })
        else:
            b.update({
                "gu_gs": g.group_size, "gu": [_rec5(L) for L in (g, u)], "gu_opts": _gopts((g, u)), "gu_nbits": g.nbits, "d": d,
                "g": torch.empty(B, g.out_features, dtype=dt, device=dev), "u": torch.empty(B, u.out_features, dtype=dt, device=dev),
                "a": torch.empty(B, g.out_features, dtype=dt, device=dev),
            })
        if self.lora:   # per group: the adapted members as (index within the group, A, B, scaling) — the tensors themselves (static addresses under graph capture)
            for name, lo, hi in LORA_GROUPS:
                if self.lora_bank is not None:   # (index, A [n, K, r], B [n, r, N], scaling fp32 [n]): the bank's tensors in the wrappers' place
                    b["lora_" + name] = [(i,) + tuple(self.lora_bank.layer(w.name)) for i, w in enumerate(wrs[lo:hi]) if w is not None]
                    continue
                b["lora_" + name] = [(i, w.lora_A.data, w.lora_B.data, w._scaling_float()) for i, w in enumerate(wrs[lo:hi]) if w is not None]
        if self.qkv_bias:   # the three layers' own bias tensors (static addresses under graph capture); the launch records above stay bias-free
            b["qkv_bias"] = (q.bias, k.bias, v.bias)
        b.update(self._choose(bool(b.get("lora_gu"))))
        if b["qkv_stage"] is S._qkv_folded_rope:
            # q and k in the rotary-paired row order (ops.rotary_pair_layout): the q|k|v launch's epilogue applies the rotary embedding and writes the cache
            # (the kernel attention folds the rotary embedding into the attention launch instead: it keeps the natural order)
            qp, kp = (ops.rotary_pair_layout(_rec(L), L.in_features, L.group_size, L.nbits, self.hd, w3s=L.w3s) for L in (q, k))
            b["qkv_rope"] = [qp, kp, _rec(v)]
            b["qkv_rope_opts"] = _opts(_relaid_scalable(dt, qp, q) and _relaid_scalable(dt, kp, k) and bool(v.opts & ops.OPT_META_SCALABLE), q.w3s)
        if b["mlp_stage"] is S._mlp_folded:
            # gate|up as ONE paired layer: a packed row holds gate row n and up row n (ops.pair_layers); the layers' own tensors stay as they are
            pair = ops.pair_layers(_rec(g), _rec(u), g.in_features, g.group_size, g.nbits, w3s=g.w3s)
            b["gu_pair"], b["gu_pair_opts"] = [pair], _opts(_relaid_scalable(dt, pair, g), g.w3s)
            b["o_rec"], b["o_opts"], b["d_rec"], b["d_opts"] = [_rec(o)], ops.layer_opts(o.opts), [_rec(d)], ops.layer_opts(d.opts)
        return b

    def _buffers(self, glue: str) -> None:
        """the step's own buffers (static addresses: the step is captured in a hipGraph), the rotary tables and what the front of a call is"""
        inner, cfg, B, dt, dev = self.inner, self.model.config, self.B, self.dt, self.device
        # ONE adapter workspace for the whole step, sized for its largest group (the groups run one after the other on one stream)
        groups = [ad for b in self.blocks for name, _, _ in LORA_GROUPS if (ad := b.get("lora_" + name))]
        lora_ws_bytes = max((ops.lora_decode_workspace_bytes(B, ad[0][1].shape[-2], [a[1].shape[-1] for a in ad]) for ad in groups), default=0)
        self.lora_ws = torch.empty(lora_ws_bytes, dtype=torch.uint8, device=dev) if self.lora else None
        # with a bank: the adapter of every row, read by the routed kernels on the device (-1: none)
        self.slots = torch.full((B,), -1, dtype=torch.int64, device=dev) if self.lora_bank is not None else None
        self.h = torch.empty(B, self.H, dtype=dt, device=dev)       # the residual stream
        self.xn = torch.empty(B, self.H, dtype=dt, device=dev)      # its normalised copy, input of the next linears
        self.delta = torch.empty(B, self.H, dtype=dt, device=dev)   # output of o / down, added by the next add_rmsnorm
        self.att = torch.empty(B, self.n_heads * self.hd, dtype=dt, device=dev)   # attention output (attention="hip")
        self.attn_ws = {}                                                          # splits -> record buffer of the split attention launches
        # the causal mask of one query per sequence over the static cache, in the additive form SDPA turns a boolean mask into on every call
        # (where(mask, 0, -inf) in the query dtype): built once per token here instead of once per decoder block inside the attention function
        self.mask = torch.zeros(B, 1, 1, self.L, dtype=dt, device=dev)
        # what the front of a call fills of it: nothing for the kernel attention, which masks by position itself (and shares a head's keys out over `splits` workgroups)
        self._mask_rows = None if self.attention == "hip" else self.mask.view(B, -1)
        self.ar = torch.arange(self.L, device=dev)
        # cos / sin of every cache position, from the model's own rotary module called once (elementwise in the position: the rows equal what a
        # per-token call returns); rope types whose frequencies depend on the sequence length ("dynamic", "longrope") keep the per-token call
        self.cos_tab = self.sin_tab = None
        if getattr(inner.rotary_emb, "rope_type", "default") in ("default", "linear", "llama3", "yarn") and \
                self.L <= getattr(cfg, "max_position_embeddings", self.L):
            with torch.no_grad():
                c, s_ = inner.rotary_emb(torch.empty(1, 1, self.H, dtype=dt, device=dev), self.ar.view(1, -1))
            self.cos_tab, self.sin_tab = c[0].contiguous(), s_[0].contiguous()   # [max_cache_len, hd]
        self.zero = torch.zeros((), dtype=dt, device=dev)
        self.ninf = torch.full((), float("-inf"), dtype=dt, device=dev)
        # the front of a step as one launch (ops.token_prologue_batched) where it is a plain table lookup: an ordinary nn.Embedding in the compute dtype and
        # precomputed rotary tables.  glue="kernels" on an axis-1 model is the comparison leg that keeps the separate front.
        emb = inner.embed_tokens
        self.one_launch_front = bool((glue != "kernels" or self.axis0) and self.cos_tab is not None and type(emb) is torch.nn.Embedding and emb.max_norm is None and emb.weight.dtype == dt
                                     and emb.weight.is_contiguous() and emb.weight.device == self.h.device and self.H % 8 == 0 and dt in (torch.float16, torch.bfloat16))
        self.cos_v = torch.empty(B, self.hd, dtype=dt, device=dev)
        self.sin_v = torch.empty(B, self.hd, dtype=dt, device=dev)

    @torch.no_grad()
    def __call__(self, tok: Tensor, pos: Tensor, kv_len: int | None = None) -> Tensor:
        """tok [B, 1] int64, pos [B] int64 (each sequence's position; both on the device) -> logits [B, vocab] of the next tokens.
        kv_len (host integer > the LARGEST position, default the whole cache): HF's attention function attends over the first kv_len cache positions only
        (each row masked beyond its own position) — its cost follows the length it is given, so a caller that knows the positions passes a bucket just
        above them; the kernel attention takes its split count from it"""
        c = self._front(tok, pos, kv_len)
        for b in self.blocks:   # (the stages _choose picked when the step was built)
            b["qkv_stage"](self, b, c)
            b["mlp_stage"](self, b, c, b["attend_stage"](self, b, c))
        ops.add_rmsnorm(self.h, c.delta, self.inner.norm.weight, self.inner.norm.variance_epsilon, out=self.xn)
        return self.model.lm_head(self.xn)

    def _front(self, tok: Tensor, pos: Tensor, kv_len):
        """the residual stream's first rows, and what the stages of this call share: cos / sin of the rows' positions, pos, the attended length kvl with the
        mask's slice over it, the attention's split count, and delta — what the next add_rmsnorm has to add to h (None: nothing yet, or added already)"""
        inner, B, h = self.inner, self.B, self.h
        # (the positions themselves are device memory — the step is graph-replayed —: the kernels that index the cache with them skip their
        #  writes beyond the cache's last slot, csrc/block.hip; callers that know the positions on the host check them there, generation.py)
        if self.one_launch_front:   # embedding rows, rotary table rows and the causal masks in ONE launch (csrc/block.hip: copies and compares, the same bits as the ops below)
            ops.token_prologue_batched(tok, pos, inner.embed_tokens.weight, h, self.cos_tab, self.sin_tab, self.cos_v, self.sin_v, self._mask_rows)
            cos, sin = self.cos_v, self.sin_v
        else:
            h.copy_(inner.embed_tokens(tok).view(B, self.H))
            if self.cos_tab is not None:
                cos, sin = self.cos_tab.index_select(0, pos), self.sin_tab.index_select(0, pos)
            else:
                cos, sin = inner.rotary_emb(h.view(B, 1, self.H), pos.view(B, 1))   # [B, 1, hd] each, the model's own rotary module
                cos, sin = cos.reshape(B, -1).contiguous(), sin.reshape(B, -1).contiguous()
            if self._mask_rows is not None:
                torch.where(self.ar.view(1, -1) <= pos.view(-1, 1), self.zero, self.ninf, out=self._mask_rows)   # the causal mask of one query per row at its `pos`
        kvl = self.L if kv_len is None else min(int(kv_len), self.L)
        # (kernel attention: kv_len only picks how many workgroups share a head — or, grouped, a KV group — 's keys)
        splits = 1 if self._mask_rows is not None else ops.attn_gqa_splits(kvl, B, self.n_kv) if self.gqa_attention == "group" else ops.attn_splits(kvl)
        if splits > 1 and splits not in self.attn_ws:
            self.attn_ws[splits] = ops.attn_workspace_batched(self.device, B, self.n_heads, self.hd, splits)
        return SimpleNamespace(cos=cos, sin=sin, pos=pos, kvl=kvl, mask=self.mask[..., :kvl], splits=splits, delta=None)

    # ---- the q|k|v stage (b: the block's record, c: _front's) -----------------------------------------------------------------------------------------------
    def _qkv_folded_rope(self, b, c) -> None:   # RMSNorm in the prologue, rotary embedding + cache write in the epilogue: q|k|v lands rotated in qr / the caches
        ops.gemv_block(self.h, b["n1"].weight, b["n1"].variance_epsilon, b["qkv_rope"], self.H, b["qkv_gs"], b["qkv_nbits"], [b["qr"], b["kc"], b["vc"]],
                       ops.BLOCK_NORM | ops.BLOCK_ROPE, opts=b["qkv_rope_opts"], rope=(c.cos, c.sin, c.pos, self.hd, self.L))

    def _qkv_folded(self, b, c) -> None:   # RMSNorm in the launch's prologue: every workgroup normalises h itself while its first weights are in flight
        ops.gemv_block(self.h, b["n1"].weight, b["n1"].variance_epsilon, b["qkv"], self.H, b["qkv_gs"], b["qkv_nbits"], [b["q"], b["k"], b["v"]], ops.BLOCK_NORM, opts=b["qkv_opts"])

    def _qkv_kernels(self, b, c) -> None:
        ops.add_rmsnorm(self.h, c.delta, b["n1"].weight, b["n1"].variance_epsilon, out=self.xn)
        b["grouped"](self, b, "qkv", [b["q"], b["k"], b["v"]])
        self._adapters(b, "qkv", self.xn, [b["q"], b["k"], b["v"]])

    # ---- the rotary / cache / attention stage -> the attention's output ---------------------------------------------------------------------------------------
    def _attend_kvq(self, b, c) -> Tensor:   # rotary + quantised cache write, then the attention on the packed rows
        ops.rope_kvq_cache_batched(b["q"], b["k"], b["v"], c.cos, c.sin, c.pos, b["kvq"], b["qr"])
        return ops.attn_decode_kvq_batched(b["qr"], b["kvq"], c.pos, self.att, b["attn"].scaling, self.hd, splits=c.splits, workspace=self.attn_ws.get(c.splits))

    def _attend_kvq_gqa(self, b, c) -> Tensor:   # the same two launches, the attention per KV-head group
        ops.rope_kvq_cache_batched(b["q"], b["k"], b["v"], c.cos, c.sin, c.pos, b["kvq"], b["qr"])
        return ops.attn_decode_gqa_kvq_batched(b["qr"], b["kvq"], c.pos, self.att, b["attn"].scaling, self.hd, splits=c.splits, workspace=self.attn_ws.get(c.splits))

    def _attend_verify(self, b, c) -> Tensor:   # the rows are positions of one sequence: all of their keys / values into its cache first, then row i over keys [0, pos[i]]
        ops.rope_cache_shared(b["q"], b["k"], b["v"], c.cos, c.sin, c.pos, b["kc"], b["vc"], b["qr"])
        return self._verify_attn(b["qr"], b["kc"], b["vc"], c.pos, self.att, b["attn"].scaling, splits=c.splits, workspace=self.attn_ws.get(c.splits))

    def _attend_rope_attn(self, b, c) -> Tensor:   # rotary + cache write + attention: one launch
        return ops.rope_attn_decode_batched(b["q"], b["k"], b["v"], c.cos, c.sin, c.pos, b["kc"], b["vc"], self.att, b["attn"].scaling, splits=c.splits,
                                            workspace=self.attn_ws.get(c.splits))

    def _rotary(self, b, c) -> None:   # the family's rotary-and-cache launch; either attention then reads the rotated qr
        getattr(ops, self._rope_cache)(b["q"], b["k"], b["v"], *self._rope_extra(b), c.cos, c.sin, c.pos, b["kc"], b["vc"], b["qr"])

    def _attend_rotary_hip(self, b, c) -> Tensor:
        self._rotary(b, c)
        return ops.attn_decode_batched(b["qr"], b["kc"], b["vc"], c.pos, self.att, b["attn"].scaling, splits=c.splits, workspace=self.attn_ws.get(c.splits))

    def _attend_rotary_gqa(self, b, c) -> Tensor:   # every family, the llama family too: the grouped kernel has no rotary-fused form
        self._rotary(b, c)
        return ops.attn_decode_gqa_batched(b["qr"], b["kc"], b["vc"], c.pos, self.att, b["attn"].scaling, splits=c.splits, workspace=self.attn_ws.get(c.splits))

    def _attend_rotary_sdpa(self, b, c) -> Tensor:
        self._rotary(b, c)
        return self._attend_sdpa(b, c)

    def _attend_sdpa(self, b, c) -> Tensor:   # (alone where the q|k|v epilogue has rotated and cached already)
        return self.attn_fn(b["attn"], b["qr"], b["kc"][:, :, :c.kvl], b["vc"][:, :, :c.kvl], c.mask, dropout=0.0, scaling=b["attn"].scaling)[0]

    # ---- the o / MLP stage (att: the attention's output) ------------------------------------------------------------------------------------------------------
    def _mlp_folded(self, b, c, att) -> None:
        # o: h += o(att) in the epilogue; gate|up: RMSNorm prologue + silu(gate) * up epilogue on the paired layer; down: h += down(a) in the epilogue
        o, d = b["o"], b["d"]
        ops.gemv_block(att.reshape(1, -1), None, 0.0, b["o_rec"], o.in_features, o.group_size, o.nbits, [self.h], ops.BLOCK_RESID, opts=b["o_opts"])
        ops.gemv_block(self.h, b["n2"].weight, b["n2"].variance_epsilon, b["gu_pair"], self.H, b["gu_gs"], b["gu_nbits"], [b["a"]], ops.BLOCK_NORM | ops.BLOCK_SILU, opts=b["gu_pair_opts"])
        ops.gemv_block(b["a"], None, 0.0, b["d_rec"], d.in_features, d.group_size, d.nbits, [self.h], ops.BLOCK_RESID, opts=b["d_opts"])

    def _o_kernels(self, b, att) -> None:
        """self.delta = o(att) + its adapter terms; h += that, and self.xn = the MLP's normalised input"""
        xo = att.reshape(self.B, -1)
        b["single"](self, xo, b["o"])
        self._adapters(b, "o", xo, [self.delta])     # before the residual add (the next add_rmsnorm)
        ops.add_rmsnorm(self.h, self.delta, b["n2"].weight, b["n2"].variance_epsilon, out=self.xn)

    def _down_kernels(self, b, c) -> None:
        b["single"](self, b["a"], b["d"])
        self._adapters(b, "d", b["a"], [self.delta])
        c.delta = self.delta

    def _mlp_moe(self, b, c, att) -> None:   # the router fills the block's idx / weights, the two expert launches read them on the device; self.delta = the routed MLP's output
        self._o_kernels(b, att)
        ops.moe_router(self.xn, b["router"], b["top_k"], b["renorm"], b["round_w"], idx=b["idx"], weights=b["w"])
        ops.moe_gate_up(self.xn, b["idx"], b["ex"][0], b["ex"][1], *b["ex_dims"], a=b["a"])
        ops.moe_down(b["a"], b["idx"], b["w"], b["ex"][2], *b["ex_dims"], out=self.delta)
        c.delta = self.delta

    def _mlp_silu_in_reduce(self, b, c, att) -> None:   # SiLU * up rides in the grouped launch's reduce: no silu_mul launch
        self._o_kernels(b, att)
        b["grouped"](self, b, "gu", [b["a"]], flags=ops.BLOCK_SILU)
        self._down_kernels(b, c)

    def _mlp_kernels(self, b, c, att) -> None:   # (an adapted gate | up of an axis-0 model too: the adapter terms come before SiLU)
        self._o_kernels(b, att)
        b["grouped"](self, b, "gu", [b["g"], b["u"]])
        self._adapters(b, "gu", self.xn, [b["g"], b["u"]])
        ops.silu_mul(b["g"], b["u"], out=b["a"])
        self._down_kernels(b, c)

    # ---- the launches of the unfolded stages: q|k|v ("qkv") or gate|up ("gu") of block b on the normalised rows self.xn as one grouped launch on the layers'
    # own tensors; o or down as self.delta = L(x), added to the residual stream by the next add_rmsnorm ----------------------------------------------------------
    def _grouped_axis0(self, b, which: str, outs, flags: int = 0) -> None:
        ops.gemv_axis0_grouped(self.xn, b[which], self.H, b[which + "_gs"], b[which + "_nbits"], outs=outs, flags=flags)

    def _grouped_axis1(self, b, which: str, outs) -> None:
        ops.gemv_grouped(self.xn, b[which], self.H, b[which + "_gs"], b[which + "_nbits"], outs=outs, opts=b[which + "_opts"])

    def _single_axis0(self, x: Tensor, L) -> None:
        ops.gemv_axis0(x, L.W_q, L.scale, L.zero, None, L.out_features, L.in_features, L.group_size, L.nbits, out=self.delta)

    def _single_axis1(self, x: Tensor, L) -> None:
        ops.gemv(x, L.W_q, L.scale, L.zero, None, L.out_features, L.in_features, L.group_size, L.nbits, out=self.delta, opts=ops.layer_opts(L.opts))

    def _adapters(self, b, which: str, x: Tensor, ys) -> None:
        """the adapter terms of group `which` of block b added to the base launch's outputs ys, on the rows x that launch read: one lora_shrink + one
        lora_expand over the adapted members; nothing where the group has none (or the step serves no adapters).  With a bank: the routed pair on the bank's
        tensors, every row under the adapter self.slots names for it"""
        ad = b.get("lora_" + which)
        if not ad:
            return
        if self.lora_bank is not None:
            ops.lora_shrink_routed(x, [a[1] for a in ad], self.slots, self.lora_ws)
            ops.lora_expand_routed(self.lora_ws, [a[2] for a in ad], [a[3] for a in ad], self.slots, [ys[a[0]] for a in ad], x.shape[-1])
            return
        ops.lora_shrink(x, [a[1] for a in ad], self.lora_ws)
        ops.lora_expand(self.lora_ws, [a[2] for a in ad], [a[3] for a in ad], [ys[a[0]] for a in ad], x.shape[-1])

    def account_tokens(self, n: int) -> None:
        """StaticLayer.update's bookkeeping for the n tokens the fused steps appended (kept out of the captured step: one add per layer).  For the
        single-sequence caller: the rows of a batch have different lengths, and nothing reads a B-row cache's cumulative_length"""
        for b in self.blocks:
            b["len"].add_(n)


class FusedLlamaBatchStep(FusedLlamaStep):
    """FusedLlamaStep under the name and positional signature the batched callers construct it by: no `glue` argument ("auto": the one-launch front
    wherever the tables exist)"""

    def __init__(self, model, cache, max_cache_len: int, batch: int, attention: str = "sdpa", axis0: bool = False, qk_norm: bool = False, qkv_bias: bool = False,
                 lora: bool = False, moe: bool = False, kv_cache: str | None = None, lora_bank=None, gqa_attention: str = "heads"):
        super().__init__(model, cache, max_cache_len, attention=attention, axis0=axis0, batch=batch, qk_norm=qk_norm, qkv_bias=qkv_bias, lora=lora, moe=moe,
                         kv_cache=kv_cache, lora_bank=lora_bank, gqa_attention=gqa_attention)
