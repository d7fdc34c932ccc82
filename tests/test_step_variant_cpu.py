"""CPU side of the decode step's model variant (hqq_amd.utils.llama_fused): which architectures the three predicates accept, knob by knob; the precedence by
which resolve() picks a variant; and which flag combinations are a variant at all.  Tiny randomly initialised HF models: 2 blocks, hidden size 64."""
import inspect
import itertools

import pytest
import torch

FLAGS = ("axis0", "qk_norm", "qkv_bias", "lora")
# the six served combinations of (axis0, qk_norm, qkv_bias, lora), in resolve()'s order of precedence
SERVED = [(0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (1, 0, 0, 1)]


def _classes(kind):
    import transformers as tf
    return {"llama": (tf.LlamaConfig, tf.LlamaForCausalLM), "mistral": (tf.MistralConfig, tf.MistralForCausalLM),
            "qwen2": (tf.Qwen2Config, tf.Qwen2ForCausalLM), "qwen3": (tf.Qwen3Config, tf.Qwen3ForCausalLM)}[kind]


def _tiny(kind, **kw):
    Config, Model = _classes(kind)
    torch.manual_seed(0)
    args = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=2, vocab_size=64, max_position_embeddings=64)
    if kind == "mistral":
        args["sliding_window"] = None   # (MistralConfig's default is a window of 4096, which no predicate takes: the base case is a full-attention Mistral)
    args.update(kw)
    return Model(Config(**args))


def _multiplier(m):
    m.config.residual_multiplier = 0.5   # Granite's config field: none of the four classes has it, the predicates read it off any config


def _leave_window_on_config(m):
    m.config.sliding_window = 16   # with use_sliding_window off and full attention in every layer: what Qwen2 checkpoints' configs carry


def _graft_q_norm(m):
    m.model.layers[0].self_attn.q_norm = torch.nn.Identity()


def _drop_k_bias(m):
    m.model.layers[1].self_attn.k_proj.bias = None


# knob -> (config keywords, applied to the classes whose __init__ names every one of them; edit of the built model; the kinds the edit is for)
KNOBS = {
    "none": ({}, None, ()),
    "sliding_window": (dict(sliding_window=16), None, ()),
    "window_left_on_config": ({}, _leave_window_on_config, ("llama", "mistral", "qwen2", "qwen3")),
    "use_sliding_window": (dict(use_sliding_window=True), None, ()),
    "layer_types": (dict(layer_types=["full_attention", "sliding_attention"]), None, ()),
    "attention_bias": (dict(attention_bias=True), None, ()),
    "mlp_bias": (dict(mlp_bias=True), None, ()),
    "gelu": (dict(hidden_act="gelu"), None, ()),
    "multiplier": ({}, _multiplier, ("llama", "mistral", "qwen2", "qwen3")),
    "q_norm_grafted": ({}, _graft_q_norm, ("llama", "mistral", "qwen2")),
    "k_bias_removed": ({}, _drop_k_bias, ("qwen2",)),
}

# (arch_supported, qk_norm_arch_supported, qkv_bias_arch_supported) of every case below, recorded by running this table on the commit BEFORE the three
# predicates were given one body (transformers 5.15): the refactor changes none of them.  A knob is absent where the config class does not take it.
L, Q3, Q2, NO = (True, False, False), (False, True, False), (False, False, True), (False, False, False)
EXPECTED = {
    ("llama", "none"): L,
    ("llama", "window_left_on_config"): NO,
    ("llama", "attention_bias"): NO,
    ("llama", "mlp_bias"): NO,
    ("llama", "gelu"): NO,
    ("llama", "multiplier"): NO,
    ("llama", "q_norm_grafted"): NO,
    ("mistral", "none"): L,
    ("mistral", "sliding_window"): NO,
    ("mistral", "window_left_on_config"): NO,
    ("mistral", "gelu"): NO,
    ("mistral", "multiplier"): NO,
    ("mistral", "q_norm_grafted"): NO,
    ("qwen2", "none"): Q2,
    ("qwen2", "sliding_window"): Q2,
    ("qwen2", "window_left_on_config"): Q2,
    ("qwen2", "use_sliding_window"): Q2,
    ("qwen2", "layer_types"): NO,
    ("qwen2", "gelu"): NO,
    ("qwen2", "multiplier"): NO,
    ("qwen2", "q_norm_grafted"): NO,
    ("qwen2", "k_bias_removed"): NO,
    ("qwen3", "none"): Q3,
    ("qwen3", "sliding_window"): Q3,
    ("qwen3", "window_left_on_config"): NO,
    ("qwen3", "use_sliding_window"): NO,
    ("qwen3", "layer_types"): NO,
    ("qwen3", "attention_bias"): NO,
    ("qwen3", "gelu"): NO,
    ("qwen3", "multiplier"): NO,
}


def _cases():
    for kind in ("llama", "mistral", "qwen2", "qwen3"):
        accepted = inspect.signature(_classes(kind)[0].__init__).parameters
        for knob, (kw, edit, kinds) in KNOBS.items():
            if all(k in accepted for k in kw) and (edit is None or kind in kinds):
                yield kind, knob


def _triple(kind, knob):
    from hqq_amd.utils import llama_fused
    kw, edit, _ = KNOBS[knob]
    m = _tiny(kind, **kw)
    if edit is not None:
        edit(m)
    return llama_fused.arch_supported(m), llama_fused.qk_norm_arch_supported(m), llama_fused.qkv_bias_arch_supported(m)


def test_the_table_covers_every_case_the_installed_config_classes_allow():
    assert set(_cases()) == set(EXPECTED)


@pytest.mark.parametrize("kind,knob", sorted(EXPECTED))
def test_architecture_predicates_knob_by_knob(kind, knob):
    assert _triple(kind, knob) == EXPECTED[kind, knob]


def _chain(opted, ok):
    """GraphedGreedyDecoder.__init__'s if-chain as it stood before resolve() (fused=True), over plain booleans: `opted` the keywords set to "fused", ok[flags]
    what the supports_* function of that combination answers.  Returns the (axis0, qk_norm, qkv_bias, lora) the step was then built with, or None."""
    axis0, qk_norm, qkv_bias, lora = (f in opted for f in FLAGS)
    fused = ok[0, 0, 0, 0]
    fused_axis0 = axis0 and not fused and ok[1, 0, 0, 0]
    fused_qk_norm = qk_norm and not fused and not fused_axis0 and ok[0, 1, 0, 0]
    fused_qkv_bias = qkv_bias and not fused and not fused_axis0 and not fused_qk_norm and ok[0, 0, 1, 0]
    fused_lora, lora_axis0 = False, False
    if lora and not (fused or fused_axis0 or fused_qk_norm or fused_qkv_bias):
        if ok[0, 0, 0, 1]:
            fused_lora = True
        elif axis0 and ok[1, 0, 0, 1]:
            fused_lora = lora_axis0 = True
    if not (fused or fused_axis0 or fused_qk_norm or fused_qkv_bias or fused_lora):
        return None
    return (int(fused_axis0 or lora_axis0), int(fused_qk_norm), int(fused_qkv_bias), int(fused_lora))


def test_resolve_follows_the_decoders_former_precedence(monkeypatch):
    from hqq_amd.utils import llama_fused
    model, supported, asked = object(), set(), []

    def fake(m, variant, batch=None):
        assert m is model
        asked.append(batch)
        return tuple(int(variant.flags()[f]) for f in FLAGS) in supported

    monkeypatch.setattr(llama_fused, "variant_supported", fake)
    for n_opt in range(5):
        for opted in itertools.combinations(FLAGS, n_opt):
            for bits in itertools.product((False, True), repeat=len(SERVED)):
                supported.clear()
                supported.update(s for s, on in zip(SERVED, bits) if on)
                want = _chain(opted, {s: s in supported for s in SERVED})
                got = llama_fused.resolve(model, set(opted))
                assert (None if got is None else tuple(int(got.flags()[f]) for f in FLAGS)) == want, (opted, sorted(supported))
    assert set(asked) == {None}
    supported.update(SERVED)
    asked.clear()
    assert llama_fused.resolve(model, set(), 3) == llama_fused.StepVariant() and asked == [3]   # the batch goes through to variant_supported


def test_exactly_six_flag_combinations_are_a_variant():
    from hqq_amd.utils.llama_fused import StepVariant
    built = []
    for combo in itertools.product((0, 1), repeat=4):
        flags = dict(zip(FLAGS, map(bool, combo)))
        if combo in SERVED:
            v = StepVariant.from_flags(**flags)
            assert v.flags() == flags and StepVariant.from_flags(**v.flags()) == v
            assert StepVariant(v.family, v.axis0, v.lora) == v and hash(v) == hash(StepVariant.from_flags(**flags))
            built.append(v)
        else:
            with pytest.raises(ValueError):
                StepVariant.from_flags(**flags)
    assert len(set(built)) == 6
    assert StepVariant() == StepVariant.from_flags() and StepVariant().family == "llama"
    assert {v.family for v in built} == {"llama", "qwen3", "qwen2"}
    with pytest.raises(Exception):   # frozen
        built[0].axis0 = True
    for family in ("qwen3", "qwen2"):   # only Llama / Mistral admit axis 0 or adapters, however the variant is built
        for kw in (dict(axis0=True), dict(lora=True)):
            with pytest.raises(ValueError):
                StepVariant(family, **kw)
    with pytest.raises(ValueError):
        StepVariant("granite")
