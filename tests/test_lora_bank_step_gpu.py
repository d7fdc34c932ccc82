"""GPU tests of several LoRA adapters served over one quantised base: FusedLlamaStep(lora=True, lora_bank=bank), GraphedGreedyDecoder / HFGenerator with
lora_bank= and the adapter / adapters keywords, on tiny adapted Llamas of their own (2 blocks, hidden 64, one head of 64, vocabulary 512, int4, group_size 64, a
cache of 64 positions; three adapters whose lora_B is random and far from zero).

The reference of every comparison is code that exists without the bank — bank.activate(model, a) puts adapter a into the wrappers, then the one-adapter
FusedLlamaStep / GraphedGreedyDecoder(lora="fused") / default route runs — and every comparison is exact: the routed launches give each row the bits of the
one-adapter launches with its adapter, the other launches are the same, and the rows of a batch are independent of each other."""
import functools

import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

CACHE, VOCAB, N_ADAPTERS = 64, 512, 3
ATTN, MLP = ("q_proj", "k_proj", "v_proj", "o_proj"), ("gate_proj", "up_proj", "down_proj")


def _build(axis):
    """(the adapted, patched model; the three adapters as {module_name: state_dict} dictionaries on the CPU)"""
    from transformers import LlamaConfig, LlamaForCausalLM
    from hqq_amd.backends.hip import group_llama_projections
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    from hqq_amd.core.quantize import BaseQuantizeConfig
    from hqq_amd.utils.model import quantize_model
    from hqq_amd.utils.patching import prepare_for_inference
    torch.manual_seed(0)
    cfg = LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1, num_key_value_heads=1, vocab_size=VOCAB,
                      max_position_embeddings=128)
    model = LlamaForCausalLM(cfg).half().cuda().eval()
    quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=axis), compute_dtype=torch.float16, device="cuda")
    peft = {f"self_attn.{n}": {"r": 8, "lora_alpha": 16, "dropout": 0.0} for n in ATTN}
    peft.update({f"mlp.{n}": {"r": 4, "lora_alpha": 16, "dropout": 0.0} for n in MLP})
    PeftUtils.add_lora(model, peft)
    prepare_for_inference(model, backend="hip")
    if axis == 1:
        group_llama_projections(model)
    g = torch.Generator().manual_seed(7)
    adapters = []
    for a in range(N_ADAPTERS):
        params = {}
        for name, m in model.named_modules():
            if is_hqq_lora_layer(m):
                params[name] = {"lora_A": torch.randn(m.lora_A.shape, generator=g) / m.in_features ** 0.5, "lora_B": 0.3 * torch.randn(m.lora_B.shape, generator=g),
                                "scaling": 2.0 + 0.5 * a, "bias": None}
        adapters.append(params)
    return model.eval(), adapters


@functools.lru_cache(maxsize=None)
def _world(axis):
    """(axis, model, bank, adapters, the decoder keywords that opt the model into the fused lora step) — built once per axis.  The tests rewrite the
    wrappers through bank.activate and nothing else; each activates what it needs before it reads them"""
    from hqq_amd.core.peft import LoRABank
    model, adapters = _build(axis)
    bank = LoRABank.from_params(model, adapters)
    kw = dict(lora="fused", axis0="fused") if axis == 0 else dict(lora="fused")
    return axis, model, bank, adapters, kw


@pytest.fixture(params=[1, 0], ids=["axis1", "axis0"])
def world(request):
    return _world(request.param)


@pytest.fixture()
def axis1():
    return _world(1)


def _prompts(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, VOCAB, (1, T), generator=g).cuda() for T in lengths]


def _teacher_forced(model, bank, prompts, slots, forced, axis0, with_bank, uniform=None):
    """logits [steps, B, vocab] of a B-row step fed forced[b]'s tokens after prompt b.  Prompt b is prefilled under adapter slots[b] into a fresh B-row cache (the
    same cache contents for every run).  with_bank: the step reads the bank, rows routed by `slots`; else: the one-adapter step, built after
    bank.activate(model, uniform)"""
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep
    cfg, B = model.config, len(prompts)
    bc = StaticCache(config=cfg, max_cache_len=CACHE)
    bc.early_initialization(B, cfg.num_key_value_heads, cfg.hidden_size // cfg.num_attention_heads, torch.float16, torch.device("cuda"))
    for b, x in enumerate(prompts):
        bank.activate(model, slots[b])
        c = StaticCache(config=cfg, max_cache_len=CACHE)
        with torch.no_grad():
            model(x, past_key_values=c, cache_position=torch.arange(x.shape[1], device="cuda"), use_cache=True)
        for dst, src in zip(bc.layers, c.layers):
            dst.keys[b, :, :x.shape[1]].copy_(src.keys[0, :, :x.shape[1]])
            dst.values[b, :, :x.shape[1]].copy_(src.values[0, :, :x.shape[1]])
    if with_bank:
        step = FusedLlamaBatchStep(model, bc, CACHE, B, axis0=axis0, lora=True, lora_bank=bank)
        assert step.slots.dtype == torch.int64 and tuple(step.slots.shape) == (B,) and step.slots.is_cuda and bool((step.slots == -1).all())
        step.slots.copy_(torch.tensor(slots, dtype=torch.int64))
    else:
        bank.activate(model, uniform)
        step = FusedLlamaBatchStep(model, bc, CACHE, B, axis0=axis0, lora=True)
        assert step.lora_bank is None and step.slots is None
    T = [x.shape[1] for x in prompts]
    out = []
    for t in range(forced.shape[1]):
        tok = forced[:, t:t + 1].contiguous()
        pos = torch.tensor([T[b] + t for b in range(B)], device="cuda")
        out.append(step(tok, pos, CACHE).clone())
    return torch.stack(out)


def test_each_row_of_the_bank_step_has_the_logits_of_the_one_adapter_step(world):
    axis, model, bank, _, _ = world
    slots = [1, -1, 0]
    prompts = _prompts([3, 6, 9], 31)
    forced = torch.randint(0, VOCAB, (3, 4), generator=torch.Generator().manual_seed(32)).cuda()
    got = _teacher_forced(model, bank, prompts, slots, forced, axis == 0, True)
    assert bool(torch.isfinite(got.float()).all())
    for i, a in enumerate(slots):
        want = _teacher_forced(model, bank, prompts, slots, forced, axis == 0, False, uniform=a)
        assert torch.equal(got[:, i].view(torch.int16), want[:, i].view(torch.int16)), (i, a, float((got[:, i].float() - want[:, i].float()).abs().max()))


def test_adapters_are_not_ignored(world):
    """the same prompt and tokens in four rows under adapters 0, 1, 2 and none: the rows' logits all differ from each other, visibly"""
    axis, model, bank, _, _ = world
    slots = [0, 1, 2, -1]
    prompts = _prompts([5], 33) * 4
    forced = torch.randint(0, VOCAB, (1, 4), generator=torch.Generator().manual_seed(34)).cuda().repeat(4, 1)
    got = _teacher_forced(model, bank, prompts, slots, forced, axis == 0, True).float()
    for i in range(4):
        for j in range(i + 1, 4):
            d = float((got[:, i] - got[:, j]).abs().max())
            print(f"axis {axis}: max |logits under {slots[i]} - under {slots[j]}| = {d:.3f}")
            assert d > 0.05, (slots[i], slots[j], d)


def test_generate_batch_with_mixed_adapters_emits_todays_tokens_row_by_row(world):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    axis, model, bank, _, kw = world
    slots = [1, -1, 0]
    prompts = _prompts([3, 6, 9], 35)
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, lora_bank=bank, **kw)
    got = dec.generate_batch(prompts, 8, adapters=slots)
    st = dec._batch.get(3)
    assert st is not None and st["step"].lora_bank is bank and dec.batch_graphs, "the batched bank step served the batch, through captured graphs"
    assert st["step"].slots.tolist() == slots
    for i, a in enumerate(slots):
        bank.activate(model, a)
        ref = GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw)
        want = ref.generate_batch(prompts, 8)
        assert ref._batch.get(3) is not None and ref._batch[3]["step"].lora_bank is None
        assert torch.equal(got[i], want[i]), (i, a, got[i].tolist(), want[i].tolist())
    # another mix on the kept state: no rebuild, and the rows follow
    step, graphs = st["step"], dec.batch_graphs
    again = dec.generate_batch(prompts, 8, adapters=[-1, 0, 1])
    assert dec._batch[3]["step"] is step and dec.batch_graphs is graphs
    for i, a in enumerate([-1, 0, 1]):
        bank.activate(model, a)
        assert torch.equal(again[i], GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw).generate_batch(prompts, 8)[i]), (i, a)
    assert torch.equal(dec.generate_batch(prompts, 8)[1], got[1]), "adapters=None is the base model for every row"


def test_one_sequence_under_every_adapter_and_no_rebuild_in_between(world, tmp_path):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    axis, model, bank, adapters, kw = world
    x = _prompts([6], 36)[0]
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, lora_bank=bank, **kw)
    got = {}
    for a in (0, 2, -1, 1):
        got[a] = dec.generate(x, 10, adapter=a)
        if a == 0:
            step, graphs = dec.step, dec.graphs
            assert step is not None and step.lora_bank is bank and dec.fused_lora
        assert dec.step is step and dec.graphs is graphs and dec.graph is not None, "another adapter keeps the step and its graphs"
        assert dec.step.slots.tolist() == [a]
    assert torch.equal(dec.generate(x, 10), got[-1]), "adapter=None is the base model"
    for a in (-1, 0, 1, 2):
        bank.activate(model, a)
        ref = GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw)
        want = ref.generate(x, 10)
        assert ref.step is not None and ref.step.lora and ref.step.lora_bank is None
        assert torch.equal(got[a], want), (a, got[a].tolist(), want.tolist())
    assert len({tuple(t[0].tolist()) for t in got.values()}) > 1, "the adapters change the tokens"
    # bank.set in place: slot 2 now holds adapter 0 — its tokens, the same step, the same graphs
    f0 = str(tmp_path / "adapter0.pt")
    torch.save({"peft_config": model.peft_config, "parameters": adapters[0]}, f0)
    try:
        bank.set(2, f0)
        assert torch.equal(dec.generate(x, 10, adapter=2), got[0])
        assert dec.step is step and dec.graphs is graphs
    finally:
        bank.set(2, adapters[2])
    assert torch.equal(dec.generate(x, 10, adapter=2), got[2]) and dec.step is step


def test_the_composed_route_serves_the_bank_through_activate(axis1):
    """lora="model" (the default): no fused step, the same tokens as activate + today's default route, one prompt after another in a batch"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    _, model, bank, _, _ = axis1
    prompts = _prompts([4, 7], 37)
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, lora_bank=bank)
    assert not dec.fused_lora
    got = {a: dec.generate(prompts[0], 8, adapter=a) for a in (1, -1, 2)}
    assert dec.step is None and dec.graph is not None, "the composed route, through captured graphs (kept per set of scalings: the adapters' differ)"
    batch = dec.generate_batch(prompts, 8, adapters=[2, 0])
    assert not dec._batch
    for a in (1, -1, 2):
        bank.activate(model, a)
        assert torch.equal(got[a], GraphedGreedyDecoder(model, max_cache_len=CACHE).generate(prompts[0], 8)), a
    for i, a in enumerate([2, 0]):
        bank.activate(model, a)
        assert torch.equal(batch[i], GraphedGreedyDecoder(model, max_cache_len=CACHE).generate(prompts[i], 8)), (i, a)
    assert torch.equal(batch[0], got[2]) and not torch.equal(got[1], got[-1])


def test_keywords_and_banks_the_step_refuses(axis1):
    from transformers import StaticCache
    from hqq_amd.core.peft import LoRABank
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    _, model, bank, adapters, kw = axis1
    cache = StaticCache(config=model.config, max_cache_len=CACHE)
    with pytest.raises(ValueError, match="lora=True"):
        FusedLlamaStep(model, cache, CACHE, lora_bank=bank)
    with pytest.raises(ValueError, match="verify"):
        FusedLlamaStep(model, cache, CACHE, lora=True, lora_bank=bank, verify=True, batch=4, attention="hip")
    few = sorted(n for n in bank.names if "mlp" not in n)

    class Fewer:   # the bank's interface over a subset of the model's wrappers
        n, names = bank.n, few

        def layer(self, name):
            return bank.layer(name)

    with pytest.raises(ValueError, match="not exactly"):
        FusedLlamaStep(model, cache, CACHE, lora=True, lora_bank=Fewer())
    wide = LoRABank.from_params(model, [adapters[0]] * 2, dtype=torch.float64)   # an adapter dtype the kernels do not read
    with pytest.raises(ValueError, match="lora_routed_covers"):
        FusedLlamaStep(model, cache, CACHE, lora=True, lora_bank=wide)
    dec = GraphedGreedyDecoder(model, max_cache_len=CACHE, lora_bank=bank, **kw)
    x = _prompts([5], 38)[0]
    for bad in (3, -2, 1.0):
        with pytest.raises(ValueError, match="not an index into the bank"):
            dec.generate(x, 4, adapter=bad)
    with pytest.raises(ValueError, match="adapters for 2 prompts"):
        dec.generate_batch([x, x], 4, adapters=[0])
    with pytest.raises(ValueError, match="without one"):
        GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw).generate(x, 4, adapter=0)
    with pytest.raises(ValueError, match="without one"):
        GraphedGreedyDecoder(model, max_cache_len=CACHE, **kw).generate_batch([x, x], 4, adapters=[0, 1])


def test_hfgenerator_passes_the_keywords_on(axis1):
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator
    from test_model_gpu import _ToyTokenizer
    _, model, bank, _, kw = axis1
    gen = HFGenerator(model, _ToyTokenizer(), max_new_tokens=8, compile="partial", lora_bank=bank, **kw)
    assert gen.decoder.lora_bank is bank
    prompts = ["7 8 9 10 11", "400 3 77", "5 6 7 8 9 10"]
    one = {a: gen.generate(prompts[0], use_chat_template=False, verbose=False, adapter=a) for a in (2, 0)}
    assert gen.decoder.step is not None and gen.decoder.step.lora_bank is bank
    batch = gen.generate_batch(prompts, use_chat_template=False, verbose=False, adapters=[2, -1, 1])
    assert gen.decoder._batch.get(3) is not None and gen.decoder._batch[3]["step"].slots.tolist() == [2, -1, 1]
    assert not torch.equal(one[2]["output_tokens"], one[0]["output_tokens"])
    dec = GraphedGreedyDecoder(model, max_cache_len=gen.cache_size, lora_bank=bank, **kw)
    ids = [torch.tensor([[int(t) for t in p.split()]]).cuda() for p in prompts]
    for a in (2, 0):
        assert torch.equal(one[a]["output_tokens"], dec.generate(ids[0], 8, adapter=a)[0, ids[0].shape[1]:].cpu()), a
    for x, r, w in zip(ids, batch, dec.generate_batch(ids, 8, adapters=[2, -1, 1])):
        assert torch.equal(r["output_tokens"], w[0, x.shape[1]:].cpu()) and torch.equal(r["input_tokens"], x[0].cpu())
    with pytest.raises(ValueError, match="without one"):
        HFGenerator(model, _ToyTokenizer(), max_new_tokens=8, **kw).generate(prompts[0], use_chat_template=False, verbose=False, adapter=0)
