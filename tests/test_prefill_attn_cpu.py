"""Host-side checks of the prompt's causal attention (tests/_prefill_cases.py; csrc/attn_prefill.hip; GraphedGreedyDecoder(prefill_attention="hip")): the two
symbols and the ABI version, the case bed and its band condition on the CPU, the keyword's validation, the coverage rule, and the wrappers' shape errors."""
import os

import pytest

torch = pytest.importorskip("torch")

import _prefill_cases as pc  # noqa: E402
import _tile_cases as tc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_symbols_are_bound_and_the_abi_version_stays():
    from hqq_amd import _C
    lib = _C.lib()
    for name in ("hqq_hip_attn_prefill", "hqq_hip_attn_prefill_kvq"):
        assert name in _C.SYMBOLS and hasattr(lib, name), name
    assert _C.ABI_VERSION == 9 == lib.hqq_hip_abi_version()
    head = open(os.path.join(ROOT, "include", "hqq_hip.h")).read().split("int hqq_hip_attn_prefill(")[0][-3000:]
    assert "added without raising HQQ_HIP_ABI_VERSION" in head


def test_the_library_refuses_bad_arguments_before_it_touches_a_device():
    """the entries' own checks need no GPU: they come first, and nothing is launched after them"""
    from hqq_amd import _C
    lib = _C.lib()
    p = 4096   # (an aligned non-null address that is never dereferenced)

    def dense(pos0=0, T=16, L=64, qrs=256, qhs=64, hd=64, dtype=1, heads=(4, 4)):
        return lib.hqq_hip_attn_prefill(p, qrs, qhs, p, p, pos0, T, p, heads[0], heads[1], hd, L, 0.125, dtype, None)

    for kw in (dict(T=0), dict(T=-3), dict(pos0=-1), dict(pos0=49, T=16), dict(pos0=64, T=1), dict(T=65), dict(L=0)):
        assert dense(**kw) == -2, kw
        assert b"do not fit" in lib.hqq_hip_last_error(), kw
    for kw in (dict(qrs=260), dict(qhs=68), dict(qrs=-256)):
        assert dense(**kw) == -6, kw
    assert dense(hd=96, qhs=96, qrs=384) == -4 and dense(dtype=0) == -4
    assert dense(heads=(4, 3)) == -2 and dense(L=30001) == -2

    def packed(nbits=8, gs=32, pos0=0, T=16, L=64, hd=64):
        return lib.hqq_hip_attn_prefill_kvq(nbits, p, 256, 64, p, p, p, p, p, p, pos0, T, p, 4, 4, hd, gs, L, 0.125, 1, None)

    assert packed(T=0) == -2 and packed(pos0=60, T=5) == -2
    assert packed(nbits=3) == -4 and packed(nbits=4, gs=64) == -4 and packed(gs=48) == -4   # the cache's coverage rule, with its own code


# ---- the case bed ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_covers_what_it_claims():
    for dt in pc.DTS:
        for hd in pc.HDS:
            cases = pc.cases(dt, hd)
            for heads in pc.HEADS:
                mine = {(c.T, c.pos0) for c in cases if c.heads == heads}
                assert {(T, p0) for T in (1, 15, 16, 17, 31, 32, 33, 49) for p0 in (0, 5, 16, 37)} <= mine, (dt, hd, heads)
                assert (273, 0) in mine and any(c.n == c.L for c in cases if c.heads == heads)
            assert all(c.L <= 512 and c.n <= c.L for c in cases)
            assert any(-(-c.n // 32) >= 16 for c in cases)                     # 16 blocks: two per wave
            assert any(c.T % 16 and c.T > 16 for c in cases)                    # a padded last tile behind a full one
    c = pc.Case("f16", 64, 128, (4, 4), 5, 33)
    assert pc.tiles(c) == [(0, tuple(range(5, 21))), (1, tuple(range(21, 37))), (2, (37,))]


def test_every_tile_keeps_the_band_condition():
    """_tile_cases' condition, unchanged, on every tile of a slice of the bed: the terms other than the rounding of P and of the output sum to less than
    u_T vmax — the band cannot hide a failure —, and the fp64 reference rounded to T lies inside its own band"""
    worst, ran = 0.0, 0
    for dt, hd in (("f16", 256), ("bf16", 64), ("f16", 128)):
        for case in pc.cases(dt, hd):
            if case.pos0 not in (0, 37) or case.T not in (17, 49, 273):
                continue
            t = pc.build(case, "cpu")
            ref = pc.reference(t)
            assert bool(torch.isfinite(ref).all()), case.id
            for j, pos in pc.tiles(case):
                rows = slice(16 * j, 16 * j + len(pos))
                tol, rest, lead = tc.band(pc.tile_view(t, j, pos), ref[rows], hd ** -0.5)
                assert bool((lead > 0).all()) and bool((rest < lead).all()), (case.id, j, float((rest / lead).max()))
                worst = max(worst, float((rest / lead).max()))
            assert not bool(pc.outside_band(t, ref.to(pc.DT[dt]), ref).any()), case.id
            ran += 1
    assert ran >= 12 and 0.0 < worst < 1.0


def test_the_reference_of_all_rows_is_the_tiles_reference():
    """slicing one fp64 pass over all T rows gives what _tile_cases.reference_rows gives tile by tile (each row's softmax is its own)"""
    case = pc.Case("f16", 64, 128, (8, 2), 5, 33, seed=4)
    t = pc.build(case, "cpu")
    ref = pc.reference(t)
    for j, pos in pc.tiles(case):
        v = pc.tile_view(t, j, pos)
        want, _ = tc.reference_rows(v["q"], v["K"], v["V"], v["pos"], 0.125)
        assert torch.allclose(ref[16 * j:16 * j + len(pos)], want, rtol=1e-13, atol=1e-15), j


# ---- the keyword and the coverage rule ---------------------------------------------------------------------------------------------------------------------
def test_the_decoders_validate_the_keyword_before_anything_is_built():
    from hqq_amd.utils import generation as gen
    for bad in ("x", "sdpa", "Hip", "", None, True, 1):
        with pytest.raises(ValueError, match="prefill_attention"):
            gen.check_prefill_attention(bad)
        with pytest.raises(ValueError, match="prefill_attention"):
            gen.GraphedGreedyDecoder(None, prefill_attention=bad)
        with pytest.raises(ValueError, match="prefill_attention"):
            gen.HFGenerator(None, None, prefill_attention=bad)
    gen.check_prefill_attention("model")
    gen.check_prefill_attention("hip")


def _toy(dt=torch.float16, **kw):
    """the tiny Llama of tests/test_spec_cpu.py at a head size the kernels cover (that one has heads of 32 values in fp32, which the rule refuses: checked below)"""
    transformers = pytest.importorskip("transformers")
    args = dict(hidden_size=128, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64, max_position_embeddings=64)
    args.update(kw)
    return transformers.LlamaForCausalLM(transformers.LlamaConfig(**args)).to(dt).eval()


def test_supports_prefill_attention():
    transformers = pytest.importorskip("transformers")
    from hqq_amd.utils import llama_fused as lf
    from test_spec_cpu import _tiny_llama
    assert lf.supports_prefill_attention(_toy()) and lf.supports_prefill_attention(_toy(torch.bfloat16, num_key_value_heads=1))
    spec = _tiny_llama()                                                        # heads of 32 values, fp32: both refuse
    assert lf.head_dim(spec.config) == 32 and not lf.supports_prefill_attention(spec) and not lf.supports_prefill_attention(spec.half())
    assert not lf.supports_prefill_attention(_toy(torch.float32))
    assert not lf.supports_prefill_attention(_toy(hidden_size=192))             # head_dim 96
    assert not lf.supports_prefill_attention(_toy(head_dim=96))
    soft = _toy()
    soft.config.attn_logit_softcapping = 30.0
    assert not lf.supports_prefill_attention(soft)
    mistral = transformers.MistralForCausalLM(transformers.MistralConfig(hidden_size=128, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2,
                                                                         num_key_value_heads=2, vocab_size=64, sliding_window=16)).half().eval()
    assert mistral.config.sliding_window == 16 and not lf.supports_prefill_attention(mistral)
    mistral.config.sliding_window = None
    for blk in mistral.model.layers:
        if hasattr(blk.self_attn, "sliding_window"):
            blk.self_attn.sliding_window = None
    assert lf.supports_prefill_attention(mistral)
    sinks = _toy()
    sinks.model.layers[0].self_attn.sinks = torch.zeros(2)
    assert not lf.supports_prefill_attention(sinks)
    # with the cache the decoder would build: the dense cache up to the kernels' limit, the quantised one where ops.kv_covers holds
    ok = _toy()
    assert lf.supports_prefill_attention(ok, 512) and lf.supports_prefill_attention(ok, 30000) and not lf.supports_prefill_attention(ok, 30001)
    assert lf.supports_prefill_attention(ok, 512, 8) and lf.supports_prefill_attention(ok, 512, 4, 32) and not lf.supports_prefill_attention(ok, 512, 4, 64)
    assert not lf.supports_prefill_attention(object())


# ---- the wrappers -----------------------------------------------------------------------------------------------------------------------------------------
def test_wrapper_shape_errors(monkeypatch):
    """the wrappers refuse mis-shaped arguments before the library is asked (the device check is stepped over: the tensors are the CPU's)"""
    from hqq_amd import ops
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    q = torch.zeros(16, 4, 64, dtype=torch.float16)
    K, V = torch.zeros(2, 32, 64, dtype=torch.float16), torch.zeros(2, 32, 64, dtype=torch.float16)
    bad = [
        dict(q=q[:0]),                                                          # T = 0
        dict(pos0=17), dict(pos0=-1), dict(q=torch.zeros(33, 4, 64, dtype=torch.float16)),   # pos0 + T > L
        dict(pos0=torch.zeros(1, dtype=torch.int64)), dict(pos0=True),          # a host integer
        dict(q=q.float()), dict(q=q.bfloat16()), dict(k_cache=K.bfloat16()), dict(q=q.double(), k_cache=K.double(), v_cache=V.double()),   # dtypes
        dict(q=torch.zeros(16, 4, 128, dtype=torch.float16)[:, :, ::2]),        # the last dimension is not dense
        dict(q=torch.zeros(16, 4, 68, dtype=torch.float16)[:, :, :64]),         # a head stride of 68 elements
        dict(q=q.view(16, 256)), dict(q=torch.zeros(16, 4, 128, dtype=torch.float16)),       # not [T, n_heads, the caches' head_dim]
        dict(v_cache=V[:1]), dict(k_cache=K.view(2, 1, 32, 64), v_cache=V.view(2, 1, 32, 64)), dict(k_cache=K.transpose(0, 1)),
        dict(out=torch.zeros(16, 4, 64)), dict(out=torch.zeros(15, 4, 64, dtype=torch.float16)), dict(out=torch.zeros(16, 4, 128, dtype=torch.float16)[:, :, :64]),
    ]
    for kw in bad:
        args = dict(q=q, k_cache=K, v_cache=V, pos0=0)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.attn_prefill(**args)
    lv, mt = torch.zeros(2, 32, 64, dtype=torch.uint8), torch.zeros(2, 32, 2, dtype=torch.float16)
    with pytest.raises(ValueError):
        ops.attn_prefill_kvq(q, (lv, mt, mt, lv, mt), 0, 64)                    # six buffers
    with pytest.raises(ValueError):
        ops.attn_prefill_kvq(q, (mt, mt, mt, mt, mt, mt), 0, 64)                # level buffers are uint8
    with pytest.raises(ValueError):
        ops.attn_prefill_kvq(q, tuple(t.view(2, 1, *t.shape[1:]).expand(2, 2, *t.shape[1:]) for t in (lv, mt, mt, lv, mt, mt)), 0, 64)   # one sequence
    monkeypatch.setattr(ops, "kv_covers", lambda *a: True)
    for kw in (dict(q=q[:0]), dict(pos0=17), dict(q=q.bfloat16()), dict(q=torch.zeros(16, 4, 128, dtype=torch.float16)[:, :, ::2])):
        args = dict(q=q, bufs=(lv, mt, mt, lv, mt, mt), pos0=0, head_dim=64)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.attn_prefill_kvq(**args)
