"""Host-side checks of the grouped-query decode attention (tests/_gqa_cases.py; csrc/attn_gqa.hip): on the CPU the fp64 reference alone must pass every closed
form and every band condition; the split rule, the coverage rule, the wrappers' shape errors and the keyword validation of the step and the decoders."""
import pytest

torch = pytest.importorskip("torch")

import _attn_cases as ac  # noqa: E402
import _gqa_cases as gc  # noqa: E402
import _tile_cases as tc  # noqa: E402


# ---- the case bed ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_grid_covers_what_it_claims():
    cases = [c for dt in gc.DTS for hd in gc.HDS for c in gc.closed_cases(dt, hd)] + gc.random_cases()
    for kind in ("needle", "twin", "flat", "ident", "random"):
        mine = [c for c in cases if c.kind == kind]
        assert {c.heads for c in mine} == set(gc.HEADS) and {c.hd for c in mine} == set(gc.HDS) and {c.dt for c in mine} == set(gc.DTS), kind
        assert {c.S for c in mine} == set(gc.SPLITS) and {len(c.pos) for c in mine} == {1, 3}, kind
    assert {c.G for c in cases} == {1, 2, 4, 7, 16}
    seen = {p for c in cases for p in c.pos}
    assert {0, 31, 32, 255, 256, 257, 1023, gc.L_BIG - 1} <= seen
    assert all(c.L <= 2048 for c in cases)
    assert any(c.pos[b] + 1 < c.S for c in cases for b in range(len(c.pos)))            # n < S
    assert any(list(c.pos) != sorted(c.pos) for c in cases)                              # unsorted


@pytest.mark.parametrize("dt", gc.DTS)
@pytest.mark.parametrize("hd", gc.HDS)
def test_the_reference_passes_every_closed_form(dt, hd):
    cases = gc.closed_cases(dt, hd)
    bad = gc.run(cases, "cpu")
    assert not bad, gc.summary(bad, f"{dt} hd {hd}, {len(cases)} cases")


def test_ident_tells_the_heads_of_a_group_apart():
    """in every ident case the closed form differs between any two heads of a group, in every sequence and group (so a swapped or repeated head-to-row mapping
    cannot pass); in the other closed forms the heads of a group share it"""
    ran = 0
    for dt, hd in (("bf16", 64), ("f16", 256)):
        for case in gc.closed_cases(dt, hd):
            if case.kind == "random" or case.G == 1:
                continue
            B, n_kv, G = len(case.pos), case.heads[1], case.G
            cf = gc.expected(gc.build(case, "cpu")).view(B, n_kv, G, hd)
            if case.kind != "ident":
                assert bool((cf == cf[:, :, :1]).all()), case.id
                continue
            for u in range(G):
                for w in range(u + 1, G):
                    assert bool((cf[:, :, u] != cf[:, :, w]).any(-1).all()), (case.id, u, w)
            ran += 1
    assert ran >= 20


def test_every_random_case_keeps_the_band_condition():
    """_tile_cases' condition, unchanged: the terms other than the rounding of P and of the output sum to less than u_T vmax — the band cannot hide a failure.  And
    the reference itself lies inside its own band after rounding to T (it would not if the tensors held NaN in a visible row)"""
    worst = 0.0
    for case in gc.random_cases():
        t = gc.build(case, "cpu")
        ref = gc.reference(t)
        tol, rest, lead = gc.band(t, ref)
        assert bool(torch.isfinite(ref).all()) and bool((lead > 0).all()), case.id
        assert bool((rest < lead).all()), (case.id, float((rest / lead).max()))
        worst = max(worst, float((rest / lead).max()))
        assert not bool(gc.kernel_bad(t, ref.to(gc.DT[case.dt]).reshape(len(case.pos), -1), ref).any()), case.id
    assert 0.0 < worst < 1.0


def test_a_sequence_seen_as_tile_rows_is_the_one_row_reference():
    """tile_view transposes faithfully: _tile_cases.reference_rows through it equals _attn_cases.reference (the one-row fp64 attention) on the sequence"""
    case = gc.Case("random", "f16", 64, 320, (8, 2), (319, 0, 31), 3, seed=5)
    t = gc.build(case, "cpu")
    ref = gc.reference(t)
    for b, p in enumerate(case.pos):
        want, _ = ac.reference(t["q"][b].view(8, 64), t["K"][b], t["V"][b], p + 1, 64 ** -0.5)
        assert torch.allclose(ref[b], want, rtol=1e-13, atol=1e-15), b


# ---- the host rules ---------------------------------------------------------------------------------------------------------------------------------------
def test_attn_gqa_covers():
    from hqq_amd import ops
    assert all(ops.attn_gqa_covers(h, k) for h, k in ((4, 2), (8, 2), (7, 1), (16, 1), (32, 8), (28, 4), (64, 8)))
    assert not any(ops.attn_gqa_covers(h, k) for h, k in ((8, 8), (1, 1), (32, 1), (34, 2), (7, 2), (0, 1), (4, 0)))


def test_attn_gqa_splits_stays_inside_its_limits():
    from hqq_amd import ops
    assert ops.ATTN_MAX_SPLITS == 64
    for kv_len in (1, 64, 255, 256, 257, 511, 512, 1024, 1536, 4096, 16384, 30000):
        for batch in (1, 2, 3, 8, 16, 64):
            for n_kv in (1, 2, 4, 8):
                s = ops.attn_gqa_splits(kv_len, batch, n_kv)
                assert isinstance(s, int) and 1 <= s <= ops.ATTN_MAX_SPLITS, (kv_len, batch, n_kv, s)
                if kv_len // 256 >= 1:
                    assert s <= kv_len // 256, (kv_len, batch, n_kv, s)
                assert s == ops.attn_gqa_splits(kv_len, batch, n_kv)                     # a function of its arguments alone
    assert ops.attn_gqa_splits(16384, 1, 8) == 32 and ops.attn_gqa_splits(16384, 16, 8) == 2 and ops.attn_gqa_splits(16384, 64, 8) == 1
    assert ops.attn_gqa_splits(1024, 1, 8) == 4 and ops.attn_gqa_splits(30000, 1, 1) == 32 and ops.attn_gqa_splits(16384, 1, 4) == 32


def test_wrapper_shape_errors(monkeypatch):
    """the wrappers refuse mis-shaped arguments before the library is asked (the device check is stepped over: the tensors are the CPU's)"""
    from hqq_amd import ops
    monkeypatch.setattr(ops, "_dev", lambda *ts: None)
    q, out = torch.zeros(2, 8 * 64, dtype=torch.float16), torch.zeros(2, 8 * 64, dtype=torch.float16)
    K, V = torch.zeros(2, 2, 32, 64, dtype=torch.float16), torch.zeros(2, 2, 32, 64, dtype=torch.float16)
    pos = torch.zeros(2, dtype=torch.int64)
    bad = [
        dict(pos=pos.int()), dict(pos=torch.zeros(3, dtype=torch.int64)), dict(k_cache=K[0]), dict(v_cache=V[:, :1]), dict(k_cache=K.transpose(1, 2)),
        dict(q=q[:, :100]), dict(out=out[:1]), dict(q=q.t()),
    ]
    for kw in bad:
        args = dict(q=q, k_cache=K, v_cache=V, pos=pos, out=out, scaling=0.125)
        args.update(kw)
        with pytest.raises(ValueError):
            ops.attn_decode_gqa_batched(**args)
    with pytest.raises(ValueError):
        ops.attn_decode_gqa(q[0], K[0], V[0, :1], pos[:1], out[0], 0.125)                # one sequence: caches of different shapes
    with pytest.raises(ValueError):
        ops.attn_decode_gqa_kvq_batched(q, (K,) * 5, pos, out, 0.125, 64)                # six buffers
    with pytest.raises(ValueError):
        ops.attn_decode_gqa_kvq_batched(q, (K,) * 6, pos, out, 0.125, 64)                # level buffers are uint8


# ---- keyword validation -------------------------------------------------------------------------------------------------------------------------------------
def test_the_decoders_validate_the_keyword_before_anything_is_built():
    from hqq_amd.utils import generation as gen
    for bad in ("rows", "tile", "Group", "", None, True, 1):
        with pytest.raises(ValueError, match="gqa_attention"):
            gen.check_gqa_attention(bad)
        with pytest.raises(ValueError, match="gqa_attention"):
            gen.GraphedGreedyDecoder(None, gqa_attention=bad)
        with pytest.raises(ValueError, match="gqa_attention"):
            gen.HFGenerator(None, None, gqa_attention=bad)
    gen.check_gqa_attention("heads")
    gen.check_gqa_attention("group")


def _toy(n_heads, n_kv):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=64, hidden_size=256, intermediate_size=128, num_hidden_layers=1, num_attention_heads=n_heads, num_key_value_heads=n_kv,
                                   max_position_embeddings=128)
    return transformers.LlamaForCausalLM(cfg).half().eval()


def test_the_step_refuses_what_the_issue_lists():
    """the constructor's refusals need no GPU: they come before a layer or the cache is looked at"""
    from hqq_amd.utils import llama_fused as lf
    gqa, mha = _toy(4, 2), _toy(4, 4)
    assert lf.supports_gqa_attention(gqa) and not lf.supports_gqa_attention(mha)
    with pytest.raises(ValueError, match="gqa_attention: 'heads' or 'group'"):
        lf.FusedLlamaStep(gqa, None, 64, attention="hip", gqa_attention="tile")
    with pytest.raises(ValueError, match="needs attention='hip'"):
        lf.FusedLlamaStep(gqa, None, 64, attention="sdpa", gqa_attention="group")
    with pytest.raises(ValueError, match="verify step keeps verify_attention"):
        lf.FusedLlamaStep(gqa, None, 64, attention="hip", batch=4, verify=True, gqa_attention="group")
    with pytest.raises(ValueError, match="attn_gqa_covers"):
        lf.FusedLlamaStep(mha, None, 64, attention="hip", gqa_attention="group")
    with pytest.raises(ValueError, match="gqa_attention"):
        lf.FusedLlamaBatchStep(gqa, None, 64, 2, attention="hip", gqa_attention="bogus")
