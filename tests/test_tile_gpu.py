"""The verify step's tiled decode attention on a GPU (csrc/attn_tile.hip; ops.attn_decode_tiled; FusedLlamaStep(verify=True, verify_attention="tile");
GraphedGreedyDecoder(speculate="ngram", verify_attention="tile")): the closed-form and random cases of tests/_tile_cases.py against fp64 attention, the
kernel's own contract (determinism, row independence, nothing read past n_max, nothing written outside `rows` rows, argument errors before any launch), the
step against the model's forward, and the decoder against the plain route and against a host-driven loop over the same step."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

import _spec_cases as sc  # noqa: E402
import _tile_cases as tc  # noqa: E402
from test_batch_decode_gpu import _quantised, _tiny_llama  # noqa: E402
from test_spec_gpu import _dev, _plain_route, _prefilled  # noqa: E402


def _kernel(t):
    from hqq_amd import ops
    case = t["case"]
    out = torch.full((len(case.pos), case.heads[0] * case.hd), float("nan"), dtype=tc.DT[case.dt], device="cuda")
    return ops.attn_decode_tiled(t["q"], t["K"], t["V"], t["pos"], out, case.hd ** -0.5, splits=case.S)


# ---- against fp64 -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", tc.DTS)
@pytest.mark.parametrize("hd", tc.HDS)
def test_closed_forms(dt, hd):
    """tier (the per-row causal edge), twin, flat (the per-row denominator) and the split cases"""
    cases = tc.closed_cases(dt, hd)
    bad = tc.run(cases, "cuda", _kernel)
    assert not bad, tc.summary(bad, f"{dt} hd {hd}, {len(cases)} launches")


@pytest.mark.parametrize("dt", tc.DTS)
@pytest.mark.parametrize("hd", tc.HDS)
def test_needle_sweep(dt, hd):
    """every n_max from 1 to 2 KB + 33"""
    cases = tc.sweep_cases(dt, hd)
    bad = tc.run(cases, "cuda", _kernel)
    assert not bad, tc.summary(bad, f"{dt} hd {hd}, {len(cases)} launches")


def test_random_cases_stay_inside_the_band():
    cases = tc.random_cases()
    bad = tc.run(cases, "cuda", _kernel)
    assert not bad, tc.summary(bad, f"{len(cases)} launches")


# ---- the kernel's own contract -------------------------------------------------------------------------------------------------------------------------
CONTRACT = [c for c in tc.random_cases() if len(c.pos) >= 8 and (c.pos[0] in (31, 1023) or c.pos[-1] == tc.RANDOM_L - 1 or c.seed > 900)]


def test_two_calls_give_the_same_bits():
    assert len(CONTRACT) >= 6 and any(c.S > 1 for c in CONTRACT)
    for case in CONTRACT:
        t = tc.build(case, "cuda")
        assert torch.equal(tc.bits(_kernel(t)), tc.bits(_kernel(t))), case.id


def test_a_row_depends_on_no_other_rows_query():
    """the same pos, rows and splits; the queries of the rows > i replaced: no bit of the rows <= i changes (and the replaced rows do change)"""
    ran = 0
    for case in CONTRACT:
        t = tc.build(case, "cuda")
        R = len(case.pos)
        base = _kernel(t).clone()
        for i in (0, R // 2, R - 2):
            u = dict(t)
            u["q"] = t["q"].clone()
            u["q"][i + 1:] = torch.randn_like(u["q"][i + 1:])
            got = _kernel(u)
            assert torch.equal(tc.bits(got[:i + 1]), tc.bits(base[:i + 1])), (case.id, i)
            assert not torch.equal(tc.bits(got[i + 1:]), tc.bits(base[i + 1:])), (case.id, i)
            ran += 1
    assert ran >= 18


def test_garbage_past_n_max_changes_no_bit():
    """the cache from n_max on filled with NaN, with +inf, with zeros: the same bits (0 * NaN inside an MFMA would be NaN)"""
    ran = 0
    for case in tc.random_cases():
        if case.n_max == case.L:
            continue
        outs = [_kernel(tc.build(case, "cuda", fill=f)) for f in (float("nan"), float("inf"), 0.0)]
        assert bool(torch.isfinite(outs[2]).all()), case.id
        assert torch.equal(tc.bits(outs[0]), tc.bits(outs[2])) and torch.equal(tc.bits(outs[1]), tc.bits(outs[2])), case.id
        ran += 1
    assert ran >= 40


@pytest.mark.parametrize("S", [1, 3])
def test_padding_rows_read_and_write_nothing(S):
    """out: `rows` rows inside a larger allocation pre-filled with a sentinel — nothing outside them is written; q: the last `rows` rows of its allocation"""
    from hqq_amd import ops
    for R in (1, 3, 15):
        case = tc.Case("random", "f16", 128, 2048, tuple(range(1200, 1200 + R)), S, heads=(8, 2), seed=50 + R)
        t = tc.build(case, "cuda")
        n = 8 * 128
        qbig = torch.randn(R + 3, n, device="cuda").half()
        q = qbig[3:]
        q.copy_(t["q"])
        assert q.data_ptr() + q.numel() * 2 == qbig.data_ptr() + qbig.numel() * 2
        big = torch.full((R + 4, n), 12345.0, dtype=torch.float16, device="cuda")
        out = big[2:2 + R]
        ops.attn_decode_tiled(q, t["K"], t["V"], t["pos"], out, 128 ** -0.5, splits=S)
        assert bool((big[:2] == 12345.0).all()) and bool((big[2 + R:] == 12345.0).all()), R
        assert torch.equal(tc.bits(out), tc.bits(_kernel(t))), R


def test_argument_errors_come_before_any_launch():
    from hqq_amd import _C
    from hqq_amd import ops
    lib = _C.lib()
    case = tc.Case("random", "f16", 64, 256, tuple(range(100, 108)), 2, heads=(4, 4), seed=3)
    t = tc.build(case, "cuda")
    out = torch.full((16, 4 * 64), 777.0, dtype=torch.float16, device="cuda")
    need = int(lib.hqq_hip_attn_decode_workspace_bytes(8 * 4, 64, 2))
    assert need == 8 * 4 * 2 * 66 * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert tc.call(lib, t, out, ws_ptr=ws.data_ptr(), ws_bytes=need - 1) == -2          # too small
    assert tc.call(lib, t, out, ws_ptr=0, ws_bytes=need) == -2                          # missing
    assert tc.call(lib, t, out, S=1, rows=0) == -2 and tc.call(lib, t, out, S=1, rows=17) == -2
    assert tc.call(lib, t, out, S=65, ws_ptr=ws.data_ptr(), ws_bytes=need) == -2
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())                                                   # nothing was launched
    assert tc.call(lib, t, out, ws_ptr=ws.data_ptr(), ws_bytes=need) == 0
    assert torch.equal(tc.bits(out[:8]), tc.bits(_kernel(t))) and bool((out[8:] == 777.0).all())
    with pytest.raises(ValueError):
        ops.attn_decode_tiled(t["q"], t["K"].view(2, 2, 256, 64), t["V"].view(2, 2, 256, 64), t["pos"], out[:8], 0.125)
    got = ops.attn_decode_tiled(t["q"], t["K"].view(1, 4, 256, 64), t["V"].view(1, 4, 256, 64), t["pos"], torch.empty_like(out[:8]), 0.125, splits=2)
    assert torch.equal(tc.bits(got), tc.bits(out[:8]))                                  # [1, n_kv, L, hd] is accepted


def test_positions_outside_the_cache_attend_at_the_last_slot():
    """the one-row kernels' rule: a position outside [0, L) attends as if at L - 1"""
    from hqq_amd import ops
    case = tc.Case("random", "bf16", 64, 96, (40, 95, 3), 1, heads=(4, 4), seed=77)
    t = tc.build(case, "cuda")
    want = _kernel(t)
    for wild in (96, -1, 1 << 40):
        pos = torch.tensor([40, wild, 3], dtype=torch.int64, device="cuda")
        got = ops.attn_decode_tiled(t["q"], t["K"], t["V"], pos, torch.empty_like(want), 0.125)
        assert torch.equal(tc.bits(got), tc.bits(want)), wild


# ---- the verify step ------------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    return _quantised(_tiny_llama())


def test_tile_step_is_causal_and_follows_the_models_forward(tiny):
    """test_spec_gpu's check of the "rows" step, held by the "tile" step: every row's logits are the model's own forward at that position within the same band,
    and replacing the rows behind row i changes no bit of the logits of rows <= i"""
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model, L, T, R = tiny, 64, 7, 8
    seq = torch.randint(0, 512, (1, T + R), generator=torch.Generator().manual_seed(3)).cuda()
    cache, _ = _prefilled(model, seq[:, :T], L)
    step = FusedLlamaStep(model, cache, L, attention="hip", batch=R, verify=True, verify_attention="tile")
    assert step.verify_attention == "tile"
    pos = torch.arange(T, T + R, device="cuda")
    true = step(seq[0, T:].view(R, 1).contiguous(), pos, L).clone()
    with torch.no_grad():
        want = model(seq).logits[0, T:T + R]
    torch.testing.assert_close(true.float(), want.float(), rtol=5e-3, atol=5e-3)
    for i in (0, 3, 6):
        tok = seq[0, T:].clone()
        tok[i + 1:] = (tok[i + 1:] + 1 + torch.arange(R - i - 1, device="cuda")) % 512
        other = step(tok.view(R, 1), pos, L)
        assert torch.equal(other[:i + 1], true[:i + 1]), i
        assert not torch.equal(other[i + 1:], true[i + 1:]), i


def test_tile_step_refusals(tiny):
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model, L = tiny, 64
    cache, _ = _prefilled(model, torch.randint(0, 512, (1, 5)).cuda(), L)
    assert FusedLlamaStep(model, cache, L, attention="hip", batch=2, verify=True).verify_attention == "rows"
    with pytest.raises(ValueError, match="verify=True"):
        FusedLlamaStep(model, cache, L, attention="hip", verify_attention="tile")
    for other in ("Tile", "tiled", None, ""):
        with pytest.raises(ValueError, match="verify_attention"):
            FusedLlamaStep(model, cache, L, attention="hip", batch=2, verify=True, verify_attention=other)


# ---- the decoder ----------------------------------------------------------------------------------------------------------------------------------------
def _tile_decoder(model, L, R=8, N=3, **kw):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    return GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", speculate="ngram", draft_rows=R, ngram_max=N, verify_attention="tile", **kw)


def test_tile_decoder_emits_the_plain_tokens(tiny):
    """on every prompt of _spec_cases.E2E_PROMPTS — the prompts that keep the 0.05 guard band; LOOSE_PROMPTS, which no guard selects, break it on the plain route
    alone (seed 0: a step with its two best logits 0.0015 apart) and are the next test's, where no tolerance applies —: the guard band is re-checked on the plain
    route here, then the speculative decoder with the tiled attention emits the plain route's tokens.  No prompt is skipped"""
    dec = _tile_decoder(tiny, sc.CACHE_LEN)
    assert dec.speculating and dec.verify_attention == "tile"
    assert len(sc.E2E_PROMPTS) == 4 and sum(r for _, r in sc.E2E_PROMPTS) == 2
    for seed, repeated in sc.E2E_PROMPTS:
        ids = torch.tensor([sc.e2e_prompt(seed, repeated)], device="cuda")
        toks, gaps = _plain_route(tiny, ids, sc.NEW_TOKENS, sc.CACHE_LEN)
        print(f"seed {seed}: smallest top-1 / top-2 gap over {len(gaps)} steps {min(gaps):.4f}")
        assert len(gaps) == sc.NEW_TOKENS - 1 and min(gaps) > sc.GAP, (seed, min(gaps))
        got = dec.generate(ids, sc.NEW_TOKENS)
        assert dec._spec["step"].verify_attention == "tile"
        assert torch.equal(got, toks), seed
        assert dec.spec_stats["tokens"] == sc.NEW_TOKENS - 1
        if repeated:
            assert dec.spec_stats["tokens"] > dec.spec_stats["steps"]


def _host_loop(model, ids, n, L, R, N):
    """test_spec_gpu._host_loop over the "tile" step: propose_ref, the verify step run eagerly on those rows, torch's argmax, accept_ref"""
    from hqq_amd.utils.generation import kv_bucket
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    T = ids.shape[1]
    cache, logits = _prefilled(model, ids, L)
    step = FusedLlamaStep(model, cache, L, attention="hip", batch=R, verify=True, verify_attention="tile")
    hist = np.zeros(L, dtype=np.int64)
    hist[:T] = ids[0].cpu().numpy()
    hist[T] = int(logits.argmax(-1))
    p, last, done, steps, tokens, accepted = T, T + n - 1, 0, 0, 0, []
    while p < last:
        tok, pos = sc.propose_ref(hist, p, R, N)
        g = step(_dev(tok).view(R, 1), _dev(pos), kv_bucket(p + R - 1, "hip", L)).argmax(-1).tolist()
        hist, p2, done, steps, tokens = sc.accept_ref(g, tok, hist, p, last, -1, done, steps, tokens)
        accepted.append(p2 - p)
        p = p2
    return torch.as_tensor(hist[:p + 1]).view(1, -1).cuda(), steps, tokens, accepted


def test_the_captured_tile_loop_equals_a_host_driven_loop(tiny):
    """the same rows through the same launches, so no tolerance applies; assigning verify_attention rebuilds the kept state"""
    R, N, L = 8, 3, sc.CACHE_LEN
    dec = _tile_decoder(tiny, L, R, N)
    for seed, repeated in sc.LOOSE_PROMPTS:
        ids = torch.tensor([sc.e2e_prompt(seed, repeated)], device="cuda")
        want, steps, tokens, accepted = _host_loop(tiny, ids, sc.NEW_TOKENS, L, R, N)
        print(f"seed {seed}: tokens per step {accepted}")
        for every in (16, 3):
            assert torch.equal(dec.generate(ids, sc.NEW_TOKENS, check_every=every), want), (seed, every)
            assert dec.spec_stats == {"steps": steps, "tokens": tokens} and tokens == sc.NEW_TOKENS - 1
    assert dec._spec["graphs"] and dec._spec["step"].verify_attention == "tile"
    dec.verify_attention = "rows"
    dec.generate(ids, 8)
    assert dec.verify_attention == "rows" and dec._spec["step"].verify_attention == "rows"
    with pytest.raises(ValueError, match="verify_attention"):
        dec.verify_attention = "both"


def test_the_tile_loop_at_a_context_that_splits_the_attention():
    """1100 prompt tokens on a cache of 2048: the tiled attention runs with 4 splits, its workspace and the merging launch inside the captured step"""
    from hqq_amd import ops
    from hqq_amd.utils.generation import kv_bucket
    model = _quantised(_tiny_llama(max_position_embeddings=2048))
    R, N, L, T = 8, 3, 2048, 1100
    assert ops.attn_splits(kv_bucket(T + R - 1, "hip", L)) == 4
    ids = torch.randint(0, 512, (1, T), generator=torch.Generator().manual_seed(11)).cuda()
    want, steps, tokens, accepted = _host_loop(model, ids, 40, L, R, N)
    print(f"tokens per step {accepted}")
    dec = _tile_decoder(model, L, R, N)
    for _ in range(2):
        assert torch.equal(dec.generate(ids, 40, check_every=5), want)
        assert dec.speculating and dec.spec_stats == {"steps": steps, "tokens": tokens} and list(dec._spec["graphs"]) == [2048]


def test_hfgenerator_passes_the_keyword_on(tiny):
    from hqq_amd.utils.generation import HFGenerator
    from test_model_gpu import _ToyTokenizer
    gen = HFGenerator(tiny, _ToyTokenizer(), max_new_tokens=16, compile="partial", speculate="ngram", draft_rows=4, ngram_max=2, attention="hip", verify_attention="tile")
    assert gen.decoder.speculating and gen.decoder.verify_attention == "tile"
    r = gen.generate("7 8 9 10 11 7 8 9", use_chat_template=False, verbose=False)
    assert gen.decoder._spec["step"].verify_attention == "tile" and gen.decoder.spec_stats["tokens"] >= 1 and r["output_tokens"].numel() == 16
    with pytest.raises(ValueError, match="verify_attention"):
        HFGenerator(tiny, _ToyTokenizer(), max_new_tokens=16, verify_attention="tile")          # no speculation asked for
    with pytest.raises(ValueError, match="verify_attention"):
        HFGenerator(tiny, _ToyTokenizer(), max_new_tokens=16, speculate="ngram", attention="hip", verify_attention="columns")


def test_with_sdpa_the_decoder_decodes_as_before(tiny):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    ids = torch.tensor([sc.e2e_prompt(1, True)], device="cuda")
    want = GraphedGreedyDecoder(tiny, max_cache_len=64, attention="sdpa").generate(ids, 12)
    for va in ("rows", "tile"):
        dec = GraphedGreedyDecoder(tiny, max_cache_len=64, attention="sdpa", speculate="ngram", verify_attention=va)
        got = dec.generate(ids, 12)
        assert not dec.speculating and dec._spec is None and dec.spec_stats == {"steps": 0, "tokens": 0}
        assert torch.equal(got, want), va
    with pytest.raises(ValueError, match="verify_attention"):
        GraphedGreedyDecoder(tiny, max_cache_len=64, attention="hip", verify_attention="tile")  # "tile" without speculate
