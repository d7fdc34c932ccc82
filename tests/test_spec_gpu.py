"""Speculative greedy decoding by prompt lookup on a GPU: the proposer and the accept step against their host restatements (bit for bit), the two
shared-cache glue kernels against R calls of their batch-1 siblings (bit for bit), the verify step's causality (exact) and its logits against the model's
own forward, and GraphedGreedyDecoder(speculate="ngram") against the same decoder without speculation (tokens)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
transformers = pytest.importorskip("transformers")
pytestmark = pytest.mark.gpu

import _attn_cases as ac  # noqa: E402
import _spec_cases as sc  # noqa: E402
from test_batch_decode_gpu import _quantised, _tiny_llama  # noqa: E402

DTS = [torch.float16, torch.bfloat16]
CAP = 30000


def _dev(x):
    return torch.as_tensor(np.asarray(x, dtype=np.int64)).cuda()


# ---- the proposer ---------------------------------------------------------------------------------------------------------------------------------
def _propose_grid():
    return [(p, R, N) for N in (0, 1, 3, 4) for p in sorted({0, 1, 2, N, 1023, 1024, 1025, 29999}) for R in (2, 8, 16)]


def _check_propose(hist_np, hist, grid, what):
    from hqq_amd import ops
    p_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    bad = []
    for p, R, N in grid:
        p_dev.fill_(p)
        tok = torch.full((R,), -7, dtype=torch.int64, device="cuda")
        pos = torch.full((R,), -7, dtype=torch.int64, device="cuda")
        ops.spec_propose(hist, p_dev, tok, pos, N)
        want_tok, want_pos = sc.propose_ref(hist_np, p, R, N)
        if tok.tolist() != want_tok.tolist() or pos.tolist() != want_pos.tolist():
            bad.append((what, p, R, N, tok.tolist(), want_tok.tolist()))
    assert not bad, f"{len(bad)} of {len(grid)} differ, first: {bad[:3]}"


@pytest.mark.parametrize("alphabet", [2, 1 << 40])
def test_propose_equals_the_host_rule(alphabet):
    """2 symbols: matches of every length everywhere (the largest n and the latest e decide); 2^40 symbols: no match at all"""
    hist_np = np.random.RandomState(alphabet % 1000).randint(0, alphabet, CAP, dtype=np.int64)
    if alphabet > 2:
        assert len(np.unique(hist_np)) == CAP
    _check_propose(hist_np, _dev(hist_np), _propose_grid(), f"alphabet {alphabet}")


@pytest.mark.parametrize("where", ["start", "end"])
def test_propose_finds_the_only_match(where):
    """a history without repeats in which the n-gram the history ends with is planted ONCE: ending at e = n - 1 (the first place a match can end) or at
    e = p - 1 (the last one; there it overlaps the tail, so the n + 1 tokens up to p are one symbol)"""
    from hqq_amd import ops
    base = np.random.RandomState(5).randint(0, 1 << 40, CAP, dtype=np.int64)
    hist = _dev(base)
    p_dev = torch.zeros(1, dtype=torch.int64, device="cuda")
    ran = 0
    for n in (1, 2, 3, 4):
        for p in (2 * n, 1023, 1024, 1025, 29999):
            h = base.copy()
            if where == "start":
                h[0:n] = h[p - n + 1:p + 1]
            else:
                h[p - n:p + 1] = h[p]
            hist.copy_(_dev(h))
            for R in (2, 8, 16):
                for N in (n, 4):
                    p_dev.fill_(p)
                    tok = torch.zeros(R, dtype=torch.int64, device="cuda")
                    pos = torch.zeros(R, dtype=torch.int64, device="cuda")
                    ops.spec_propose(hist, p_dev, tok, pos, N)
                    want, _ = sc.propose_ref(h, p, R, N)
                    assert tok.tolist() == want.tolist(), (where, n, p, R, N)
                    e = n - 1 if where == "start" else p - 1
                    assert int(tok[1]) == int(h[e + 1]), "the planted match was taken"   # (the continuation of the planted place)
                    ran += 1
    assert ran == 4 * 5 * 3 * 2


def test_propose_outside_the_history_reads_nothing():
    from hqq_amd import ops
    hist = torch.arange(1, 9, device="cuda")
    for p in (8, -1, 1 << 40):
        tok = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        pos = torch.full((4,), -7, dtype=torch.int64, device="cuda")
        ops.spec_propose(hist, torch.tensor([p], device="cuda"), tok, pos, 3)
        assert tok.tolist() == [0, 0, 0, 0] and pos.tolist() == [p + i for i in range(4)]


# ---- the accept step ------------------------------------------------------------------------------------------------------------------------------
def _accept_on_gpu(g, tok, hist, p, last, eos, done, steps, tokens):
    from hqq_amd import ops
    s = _dev([p, last, eos, done, steps, tokens])
    h = _dev(hist)
    ops.spec_accept(_dev(g), _dev(tok), h, s[0:1], s[1:2], s[2:3], s[3:4], s[4:5], s[5:6])
    v = s.tolist()
    return h.cpu().numpy(), v[0], v[3], v[4], v[5], v[1], v[2]


@pytest.mark.parametrize("R", [2, 8, 16])
def test_accept_equals_the_host_rule(R):
    """the first mismatch at every row and nowhere; EOS at every row, inside and past the accepted prefix, and absent; `last` cutting the prefix after 1 and 3
    tokens and not at all; the counters from a nonzero start"""
    hist = np.arange(1000, 1064)
    p = 20
    g = [500 + i for i in range(R)]
    n_cases, committed = 0, set()
    for miss in range(1, R + 1):                       # the first row whose input token is not the model's; R: none
        tok = [hist[p]] + [g[i - 1] for i in range(1, R)]
        if miss < R:
            tok[miss] = 77
            if miss + 1 < R:
                assert tok[miss + 1] == g[miss]        # the rows behind the mismatch match again: they must not count
        for eos_row in [None] + list(range(R)):
            eos = -1 if eos_row is None else g[eos_row]
            for room in (1, 3, 40):
                want = sc.accept_ref(g, tok, hist, p, p + room, eos, 0, 5, 11)
                got = _accept_on_gpu(g, tok, hist, p, p + room, eos, 0, 5, 11)
                assert got[0].tolist() == want[0].tolist() and got[1:5] == tuple(int(x) for x in want[1:]), (miss, eos_row, room, got[1:5], want[1:])
                assert got[5:] == (p + room, eos)      # last and eos are inputs
                n_cases += 1
                committed.add(want[1] - p)
    assert n_cases == R * (R + 1) * 3 and committed == set(range(1, R + 1))   # every prefix length occurred


@pytest.mark.parametrize("R", [2, 16])
def test_accept_leaves_a_frozen_state_untouched(R):
    hist = np.arange(1000, 1064)
    g = [500 + i for i in range(R)]
    tok = [1020] + g[:-1]
    for p, last, done in ((20, 40, 1), (20, 20, 0), (21, 20, 0), (40, 40, 7), (-1, 40, 0), (20, 64, 0)):   # done; p >= last; a p / last outside the history
        got = _accept_on_gpu(g, tok, hist, p, last, g[0], done, 5, 11)
        assert got[0].tolist() == hist.tolist() and got[1:] == (p, done, 5, 11, last, g[0]), (p, last, done)


# ---- the shared-cache glue kernels ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("first", [3, 29])
def test_rope_cache_shared_equals_batch1_calls(dt, first):
    """rows at positions 3 .. 7, and 29 .. 33 on a cache of 32 (the last two write nothing): q_out and EVERY cache slot are those of R batch-1 calls"""
    from hqq_amd import ops
    R, nh, nkv, hd, L = 5, 4, 2, 64, 32
    g = torch.Generator(device="cuda").manual_seed(first)
    q = torch.randn(R, nh * hd, device="cuda", generator=g).to(dt)
    k = torch.randn(R, nkv * hd, device="cuda", generator=g).to(dt)
    v = torch.randn(R, nkv * hd, device="cuda", generator=g).to(dt)
    cos = torch.randn(R, hd, device="cuda", generator=g).to(dt)
    sin = torch.randn(R, hd, device="cuda", generator=g).to(dt)
    pos = torch.arange(first, first + R, device="cuda")
    kc = torch.full((1, nkv, L, hd), -3.0, dtype=dt, device="cuda")    # a sentinel no rotated value equals in every element
    vc = torch.full((1, nkv, L, hd), -5.0, dtype=dt, device="cuda")
    kc1, vc1 = kc[0].clone(), vc[0].clone()
    qr = torch.full((R, nh, 1, hd), float("nan"), dtype=dt, device="cuda")
    ops.rope_cache_shared(q, k, v, cos, sin, pos, kc, vc, qr)
    for i in range(R):
        qr1 = torch.empty(1, nh, 1, hd, dtype=dt, device="cuda")
        ops.rope_cache(q[i], k[i], v[i], cos[i], sin[i], pos[i:i + 1], kc1, vc1, qr1)
        assert torch.equal(qr[i], qr1[0]), i
    assert torch.equal(kc[0], kc1) and torch.equal(vc[0], vc1)
    written = [int(x) for x in pos.tolist() if x < L]
    for j in range(L):
        assert bool((kc[0, :, j] == -3.0).all()) == (j not in written) and bool((vc[0, :, j] == -5.0).all()) == (j not in written), j
    # the [n_kv, L, hd] view of the same tensors is the same call
    kc2, vc2 = torch.full_like(kc1, -3.0), torch.full_like(vc1, -5.0)
    ops.rope_cache_shared(q, k, v, cos, sin, pos, kc2, vc2, torch.empty_like(qr))
    assert torch.equal(kc2, kc1) and torch.equal(vc2, vc1)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
@pytest.mark.parametrize("hd", ac.HDS)
@pytest.mark.parametrize("heads", [(4, 4), (8, 2)], ids=["mha", "gqa8over2"])
def test_attn_decode_shared_rows_equal_attn_decode(dt, hd, heads):
    """row i of the shared launch is attn_decode at row i's position, torch.equal: rows straddling a multiple of the kernel's key step, the 1024 | 1025 boundary,
    and on a cache of 2048 the share edges of 2 and 3 splits up to the last slot; the cache holds NaN beyond the last row's position"""
    from hqq_amd import ops
    T = ac.DT[dt]
    nh, nkv = heads
    L = 2048
    g = torch.Generator(device="cuda").manual_seed(hd + nh)
    kc0 = torch.randn(nkv, L, hd, device="cuda", generator=g).to(T)
    vc0 = torch.randn(nkv, L, hd, device="cuda", generator=g).to(T)
    scaling = hd ** -0.5
    st = ac.step(hd)
    ran = 0
    for R in (2, 8, 16):
        q = torch.randn(R, nh * hd, device="cuda", generator=g).to(T)
        starts = {1: [3 * st - R // 2, 4 * 4 * st - 1, 1025 - R // 2 - 1, 0], 2: [1025 - R // 2 - 1, L - R, 3], 3: [1025 - R // 2 - 1, L - R, 1536 - R // 2]}
        for S, p0s in starts.items():
            for p0 in p0s:
                pos = torch.arange(p0, p0 + R, device="cuda")
                assert p0 >= 0 and p0 + R <= L
                kc, vc = kc0.clone(), vc0.clone()
                kc[:, p0 + R:] = float("nan")
                vc[:, p0 + R:] = float("nan")
                out = torch.full((R, nh * hd), float("nan"), dtype=T, device="cuda")
                ops.attn_decode_shared(q, kc.view(1, nkv, L, hd), vc.view(1, nkv, L, hd), pos, out, scaling, splits=S)
                assert bool(torch.isfinite(out).all()), (R, S, p0)
                for i in range(R):
                    o1 = torch.empty(nh * hd, dtype=T, device="cuda")
                    ops.attn_decode(q[i], kc, vc, pos[i:i + 1], o1, scaling, splits=S)
                    assert torch.equal(out[i], o1), (R, S, p0, i)
                ran += 1
    assert ran == 3 * 10


# ---- the verify step --------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny():
    return _quantised(_tiny_llama())


def _prefilled(model, ids, L):
    from transformers import StaticCache
    cache = StaticCache(config=model.config, max_cache_len=L)
    with torch.no_grad():
        out = model(ids, past_key_values=cache, cache_position=torch.arange(ids.shape[1], device="cuda"), use_cache=True)
    return cache, out.logits[:, -1]


def test_verify_step_is_causal_and_follows_the_models_forward(tiny):
    """8 rows = 8 true tokens of one sequence: (1) replacing the rows behind row i changes no bit of the logits of rows <= i (the same row index and launch shapes:
    no tolerance applies); (2) every row's logits are the model's own forward on the whole sequence at that position, within the band test_batch_decode_gpu
    holds the batched kernel-attention step to"""
    from hqq_amd.utils.llama_fused import FusedLlamaStep, supports_speculation
    model, L, T, R = tiny, 64, 7, 8
    assert supports_speculation(model, R) and not supports_speculation(model, 17) and not supports_speculation(model, 1)
    seq = torch.randint(0, 512, (1, T + R), generator=torch.Generator().manual_seed(3)).cuda()
    cache, _ = _prefilled(model, seq[:, :T], L)
    step = FusedLlamaStep(model, cache, L, attention="hip", batch=R, verify=True)
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
        assert not torch.equal(other[i + 1:], true[i + 1:]), i      # (the replaced rows did change something)


def test_verify_step_refuses_everything_else(tiny):
    from transformers import StaticCache
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    model, L = tiny, 64
    cache, _ = _prefilled(model, torch.randint(0, 512, (1, 5)).cuda(), L)
    FusedLlamaStep(model, cache, L, attention="hip", batch=2, verify=True)
    for kw in (dict(attention="sdpa", batch=8), dict(attention="hip", batch=1), dict(attention="hip", batch=17), dict(attention="hip", batch=8, axis0=True),
               dict(attention="hip", batch=8, qk_norm=True), dict(attention="hip", batch=8, kv_cache="q8"), dict(attention="hip", batch=8, glue="folded")):
        with pytest.raises(ValueError):
            FusedLlamaStep(model, cache, L, verify=True, **kw)
    wide = StaticCache(config=model.config, max_cache_len=L)
    wide.early_initialization(8, 4, 64, torch.float16, torch.device("cuda"))
    with pytest.raises(ValueError, match="batch 1"):   # the rows share ONE sequence's cache
        FusedLlamaStep(model, wide, L, attention="hip", batch=8, verify=True)


# ---- the decoder ------------------------------------------------------------------------------------------------------------------------------------
def _plain_route(model, ids, n, L):
    """greedy decoding through the plain one-row step with the kernel attention, by hand: (tokens [1, T + n], the top-1 / top-2 logit gap of every decode step)"""
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    T = ids.shape[1]
    cache, logits = _prefilled(model, ids, L)
    step = FusedLlamaStep(model, cache, L, attention="hip")
    tok = logits.argmax(-1, keepdim=True)
    toks, gaps = [tok], []
    for t in range(n - 1):
        lg = step(tok, torch.tensor([T + t], device="cuda"), L).float()
        top = lg.view(-1).topk(2).values
        gaps.append(float(top[0] - top[1]))
        tok = lg.argmax(-1, keepdim=True)
        toks.append(tok)
    return torch.cat([ids] + toks, dim=1), gaps


@pytest.fixture(scope="module")
def plain(tiny):
    """per prompt of _spec_cases.E2E_PROMPTS: (ids, the plain route's tokens, its gaps), computed once"""
    out = []
    for seed, repeated in sc.E2E_PROMPTS:
        ids = torch.tensor([sc.e2e_prompt(seed, repeated)], device="cuda")
        out.append((ids, repeated) + _plain_route(tiny, ids, sc.NEW_TOKENS, sc.CACHE_LEN))
    return out


def test_the_prompts_keep_the_guard_band(tiny, plain):
    """a set-up check, on the plain route alone: the one-row and the R-row kernels round differently, so equal tokens can only be asked where no step's two best
    logits are within 0.05 — four times the 5e-3 (1 + |logit|) band the batched step is held to.  A prompt that breaks it fails here; none may be dropped"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    assert len(sc.E2E_PROMPTS) == 4 and sum(r for _, r in sc.E2E_PROMPTS) == 2
    dec = GraphedGreedyDecoder(tiny, max_cache_len=sc.CACHE_LEN, attention="hip")
    for (seed, _), (ids, _, toks, gaps) in zip(sc.E2E_PROMPTS, plain):
        print(f"seed {seed}: smallest top-1 / top-2 gap over {len(gaps)} steps {min(gaps):.4f}")
        assert len(gaps) == sc.NEW_TOKENS - 1 and min(gaps) > sc.GAP, (seed, min(gaps))
        assert torch.equal(dec.generate(ids, sc.NEW_TOKENS), toks), seed      # the decoder's plain route is that step
    assert not dec.speculating and dec.spec_stats == {"steps": 0, "tokens": 0}


def test_speculative_decoding_emits_the_plain_tokens(tiny, plain):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    R = 8
    dec = GraphedGreedyDecoder(tiny, max_cache_len=sc.CACHE_LEN, attention="hip", speculate="ngram", draft_rows=R, ngram_max=3)
    eager = GraphedGreedyDecoder(tiny, max_cache_len=sc.CACHE_LEN, attention="hip", speculate="ngram", draft_rows=R, ngram_max=3)
    assert dec.speculating
    for ids, repeated, toks, _ in plain:      # one decoder for all four: the kept state serves the next prompt
        got = dec.generate(ids, sc.NEW_TOKENS)
        assert dec.speculating and torch.equal(got, toks)
        steps, tokens = dec.spec_stats["steps"], dec.spec_stats["tokens"]
        print(f"repeated span {repeated}: {tokens} tokens in {steps} steps")
        assert tokens == sc.NEW_TOKENS - 1 and steps <= tokens <= steps * R
        if repeated:
            assert tokens > steps
        assert torch.equal(eager.generate(ids, sc.NEW_TOKENS, use_graph=False), toks)
        assert eager.spec_stats == dec.spec_stats
    assert dec._spec["graphs"] and not eager._spec["graphs"]
    # other rows and n-gram lengths, a check interval of 1 and one longer than the run: the same tokens
    ids, _, toks, _ = plain[1]
    for R2, N2, every in ((2, 1, 16), (16, 4, 1), (4, 0, 64)):
        d2 = GraphedGreedyDecoder(tiny, max_cache_len=sc.CACHE_LEN, attention="hip", speculate="ngram", draft_rows=R2, ngram_max=N2)
        assert torch.equal(d2.generate(ids, sc.NEW_TOKENS, check_every=every), toks), (R2, N2, every)
        assert d2.spec_stats["tokens"] == sc.NEW_TOKENS - 1
        if N2 == 0:
            assert d2.spec_stats["steps"] <= sc.NEW_TOKENS - 1   # (no n-gram drafts: only a repeated last token can be confirmed)


def _host_loop(model, ids, n, L, R, N):
    """the decoder's loop driven from the host: propose_ref, the verify step run eagerly on those rows, torch's argmax, accept_ref"""
    from hqq_amd.utils.generation import kv_bucket
    from hqq_amd.utils.llama_fused import FusedLlamaStep
    T = ids.shape[1]
    cache, logits = _prefilled(model, ids, L)
    step = FusedLlamaStep(model, cache, L, attention="hip", batch=R, verify=True)
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


def test_the_decoders_loop_equals_a_host_driven_loop(tiny):
    """prompts no guard selects, so drafts get rejected: the captured loop (device state, graphs, warm-up snapshot and restore, host reads every few steps) emits
    exactly what propose_ref / accept_ref around the same verify step emit — the same rows through the same launches, so no tolerance applies"""
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    R, N, L = 8, 3, sc.CACHE_LEN
    dec = GraphedGreedyDecoder(tiny, max_cache_len=L, attention="hip", speculate="ngram", draft_rows=R, ngram_max=N)
    seen = set()
    for seed, repeated in sc.LOOSE_PROMPTS:
        ids = torch.tensor([sc.e2e_prompt(seed, repeated)], device="cuda")
        want, steps, tokens, accepted = _host_loop(tiny, ids, sc.NEW_TOKENS, L, R, N)
        print(f"seed {seed}: tokens per step {accepted}")
        for every in (16, 3):
            got = dec.generate(ids, sc.NEW_TOKENS, check_every=every)
            assert torch.equal(got, want), (seed, every)
            assert dec.spec_stats == {"steps": steps, "tokens": tokens} and tokens == sc.NEW_TOKENS - 1
        seen |= set(accepted)
    assert 1 in seen and max(seen) > 1 and any(1 < a < R for a in seen), seen   # rejected at once, confirmed, and cut short part of the way


def test_the_loop_at_a_context_that_splits_the_attention():
    """1100 prompt tokens on a cache of 2048: every step's bucket is 2048, so the shared attention runs with 4 splits, its workspace and the merging launch inside
    the captured step; a long random prompt over 512 symbols also gives the proposer matches of every length to choose from.  Exact, as above"""
    from hqq_amd import ops
    from hqq_amd.utils.generation import GraphedGreedyDecoder, kv_bucket
    model = _quantised(_tiny_llama(max_position_embeddings=2048))
    R, N, L, T = 8, 3, 2048, 1100
    assert ops.attn_splits(kv_bucket(T + R - 1, "hip", L)) == 4
    ids = torch.randint(0, 512, (1, T), generator=torch.Generator().manual_seed(11)).cuda()
    want, steps, tokens, accepted = _host_loop(model, ids, 40, L, R, N)
    print(f"tokens per step {accepted}")
    dec = GraphedGreedyDecoder(model, max_cache_len=L, attention="hip", speculate="ngram", draft_rows=R, ngram_max=N)
    for _ in range(2):   # fresh (the first step eager, then captured), and kept
        assert torch.equal(dec.generate(ids, 40, check_every=5), want)
        assert dec.speculating and dec.spec_stats == {"steps": steps, "tokens": tokens} and list(dec._spec["graphs"]) == [2048]


def test_the_eos_cut_is_the_plain_routes(tiny, plain):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    dec = GraphedGreedyDecoder(tiny, max_cache_len=sc.CACHE_LEN, attention="hip", speculate="ngram")
    one = GraphedGreedyDecoder(tiny, max_cache_len=sc.CACHE_LEN, attention="hip")
    for ids, _, toks, _ in plain:
        T = ids.shape[1]
        for at in (0, 1, 10, 30):
            eos = int(toks[0, T + at])
            want = one.generate(ids, sc.NEW_TOKENS, eos_token_id=eos, check_every=4)
            got = dec.generate(ids, sc.NEW_TOKENS, eos_token_id=eos, check_every=4)
            assert torch.equal(got, want) and int(got[0, -1]) == eos and got.shape[1] <= T + at + 1, (at, got.shape)
        absent = next(t for t in range(512) if t not in toks[0].tolist())
        assert torch.equal(dec.generate(ids, sc.NEW_TOKENS, eos_token_id=absent), toks)
        assert torch.equal(dec.generate(ids, 1), toks[:, :T + 1])


def test_hfgenerator_passes_the_keywords_on(tiny):
    from hqq_amd.utils.generation import HFGenerator
    from test_model_gpu import _ToyTokenizer
    gen = HFGenerator(tiny, _ToyTokenizer(), max_new_tokens=16, compile="partial", speculate="ngram", draft_rows=4, ngram_max=2, attention="hip")
    ref = HFGenerator(tiny, _ToyTokenizer(), max_new_tokens=16, compile="partial", attention="hip")
    assert gen.decoder.speculating and gen.decoder.draft_rows == 4 and gen.decoder.ngram_max == 2 and not ref.decoder.speculating
    r = gen.generate("7 8 9 10 11 7 8 9", use_chat_template=False, verbose=False)
    assert gen.decoder.spec_stats["tokens"] >= 1 and set(r) == {"output_text", "output_tokens", "input_tokens"} and r["output_tokens"].numel() == 16
    assert not HFGenerator(tiny, _ToyTokenizer(), max_new_tokens=16, speculate="ngram").decoder.speculating     # (HF's attention function: not served)


@pytest.mark.parametrize("which", ["sdpa", "q8", "axis0"])
def test_unsupported_requests_decode_as_before(which, tiny):
    from hqq_amd.utils.generation import GraphedGreedyDecoder
    if which == "axis0":
        from hqq_amd.core.quantize import BaseQuantizeConfig
        from hqq_amd.utils.model import quantize_model
        from hqq_amd.utils.patching import prepare_for_inference
        model = _tiny_llama()
        quantize_model(model, BaseQuantizeConfig(nbits=4, group_size=64, axis=0), compute_dtype=torch.float16, device="cuda")
        prepare_for_inference(model, backend="hip")
        kw = dict(attention="hip", axis0="fused")
    else:
        model = tiny
        kw = dict(attention="sdpa") if which == "sdpa" else dict(attention="hip", kv_cache="q8")
    ids = torch.tensor([sc.e2e_prompt(1, True)], device="cuda")
    dec = GraphedGreedyDecoder(model, max_cache_len=64, speculate="ngram", **kw)
    got = dec.generate(ids, 12)
    assert not dec.speculating and dec._spec is None and dec.spec_stats == {"steps": 0, "tokens": 0}
    assert torch.equal(got, GraphedGreedyDecoder(model, max_cache_len=64, **kw).generate(ids, 12))
