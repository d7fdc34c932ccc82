"""Speculative greedy decoding by prompt lookup, the part that needs no GPU: the host restatements of the proposer and the accept step (tests/_spec_cases.py)
on hand-written cases, the whole loop on the host against plain greedy decoding, argument validation of the four entry points through the library (which
validates before it launches), the coverage rule and the keyword errors."""
import itertools

import numpy as np
import pytest

from _spec_cases import ACCEPT_CASES, PROPOSE_CASES, accept_ref, greedy, propose_ref, speculative, toy_models

P16 = 16    # a stand-in pointer: every call below must be refused before anything touches it


@pytest.mark.parametrize("case", PROPOSE_CASES, ids=[c[0] for c in PROPOSE_CASES])
def test_propose_ref_on_hand_written_cases(case):
    _, hist, p, R, N, want = case
    tok, pos = propose_ref(hist, p, R, N)
    assert tok.tolist() == want
    assert pos.tolist() == [p + i for i in range(R)] and tok.dtype == pos.dtype == np.int64


def test_propose_ref_against_a_literal_search():
    """the header's sentence word for word — every n from the largest down, every e, slices compared as lists — on all histories of 7 tokens over 2 symbols and
    on random ones over 3: propose_ref's vectorised search finds the same (n, e)"""
    def literal(hist, p, R, N):
        for n in range(min(N, p), 0, -1):
            es = [e for e in range(n - 1, p) if list(hist[e - n + 1:e + 1]) == list(hist[p - n + 1:p + 1])]
            if es:
                ext = list(hist[:p + 1])
                for i in range(1, R):
                    ext.append(ext[max(es) + i])
                return ext[p:]
        return [hist[p]] * R
    rng = np.random.RandomState(0)
    hists = [list(h) for h in itertools.product((0, 1), repeat=7)] + [rng.randint(0, 3, 24).tolist() for _ in range(200)]
    for hist in hists:
        for p in (0, 1, 2, 4, len(hist) - 1):
            for R, N in ((2, 1), (5, 2), (16, 4), (8, 3), (4, 0)):
                assert propose_ref(hist, p, R, N)[0].tolist() == literal(hist, p, R, N), (hist, p, R, N)


def test_propose_ref_outside_the_history():
    tok, pos = propose_ref([1, 2, 3], 3, 4, 3)
    assert tok.tolist() == [0, 0, 0, 0] and pos.tolist() == [3, 4, 5, 6]
    assert propose_ref([1, 2, 3], -1, 2, 3)[0].tolist() == [0, 0]


@pytest.mark.parametrize("case", ACCEPT_CASES, ids=[c[0] for c in ACCEPT_CASES])
def test_accept_ref_on_hand_written_cases(case):
    _, g, tok, p, last, eos, done, n, done_after = case
    hist = np.arange(100, 148)
    got, p2, d2, steps, tokens = accept_ref(g, tok, hist, p, last, eos, done, 7, 30)
    want = hist.copy()
    want[p + 1:p + 1 + n] = g[:n]
    assert got.tolist() == want.tolist() and p2 == p + n and d2 == done_after
    assert (steps, tokens) == ((8, 30 + n) if n else (7, 30))   # a frozen state leaves the counters alone too


@pytest.mark.parametrize("name", sorted(toy_models()))
@pytest.mark.parametrize("R,N", [(2, 1), (4, 2), (8, 3), (16, 4), (8, 0)])
def test_every_accepted_prefix_is_the_true_continuation(name, R, N):
    """brute force over deterministic toy models: after EVERY step of the speculative loop the committed history is a prefix of plain greedy decoding, the loop
    ends with exactly the greedy sequence (cut at `last` and at the first EOS alike), and steps <= tokens <= steps * R"""
    model = toy_models()[name]
    for prompt, n, eos in (([1, 2, 3], 40, -1), ([0], 1, -1), ([2, 2], 2, -1), ([6, 1, 6, 1, 6], 33, -1), ([1, 2, 3], 40, 0), ([3, 1], 25, 4), ([1, 2, 3], 40, 5)):
        want = greedy(model, prompt, n, eos)

        def check(hist, p, want=want):
            assert [int(t) for t in hist[:p + 1]] == want[:p + 1]
        got, steps, tokens = speculative(model, prompt, n, R, N, eos, check)
        assert got == want, (prompt, n, eos)
        assert tokens == len(want) - len(prompt) - 1 and steps <= tokens <= steps * R
    if name in ("pair", "constant", "counter") and N > 0:   # periodic output: the drafts must actually be accepted, or the test above shows nothing about them
        _, steps, tokens = speculative(model, [1, 2, 3], 60, R, N)
        assert tokens > steps


# ---- the library validates before it launches (no GPU is touched: the pointers are stand-ins) ----------------------------------------------------
def _lib():
    from hqq_amd import _C
    return _C.lib()


def _propose(hist=P16, cap=64, p=P16, rows=8, ngram=3, tok=P16, pos=P16):
    return _lib().hqq_hip_spec_propose(hist, cap, p, rows, ngram, tok, pos, None)


def _accept(g=P16, tok=P16, rows=8, hist=P16, cap=64, p=P16, last=P16, eos=P16, done=P16, steps=P16, tokens=P16):
    return _lib().hqq_hip_spec_accept(g, tok, rows, hist, cap, p, last, eos, done, steps, tokens, None)


def _rope(q=P16, k=P16, v=P16, cos=P16, sin=P16, pos=P16, rows=8, q_out=P16, kc=P16, vc=P16, n_heads=4, n_kv=2, hd=64, L=32, dtype=1):
    return _lib().hqq_hip_rope_cache_shared(q, k, v, cos, sin, pos, rows, q_out, kc, vc, n_heads, n_kv, hd, L, dtype, None)


def _attn(q=P16, kc=P16, vc=P16, pos=P16, rows=8, out=P16, n_heads=4, n_kv=2, hd=64, L=32, dtype=1, splits=1, ws=None, ws_bytes=0):
    return _lib().hqq_hip_attn_decode_shared(q, kc, vc, pos, rows, out, n_heads, n_kv, hd, L, 0.125, dtype, splits, ws, ws_bytes, None)


def test_bad_arguments_are_refused_before_any_launch():
    err = _lib().hqq_hip_last_error
    for name in ("hist", "p", "tok", "pos"):
        assert _propose(**{name: None}) == -2 and b"hqq_hip_spec_propose" in err()
    for bad in (dict(rows=1), dict(rows=17), dict(rows=0), dict(ngram=-1), dict(ngram=5), dict(cap=0), dict(cap=1 << 31)):
        assert _propose(**bad) == -2, bad
    for name in ("g", "tok", "hist", "p", "last", "eos", "done", "steps", "tokens"):
        assert _accept(**{name: None}) == -2 and b"hqq_hip_spec_accept" in err()
    for bad in (dict(rows=1), dict(rows=17), dict(cap=0), dict(cap=1 << 31)):
        assert _accept(**bad) == -2, bad
    for name in ("q", "k", "v", "cos", "sin", "pos", "q_out", "kc", "vc"):
        assert _rope(**{name: None}) == -2 and b"hqq_hip_rope_cache_shared" in err()
    for bad in (dict(rows=0), dict(rows=65536), dict(hd=63), dict(hd=0), dict(n_kv=0), dict(L=0)):
        assert _rope(**bad) == -2, bad
    assert _rope(dtype=0) == -4
    for name in ("q", "kc", "vc", "pos", "out"):
        assert _attn(**{name: None}) == -2 and b"hqq_hip_attn_decode_shared" in err()
    for bad in (dict(rows=0), dict(n_heads=3), dict(L=30001), dict(splits=0), dict(splits=65), dict(splits=2), dict(splits=2, ws=P16, ws_bytes=8 * 4 * 2 * 66 * 4 - 1)):
        assert _attn(**bad) == -2, bad
    assert _attn(hd=96) == -4 and _attn(dtype=0) == -4
    assert _attn(q=24) == -6


def test_ops_wrappers_refuse_what_the_library_would():
    import torch
    from hqq_amd import ops
    z = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.spec_propose(z, z[:1], z, z, 3)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.spec_accept(z, z, z, z[:1], z[:1], z[:1], z[:1], z[:1], z[:1])
    assert ops.SPEC_MAX_ROWS == ops.GEMV_MAX_M == 16 and ops.SPEC_MAX_NGRAM == 4


# ---- the coverage rule and the keywords ----------------------------------------------------------------------------------------------------------
def _tiny_llama():
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    torch.manual_seed(0)
    return LlamaForCausalLM(LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, num_key_value_heads=2, vocab_size=64,
                                        max_position_embeddings=64))


def test_supports_speculation_refuses_what_the_step_does_not_serve():
    from hqq_amd.utils import llama_fused
    model = _tiny_llama()
    assert llama_fused.arch_supported(model)
    for rows in (8, 2, 16):
        assert not llama_fused.supports_speculation(model, rows)          # dense fp32 linears on the CPU: no quantised layers to serve
    for rows in (1, 0, 17, -3, True, 8.0, None, "8"):
        assert not llama_fused.supports_speculation(model, rows)
    assert not llama_fused.supports_speculation(object(), 8)


def test_generation_front_ends_check_the_speculation_keywords():
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator, check_speculation
    model = _tiny_llama()
    for make in (lambda **kw: GraphedGreedyDecoder(model, max_cache_len=32, **kw), lambda **kw: HFGenerator(model, tokenizer=None, max_new_tokens=8, **kw)):
        for bad in ("bad", "draft", "Ngram", "", True, 1):
            with pytest.raises(ValueError, match="speculate"):
                make(speculate=bad)
        for bad in (1, 0, 17, 8.0, True, None, "8"):
            with pytest.raises(ValueError, match="draft_rows"):
                make(speculate="ngram", draft_rows=bad)
        for bad in (-1, 5, 3.0, True, None):
            with pytest.raises(ValueError, match="ngram_max"):
                make(speculate="ngram", ngram_max=bad)
        with pytest.raises(ValueError, match="greedy"):
            make(speculate="ngram", do_sample=True)
    check_speculation(None, 8, 3, True)       # sampling without speculation stays what it was
    check_speculation("ngram", 2, 0, False)
    check_speculation("ngram", 16, 4, False)
