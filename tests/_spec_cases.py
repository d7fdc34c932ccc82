"""Shared by tests/test_spec_cpu.py and tests/test_spec_gpu.py: the host restatements of the two integer kernels of speculative decoding
(csrc/spec.hip; include/hqq_hip.h states both rules), hand-written cases for them, a host model of the whole loop, and the prompts of the end-to-end test.

propose_ref / accept_ref follow the header's text, not the kernels' code: the proposer searches n from the largest down and e from the latest down with
whole-slice compares (the kernel counts match lengths per end position and reduces four maxima), the accept step walks the rows one by one (the kernel
uses two ballots).  The GPU file compares the kernels with them bit for bit."""
from __future__ import annotations

import numpy as np

MAX_ROWS, MAX_NGRAM = 16, 4


def propose_ref(hist, p: int, R: int, N: int):
    """(tok [R], pos [R]) int64: tok[0] = hist[p], pos[i] = p + i; the drafts by the rule of hqq_hip_spec_propose.  A p outside the history: tok = 0"""
    hist = np.asarray(hist, dtype=np.int64)
    pos = p + np.arange(R, dtype=np.int64)
    if p < 0 or p >= hist.shape[0]:
        return np.zeros(R, dtype=np.int64), pos
    e_best = -1
    for n in range(min(N, p), 0, -1):
        # hit[k]: the n tokens ending at e = n - 1 + k equal the n tokens ending at p, for e in [n - 1, p - 1]
        hit = np.ones(p - n + 1, dtype=bool)
        for j in range(n):
            hit &= hist[n - 1 - j:p - j] == hist[p - j]
        where = np.flatnonzero(hit)
        if where.size:
            e_best = n - 1 + int(where[-1])
            break
    tok = np.empty(R, dtype=np.int64)
    tok[0] = hist[p]
    for i in range(1, R):
        m = e_best + i
        tok[i] = hist[p] if e_best < 0 else (hist[m] if m <= p else tok[m - p])
    return tok, pos


def accept_ref(g, tok, hist, p: int, last: int, eos: int, done: int, steps: int, tokens: int):
    """the state after hqq_hip_spec_accept: (hist (a copy), p, done, steps, tokens)"""
    hist = np.array(hist, dtype=np.int64)
    R = len(g)
    if done != 0 or p >= last or p < 0 or last >= hist.shape[0]:
        return hist, p, done, steps, tokens
    a = 0
    while a + 1 < R and tok[a + 1] == g[a] and p + (a + 1) + 1 <= last:
        a += 1
    for i in range(a + 1):
        if g[i] == eos:
            a, done = i, 1
            break
    for i in range(a + 1):
        hist[p + 1 + i] = g[i]
    return hist, p + a + 1, done, steps + 1, tokens + a + 1


# ---- hand-written proposer cases: (name, hist, p, R, N, tok) ---------------------------------------------------------------------------------
PROPOSE_CASES = [
    # the history ends with 2 3.  "2 3" occurred once, early (ending at e = 2, continuation 9 ...); "3" alone occurred later (e = 5, continuation 8 ...).
    # The longer n-gram wins although its match is the older one; past p the drafts repeat themselves with period p - e = 6
    ("longest n beats the latest match", [1, 2, 3, 9, 7, 3, 8, 2, 3], 8, 8, 3, [3, 9, 7, 3, 8, 2, 3, 9]),
    ("with N = 1 the latest match of the last token is taken", [1, 2, 3, 9, 7, 3, 8, 2, 3], 8, 8, 1, [3, 8, 2, 3, 8, 2, 3, 8]),
    ("a match at the very start (e = n - 1 = 0)", [5, 6, 1, 2, 5], 4, 8, 3, [5, 6, 1, 2, 5, 6, 1, 2]),
    ("period 1: the continuation is the drafts themselves", [4, 7, 7], 2, 6, 3, [7, 7, 7, 7, 7, 7]),
    ("period 2", [1, 2, 1, 2], 3, 8, 3, [2, 1, 2, 1, 2, 1, 2, 1]),
    ("no match: every draft is the last token", [1, 2, 3, 4], 3, 4, 4, [4, 4, 4, 4]),
    ("N = 0 proposes nothing, although 3 occurred before", [3, 5, 3, 6], 2, 4, 0, [3, 3, 3, 3]),
    ("the same history with N = 1", [3, 5, 3, 6], 2, 4, 1, [3, 5, 3, 5]),
    ("p = 0: nothing lies before the last token", [9, 1, 1, 1], 0, 3, 4, [9, 9, 9]),
    ("tokens beyond p are not history", [1, 2, 8, 2, 8], 1, 4, 2, [2, 2, 2, 2]),
    ("n is capped by p: at p = 1 only the last token can match", [6, 6, 0, 0], 1, 2, 4, [6, 6]),
]

# ---- hand-written accept cases: (name, g, tok, p, last, eos, done) -> (a + 1 tokens committed, done) ------------------------------------------
ACCEPT_CASES = [
    ("every draft confirmed", [11, 12, 13, 14], [10, 11, 12, 13], 5, 40, -1, 0, 4, 0),
    ("the first draft is wrong: one token, the model's own", [11, 12, 13, 14], [10, 99, 98, 97], 5, 40, -1, 0, 1, 0),
    ("a mismatch at row 2", [11, 12, 13, 14], [10, 11, 99, 13], 5, 40, -1, 0, 2, 0),
    ("a later row that matches again does not count", [11, 12, 13, 14], [10, 99, 12, 13], 5, 40, -1, 0, 1, 0),
    ("`last` cuts the prefix", [11, 12, 13, 14], [10, 11, 12, 13], 5, 7, -1, 0, 2, 0),
    ("EOS inside the prefix ends the sequence there", [11, 12, 13, 14], [10, 11, 12, 13], 5, 40, 12, 0, 2, 1),
    ("EOS as the first emitted token", [11, 12, 13, 14], [10, 11, 12, 13], 5, 40, 11, 0, 1, 1),
    ("EOS past the accepted prefix is not seen", [11, 12, 13, 14], [10, 11, 99, 13], 5, 40, 14, 0, 2, 0),
    ("done: frozen", [11, 12, 13, 14], [10, 11, 12, 13], 5, 40, -1, 1, 0, 1),
    ("p == last: frozen", [11, 12, 13, 14], [10, 11, 12, 13], 5, 5, -1, 0, 0, 0),
]


# ---- the whole loop on the host: greedy decoding of a deterministic `model` (prefix -> next token) with and without speculation ---------------
def greedy(model, prompt, n: int, eos: int = -1):
    seq = list(prompt)
    for _ in range(n):
        seq.append(model(seq))
        if seq[-1] == eos:
            break
    return seq


def speculative(model, prompt, n: int, R: int, N: int, eos: int = -1, check=None):
    """the decoder's loop with propose_ref / accept_ref: returns (sequence, steps, tokens).  `check(hist, p)` is called after every step"""
    T = len(prompt)
    hist = np.zeros(T + n + 1, dtype=np.int64)
    hist[:T] = prompt
    hist[T] = model(list(prompt))
    p, last, done, steps, tokens = T, T + n - 1, int(hist[T] == eos), 0, 0
    while not done and p < last:
        tok, _ = propose_ref(hist, p, R, N)
        g = [model(list(hist[:p]) + [int(t) for t in tok[:i + 1]]) for i in range(R)]   # row i: the model on the committed tokens and drafts 1 .. i
        hist, p, done, steps, tokens = accept_ref(g, tok, hist, p, last, eos, done, steps, tokens)
        if check is not None:
            check(hist, p)
    return [int(t) for t in hist[:p + 1]], steps, tokens


def toy_models():
    """deterministic next-token rules over small alphabets: a pure function of the last two tokens (its greedy output becomes periodic, drafts get accepted), one
    that also depends on the position (periods break, drafts get rejected), a constant one (period 1)"""
    return {
        "pair": lambda s: (3 * s[-1] + 5 * (s[-2] if len(s) > 1 else 1) + 1) % 7,
        "positional": lambda s: (s[-1] + (len(s) % 5 == 0) + 2 * (len(s) % 11 == 0)) % 5,
        "constant": lambda s: 4,
        "counter": lambda s: (s[-1] + 1) % 23,
    }


# ---- the end-to-end test's prompts (tests/test_spec_gpu.py) ----------------------------------------------------------------------------------
VOCAB, NEW_TOKENS, CACHE_LEN, GAP = 512, 48, 128, 0.05


def e2e_prompt(seed: int, repeated: bool):
    """a seeded prompt over the tiny model's vocabulary, as a list: 12 random tokens, or (repeated) 3 random tokens, a span of 6, 2 more, and the span again"""
    rng = np.random.RandomState(seed)
    if not repeated:
        return [int(t) for t in rng.randint(0, VOCAB, 12)]
    head, span, mid = rng.randint(0, VOCAB, 3), rng.randint(0, VOCAB, 6), rng.randint(0, VOCAB, 2)
    return [int(t) for t in np.concatenate([head, span, mid, span])]


# (seed, repeated span): picked on an MI355X by the plain route's guard alone — every decode step's top-1 / top-2 logit gap above GAP on the tiny fp16 model
# with attention="hip" — among seeds 0 .. 399 in ascending order, the first two of each kind; test_spec_gpu.py re-checks the guard on every run
E2E_PROMPTS = ((30, False), (77, False), (32, True), (106, True))
# What keeps that guard on a random-weight model is a greedy output that falls into a fixed point at once, so on these four every draft is confirmed.  The loop's
# other half — drafts rejected, prefixes cut — is checked on LOOSE_PROMPTS, which no guard selects: there the decoder is compared with a host-driven loop over the
# same verify step (propose_ref / accept_ref around it), whose rows and launch shapes are the decoder's own, so the tokens are equal without any guard
LOOSE_PROMPTS = ((0, True), (1, True), (2, False), (3, True))
