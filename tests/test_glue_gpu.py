"""GPU half of the glue kernels' tests: the five base kernels of csrc/block.hip (add_rmsnorm, rope_cache, silu_mul, token_prologue, argmax_advance and their
*_batched entry points) against the float64 numpy restatements of tests/_glue_cases.py — bit for bit wherever the chain has no transcendental, inside the derived
bands where expf / rsqrtf sit in it (tests/test_glue_cpu.py proves the reference, the bands' caps, and that the cases can fail).  Everything is compared as
16-bit patterns: any NaN equals any NaN, the sign of zero counts, copies are compared payload and all.  Every output buffer starts as a per-element sentinel
pattern with guard elements either side and is compared WHOLE, so a slot the kernel should not have written, or did not write, shows."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _glue_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu

DT = {C.F16: torch.float16, C.BF16: torch.bfloat16}
TYPES = list(C.TYPES)
GUARD = 64   # elements either side of an output (128 bytes: the 16-byte alignment the kernels ask for is kept)


def dev(bits, T):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16).copy()).cuda().view(DT[T])


def host(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


class Out:
    """an output buffer of the given shape inside a sentinel-filled allocation with guards; .t is the tensor a kernel gets"""

    def __init__(self, shape, T, salt=0, fill=None):
        self.T, self.n = T, int(np.prod(shape))
        self.before = C.sentinel((self.n + 2 * GUARD,), salt)
        if fill is not None:
            self.before[GUARD:GUARD + self.n] = np.asarray(fill, dtype=np.uint16).ravel()
        self.full = dev(self.before, T)
        self.t = self.full[GUARD:GUARD + self.n].view(shape)
        self.shape = tuple(shape)

    def start(self):
        """the buffer's content before the call"""
        return self.before[GUARD:GUARD + self.n].reshape(self.shape).copy()

    def get(self, what):
        """the buffer after the call; the guards must be untouched"""
        after = host(self.full)
        assert np.array_equal(after[:GUARD], self.before[:GUARD]) and np.array_equal(after[-GUARD:], self.before[-GUARD:]), f"{what}: written outside the buffer"
        return after[GUARD:GUARD + self.n].reshape(self.shape)


# ---- silu_mul ------------------------------------------------------------------------------------------------------------------------------------------------
_S = {}


def _silu_of_every_gate(T):
    """the kernel's T(silu(gate)) for every gate pattern (up = 1.0: the product is exact), one launch of 65,536 elements; shared, never modified"""
    if T not in _S:
        from hqq_amd import ops
        pat = C.all_patterns()
        out = Out((65536,), T)
        ops.silu_mul(dev(pat, T), dev(np.full(65536, C.bits_of([1.0], T)[0]), T), out=out.t)
        _S[T] = out.get("silu_mul")
    return _S[T]


@pytest.mark.parametrize("T", TYPES)
def test_silu_of_every_gate_pattern(T):
    """all 65,536 gates x up = 1.0 and x up = -1.0 (an exact sign flip): decided patterns equal, undecided ones one of the two neighbours, non-finite gates and
    the fp32 range (-0 below about -88.72) by the reference's rule"""
    from hqq_amd import ops
    pat = C.all_patterns()
    undecided = C.check_silu_gate(_silu_of_every_gate(T), pat, T)
    print(f"silu_mul {T}: {undecided} undecided gate patterns, all inside the band")
    out = Out((65536,), T, salt=3)
    ops.silu_mul(dev(pat, T), dev(np.full(65536, C.bits_of([-1.0], T)[0]), T), out=out.t)
    got = out.get("silu_mul")
    C.check_silu_gate(got, pat, T, sign=True)
    C.expect_equal(got, C.neg(_silu_of_every_gate(T)), T, "silu_mul x -1 against x 1")


@pytest.mark.parametrize("T", TYPES)
def test_silu_product_with_every_up_pattern_is_exact(T):
    """16 fixed gates x all 65,536 up patterns: T(S * up) with S the kernel's own T(silu(gate)) of the sweep above — no band"""
    from hqq_amd import ops
    gates = C.silu_fixed_gates(T)
    g, u = np.repeat(gates, 65536), np.tile(C.all_patterns(), gates.size)
    out = Out(g.shape, T, salt=5)
    ops.silu_mul(dev(g, T), dev(u, T), out=out.t)
    C.expect_equal(out.get("silu_mul"), C.mul(_silu_of_every_gate(T)[g], u, T), T, "silu_mul product")


@pytest.mark.parametrize("n", [8, 8 * 257])
@pytest.mark.parametrize("T", TYPES)
def test_silu_shortest_call_and_one_live_thread_in_the_last_workgroup(T, n):
    from hqq_amd import ops
    rng = np.random.default_rng(n)
    g, u = C.bits_of(4.0 * rng.standard_normal(n), T), C.bits_of(rng.standard_normal(n), T)
    out = Out((n,), T, salt=n)
    ops.silu_mul(dev(g, T), dev(u, T), out=out.t)
    got = out.get("silu_mul")
    lo, hi = C.silu_bounds(g, T)
    assert (C.same(got, C.mul(lo, u, T), T) | C.same(got, C.mul(hi, u, T), T)).all()
    C.expect_equal(got, C.mul(_silu_of_every_gate(T)[g], u, T), T, "silu_mul against the sweep's own values")


# ---- rope_cache ------------------------------------------------------------------------------------------------------------------------------------------------
def _run_rope(c, T, single=False):
    """one launch of rope_cache_batched (single: rope_cache, B = 1) on a case of _glue_cases; returns (q_out, k_cache, v_cache, the caches before)"""
    from hqq_amd import ops
    B, n_kv, hd, L = c["q"].shape[0], c["n_kv"], c["hd"], c["L"]
    kc0, vc0 = C.rope_caches(c)
    kc, vc = Out(kc0.shape, T, salt=11, fill=kc0), Out(vc0.shape, T, salt=13, fill=vc0)
    qo = Out(c["q"].shape, T, salt=17)
    pos = torch.tensor(c["pos"], dtype=torch.int64, device="cuda")
    q, k, v, cos, sin = (dev(c[x], T) for x in ("q", "k", "v", "cos", "sin"))
    if single:
        assert B == 1
        ops.rope_cache(q, k, v, cos.view(hd), sin.view(hd), pos, kc.t.view(n_kv, L, hd), vc.t.view(n_kv, L, hd), qo.t)
    else:
        ops.rope_cache_batched(q, k, v, cos, sin, pos, kc.t, vc.t, qo.t)
    return qo.get("q_out"), kc.get("k_cache"), vc.get("v_cache"), kc0, vc0


def _check_rope(c, T, single=False):
    q_out, kc, vc, kc0, vc0 = _run_rope(c, T, single)
    want_q, want_kc, want_vc = C.rope_expect(c, kc0, vc0, T)
    C.expect_equal(q_out, want_q, T, "q_out")
    C.expect_equal(kc, want_kc, T, "k_cache")
    C.expect_equal(vc, want_vc, T, "v_cache", exact=True)      # a copy: NaN payloads too
    for b, p in enumerate(c["pos"]):
        if not 0 <= p < c["L"]:                                 # outside the cache: both caches keep their sentinel fill, bit for bit
            assert np.array_equal(kc[b], kc0[b]) and np.array_equal(vc[b], vc0[b]), (b, p)


@pytest.mark.parametrize("kind", ["mul", "add", "random", "rotary"])
@pytest.mark.parametrize("T", TYPES)
def test_rope_arithmetic_is_exact_on_the_q_path_and_the_k_path(T, kind):
    """_glue_cases.rope_arith_case: every pattern of x1 against each factor (mul) / each second operand (add), 65,536 random pairs per path with cos / sin of
    different halves, a real rotary row; v carries every pattern.  q_out and both caches whole, no tolerance."""
    _check_rope(C.rope_arith_case(kind, T), T)


@pytest.mark.parametrize("n_heads,n_kv,hd", C.ROPE_GEOMETRIES)
@pytest.mark.parametrize("T", TYPES)
def test_rope_geometries_and_positions(T, n_heads, n_kv, hd):
    """the single-sequence entry at L = 1 / pos 0 and L = 16 / pos 0, 15, 16, -1, 2^40, and three sequences at [0, L - 1, L] in one launch: a position outside the
    cache leaves BOTH caches at their sentinel fill and still produces q_out"""
    for L, p in C.ROPE_POSITIONS:
        _check_rope(C.rope_geometry_case(n_heads, n_kv, hd, L, [p], T), T, single=True)
    _check_rope(C.rope_geometry_case(n_heads, n_kv, hd, 16, [0, 15, 16], T), T)


# ---- add_rmsnorm ---------------------------------------------------------------------------------------------------------------------------------------------
def _run_norm(h, delta, w, eps, T):
    from hqq_amd import ops
    hb = Out(h.shape, T, salt=19, fill=h)
    out = Out(h.shape, T, salt=23)
    ops.add_rmsnorm(hb.t, None if delta is None else dev(delta, T), dev(w, T), eps, out=out.t)
    return hb.get("h"), out.get("xn")


@pytest.mark.parametrize("T", TYPES)
def test_rmsnorm_residual_add_is_exact_for_every_pattern(T):
    """every pattern of h against each of add_partners as delta (overflow to inf, subnormal sums, cancellation): the written-back h, exactly.  Without a delta h
    is untouched bit for bit."""
    partners = C.add_partners(T)
    H = 4096
    h = np.tile(C.all_patterns().reshape(16, H), (partners.size, 1))
    delta = np.repeat(partners, 16)[:, None] * np.ones((1, H), dtype=np.uint16)
    w = np.full(H, C.bits_of([1.0], T)[0], dtype=np.uint16)
    got_h, _ = _run_norm(h, delta, w, 1e-5, T)
    C.expect_equal(got_h, C.add(h, delta, T), T, "h + delta")
    got_h, _ = _run_norm(h, None, w, 1e-5, T)
    C.expect_equal(got_h, h, T, "h without delta", exact=True)


@pytest.mark.parametrize("H", C.RMS_EDGE_H)
@pytest.mark.parametrize("T", TYPES)
def test_rmsnorm_dispatch_edges_with_exact_sums(T, H):
    """either side of every dispatch threshold, 1 and 3 rows of different scales, two eps: the sum of squares is exact in fp32 in any order, so only rsqrtf and
    the product's fp32 rounding are in the interval"""
    for rows in (1, 3):
        for eps in C.RMS_EPS:
            h, d, w = C.rms_edge_case(H, rows, eps, T)
            hn, lo, hi, _ = C.rmsnorm_ref(h, d, w, eps, T, exact_sum=True)
            got_h, got = _run_norm(h, d, w, eps, T)
            C.expect_equal(got_h, hn, T, f"h rows={rows} eps={eps}", exact=True)
            C.check_rmsnorm(got, lo, hi, T, f"add_rmsnorm H={H} rows={rows} eps={eps}")


@pytest.mark.parametrize("T", TYPES)
def test_rmsnorm_random_rows_inside_the_derived_interval_and_twice_the_same(T):
    from hqq_amd import ops
    for H in C.RMS_RANDOM_H[T]:
        h, d, w = C.rms_random_case(H, T)
        hn, lo, hi, _ = C.rmsnorm_ref(h, d, w, C.RMS_EPS[0], T)
        got_h, got = _run_norm(h, d, w, C.RMS_EPS[0], T)
        C.expect_equal(got_h, hn, T, "h")
        share = C.check_rmsnorm(got, lo, hi, T, f"add_rmsnorm random H={H}")
        print(f"add_rmsnorm {T} random H={H}: inside the interval, {100 * share:.2f} % decided")
        got_h2, got2 = _run_norm(h, d, w, C.RMS_EPS[0], T)
        assert np.array_equal(got_h2, got_h) and np.array_equal(got2, got)
        out = ops.add_rmsnorm(dev(hn, T), None, dev(w, T), C.RMS_EPS[0])       # no delta, no out: the same bits
        assert np.array_equal(host(out), got)


@pytest.mark.parametrize("T", TYPES)
def test_rmsnorm_special_rows(T):
    """an all-zero row (+-0 out by IEEE's sign rules), a row with one inf, a row with one NaN, a row whose mean square is of eps's size"""
    h, w = C.rms_special_rows(T)
    for eps in C.RMS_EPS:
        hn, lo, hi, _ = C.rmsnorm_ref(h, None, w, eps, T)
        got_h, got = _run_norm(h, None, w, eps, T)
        C.expect_equal(got_h, h, T, "h", exact=True)
        C.check_rmsnorm(got, lo, hi, T, f"add_rmsnorm special rows eps={eps}")
        C.expect_equal(got[:3], lo[:3], T, "zero / inf / NaN rows")


# ---- token_prologue ------------------------------------------------------------------------------------------------------------------------------------------
def _check_prologue(T, embed, ct, st, L, hd, tok, pos, tables=True, mask=True, single=False):
    from hqq_amd import ops
    B, H = len(tok), embed.shape[1]
    want_h, want_c, want_s, want_m = C.prologue_ref(tok, pos, embed, ct if tables else None, st if tables else None, L, T)
    h = Out((B, H), T, salt=29)
    co, so, mo = Out((B, hd), T, salt=31), Out((B, hd), T, salt=37), Out((B, L), T, salt=41)
    tk, ps = torch.tensor(tok, dtype=torch.int64, device="cuda"), torch.tensor(pos, dtype=torch.int64, device="cuda")
    args = (dev(embed, T), h.t, dev(ct, T) if tables else None, dev(st, T) if tables else None, co.t if tables else None, so.t if tables else None, mo.t if mask else None)
    if single:
        ops.token_prologue(tk.view(1, 1), ps, args[0], h.t.view(H), args[2], args[3], co.t.view(hd) if tables else None, so.t.view(hd) if tables else None,
                           mo.t.view(L) if mask else None)
    else:
        ops.token_prologue_batched(tk, ps, *args)
    what = f"vocab={embed.shape[0]} H={H} L={L} hd={hd} tok={tok} pos={pos} tables={tables} mask={mask}"
    C.expect_equal(h.get("h"), want_h, T, "h " + what, exact=True)
    C.expect_equal(co.get("cos"), want_c if tables else co.start(), T, "cos " + what, exact=True)
    C.expect_equal(so.get("sin"), want_s if tables else so.start(), T, "sin " + what, exact=True)
    C.expect_equal(mo.get("mask"), want_m if mask else mo.start(), T, "mask " + what, exact=True)
    assert tk.tolist() == list(tok) and ps.tolist() == list(pos)


@pytest.mark.parametrize("vocab,H", C.PROLOGUE_TABLES)
@pytest.mark.parametrize("T", TYPES)
def test_token_prologue_copies_clamps_and_masks_by_the_documented_rule(T, vocab, H):
    """every (token, position) of {0, vocab - 1, -1, vocab, 2^40} x {0, L - 1, L, -3} as one batched launch per (L, hd), h / cos / sin / mask whole: a token or
    position outside its table reads the last (first) row, the mask takes the raw position.  With and without tables / mask; the single-sequence entry; B = 3
    with one row out of range."""
    toks = C.prologue_tokens(vocab)
    for li, L in enumerate(C.PROLOGUE_L):
        for hi, hd in enumerate(C.PROLOGUE_HD):
            embed, ct, st = C.prologue_tables(vocab, H, L, hd, T)
            tok = [t for t in toks for _ in C.prologue_positions(L)]
            pos = [p for _ in toks for p in C.prologue_positions(L)]
            _check_prologue(T, embed, ct, st, L, hd, tok, pos)
            if li == hi:
                _check_prologue(T, embed, ct, st, L, hd, tok, pos, tables=False)
                _check_prologue(T, embed, ct, st, L, hd, tok, pos, mask=False)
                _check_prologue(T, embed, ct, st, L, hd, tok, pos, tables=False, mask=False)
                _check_prologue(T, embed, ct, st, L, hd, [1 % vocab, vocab, 2 % vocab], [L - 1, 0, L], )
            if li == 1 and hi == 1:
                for t, p in zip(tok, pos):
                    _check_prologue(T, embed, ct, st, L, hd, [t], [p], single=True)


# ---- argmax_advance ------------------------------------------------------------------------------------------------------------------------------------------
POS_STARTS = (0, 41, 2 ** 31 - 1, 2 ** 40)


@pytest.mark.parametrize("n", C.ARGMAX_N)
@pytest.mark.parametrize("T", TYPES)
def test_argmax_advance_winner_ties_zeros_and_nans_on_the_stride_and_the_tree(T, n):
    """_glue_cases.argmax_cases: a single maximum, tie pairs and NaN pairs planted on the 1024-thread stride and on the levels of the LDS tree, +-0, all -inf,
    two +inf — every case a row of one batched launch (different winners per row), then row by row through the single-sequence entry; pos + 1 exactly in int64
    from 0, 41, 2^31 - 1 and 2^40; tok / pos each None in turn"""
    from hqq_amd import ops
    cases = C.argmax_cases(n, T)
    want = [w for _, _, w in cases]
    for name, bits, w in cases:
        assert C.argmax_ref(C.widen(bits, T).tolist()) == w, (n, name)
    Cn = len(cases)
    logits = dev(np.stack([b for _, b, _ in cases]), T)
    starts = [POS_STARTS[i % 4] for i in range(Cn)]

    def buffers():
        nt = torch.full((Cn + 2,), -7, dtype=torch.int64, device="cuda")
        tk = torch.full((Cn + 2,), -9, dtype=torch.int64, device="cuda")
        ps = torch.tensor([-11] + starts + [-13], dtype=torch.int64, device="cuda")
        return nt, tk, ps

    for use_tok, use_pos in ((True, True), (False, True), (True, False), (False, False)):
        nt, tk, ps = buffers()
        ops.argmax_advance_batched(logits, nt[1:-1], tk[1:-1] if use_tok else None, ps[1:-1] if use_pos else None)
        names = [c[0] for c in cases]
        got = nt.tolist()
        assert got == [-7] + want + [-7], [(names[i], got[i + 1], want[i]) for i in range(Cn) if got[i + 1] != want[i]]
        assert tk.tolist() == ([-9] + want + [-9] if use_tok else [-9] * (Cn + 2))
        assert ps.tolist() == ([-11] + [s + 1 for s in starts] + [-13] if use_pos else [-11] + starts + [-13])
    nt, tk, ps = buffers()
    for i in range(Cn):
        ops.argmax_advance(logits[i], nt[1 + i:2 + i].view(1, 1), tk[1 + i:2 + i].view(1, 1), ps[1 + i:2 + i])
    assert nt.tolist() == [-7] + want + [-7] and tk.tolist() == [-9] + want + [-9] and ps.tolist() == [-11] + [s + 1 for s in starts] + [-13]
    assert np.array_equal(host(logits), np.stack([b for _, b, _ in cases]))
