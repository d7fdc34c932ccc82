"""Host half of the glue kernels' tests: proves what tests/test_glue_gpu.py relies on, without a GPU — the rounding helpers and the add / mul restatements of
tests/_glue_cases.py against torch's CPU ops bit for bit, the share of undecided elements under the derived bands, the fp32-range rule of SiLU against torch's
own fp32 formula, and, rule by rule, that a deliberately wrong restatement fails the very checks and cases the GPU test uses."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _glue_cases as C   # noqa: E402

DT = {C.F16: torch.float16, C.BF16: torch.bfloat16}
TYPES = list(C.TYPES)


def _tensor(bits, T):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint16).view(np.int16).copy()).view(DT[T])


def _bits(t):
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def _torch_round(x64, T):
    return _bits(torch.from_numpy(np.ascontiguousarray(x64, dtype=np.float64)).to(DT[T]))


@pytest.mark.parametrize("T", TYPES)
def test_rounding_helpers_on_every_pattern_every_midpoint_and_either_side_of_it(T):
    """round_f16 / round_bf16 against torch's float64 -> T conversion on every 16-bit pattern widened and on every midpoint between neighbours (the one
    between the largest finite value and 2^(emax + 1) included), both signs.  One float64 ulp either side of a midpoint torch's conversion is NOT the
    reference: it converts through fp32, which rounds such a value onto the midpoint first and then to even (double rounding; 1 + 2^-11 + 2^-52 gives
    fp16 1.0).  There the helper is held to the correctly rounded answer — the neighbour on that side — which is what the bands of _glue_cases.py need, and
    to torch one FP32 ulp either side of the midpoint, where torch's path rounds once."""
    rnd = C.round_f16 if T == C.F16 else C.round_bf16
    pat = C.all_patterns()
    x = C.widen(pat, T)
    got = rnd(x)
    assert np.array_equal(got[~C.is_nan(pat, T)], pat[~C.is_nan(pat, T)])
    assert C.is_nan(got[C.is_nan(pat, T)], T).all()
    assert C.same(got, _torch_round(x, T), T).all()
    inf = int(C.bits_of([np.inf], T)[0])
    mag = np.arange(inf, dtype=np.uint16)                       # every finite magnitude and its upper neighbour
    lo = C.widen(mag, T)
    hi = C.widen(mag + 1, T)
    hi[-1] = 2.0 * 2.0 ** np.floor(np.log2(lo[-1]))             # beyond the largest finite value: 2^(emax + 1)
    mid = (lo + hi) / 2                                         # exact in float64
    up = mag + 1
    for sign, sbit in ((1.0, 0), (-1.0, 0x8000)):
        assert np.array_equal(rnd(sign * mid), np.where(mag % 2 == 0, mag, up) | sbit)          # ties to even; the last: overflow to inf
        assert np.array_equal(rnd(sign * mid), _torch_round(sign * mid, T))
        assert np.array_equal(rnd(sign * np.nextafter(mid, 0.0)), mag | sbit)
        assert np.array_equal(rnd(sign * np.nextafter(mid, np.inf)), up | sbit)
        m32 = mid.astype(np.float32)
        assert np.array_equal(m32.astype(np.float64), mid)
        for side in (np.float32(0.0), np.float32(np.inf)):
            x32 = np.nextafter(m32, side).astype(np.float64) * sign
            assert np.array_equal(rnd(x32), _torch_round(x32, T))
    assert rnd(np.array([0.0, -0.0]))[1] == 0x8000 and rnd(np.array([0.0, -0.0]))[0] == 0
    assert np.array_equal(rnd(np.array([1e-300, -1e-300, 1e300, -1e300])), np.array([0, 0x8000, inf, inf | 0x8000], dtype=np.uint16))


@pytest.mark.parametrize("kind", ["add", "mul"])
@pytest.mark.parametrize("T", TYPES)
def test_add_and_mul_restatements_equal_torch_cpu_on_the_sweep_operands(T, kind):
    """one float64 operation + one rounding to T = torch's CPU op on T tensors, on the operands the GPU sweeps use (every pattern against each partner,
    65,536 random pairs): the double-rounding argument of _glue_cases.py's header, observed"""
    a, b = C.sweep_operands(T, kind)
    ta, tb = _tensor(a, T), _tensor(b, T)
    want = _bits(ta + tb if kind == "add" else ta * tb)
    got = C.add(a, b, T) if kind == "add" else C.mul(a, b, T)
    bad = np.flatnonzero(~C.same(got, want, T))
    assert bad.size == 0, (bad.size, hex(a[bad[0]]), hex(b[bad[0]]), hex(got[bad[0]]), hex(want[bad[0]]))


@pytest.mark.parametrize("T", TYPES)
def test_silu_band_leaves_at_most_half_a_percent_of_the_gates_undecided(T):
    pat = C.all_patterns()
    fin = pat[C.is_finite(pat, T)]
    lo, hi = C.silu_bounds(fin, T)
    undecided = int(np.count_nonzero(lo != hi))
    print(f"silu {T}: band {C.SILU_BAND_ULPS:.3f} ulp32, {undecided} of {fin.size} finite gate patterns undecided ({100.0 * undecided / fin.size:.2f} %)")
    assert undecided <= 0.005 * fin.size
    assert (np.abs(C.order_key(lo) - C.order_key(hi)) <= 1).all()          # the two allowed values are neighbours
    assert C.check_silu_gate(C.rnd(C.silu64(pat, T), T), pat, T) == undecided   # the reference passes its own check, non-finite gates included


def test_recorded_ulp_figures_are_those_of_the_tools_kept_output():
    """EXPF_SEEN_ULPS / RSQRTF_SEEN_ULPS are the worst figures of profiles/glue_ulp.txt (tools/glue_ulp.hip's output), no device ever saw expf fail to
    overflow where the formula's fp32 range says it does, and the bands follow from them by the stated rules"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "glue_ulp.txt")).read()
    expf = [ln for ln in text.splitlines() if ln.startswith("EXPF")]
    rsq = [ln for ln in text.splitlines() if ln.startswith("RSQRTF")]
    assert len(expf) == 2 and len(rsq) == 1
    assert C.EXPF_SEEN_ULPS == max(float(x) for ln in expf for x in re.findall(r"worst=([0-9.]+)", ln))
    assert C.RSQRTF_SEEN_ULPS == max(float(x) for x in re.findall(r"worst=([0-9.]+)", rsq[0]))
    assert all(ln.rstrip().endswith("not +inf=0") for ln in expf)
    assert int(re.search(r"case arguments n=(\d+)", rsq[0]).group(1)) == C.rms_arguments().size
    assert C.EXPF_SEEN_ULPS <= C.EXPF_ULPS < C.EXPF_SEEN_ULPS + 0.25 and (4 * C.EXPF_ULPS).is_integer()      # exhaustive sweep: the next 0.25 ulp
    assert C.RSQRTF_ULPS == 2 * C.RSQRTF_SEEN_ULPS                                                             # sampled sweep: twice the seen error
    assert C.SILU_BAND_ULPS == 1.01 * (2 * C.EXPF_ULPS + 1.5)


@pytest.mark.parametrize("T", TYPES)
def test_rmsnorm_interval_decides_at_least_nine_elements_in_ten(T):
    for H in C.RMS_RANDOM_H[T]:
        h, d, w = C.rms_random_case(H, T)
        hn, lo, hi, _ = C.rmsnorm_ref(h, d, w, C.RMS_EPS[0], T)
        for row in range(h.shape[0]):
            share = float(np.mean(C.same(lo[row], hi[row], T)))
            print(f"add_rmsnorm {T} random H={H} row {row}: {100.0 * share:.2f} % decided")
            assert share >= 0.90, (T, H, row, share)
        assert (np.abs(C.order_key(lo) - C.order_key(hi)) <= 2).all()
    for H in C.RMS_EDGE_H:
        for rows in (1, 3):
            for eps in C.RMS_EPS:
                h, d, w = C.rms_edge_case(H, rows, eps, T)
                x = C.widen(C.add(h, d, T) if d is not None else h, T)
                assert set(np.unique(np.abs(x))) <= {0.25, 0.5, 1.0, 2.0, 4.0}
                s32 = np.cumsum((x * x).astype(np.float32), axis=1, dtype=np.float32)      # a sequential fp32 sum is exact here, as any order is
                assert np.array_equal(s32[:, -1].astype(np.float64), (x * x).sum(axis=1))
                hn, lo, hi, _ = C.rmsnorm_ref(h, d, w, eps, T, exact_sum=True)
                share = float(np.mean(C.same(lo, hi, T)))
                print(f"add_rmsnorm {T} edge H={H} rows={rows} eps={eps}: {100.0 * share:.2f} % decided")
                assert share >= 0.90


def test_silu_fp32_range_rule_is_that_of_torchs_fp32_formula():
    """x / (1 + torch.exp(-x)) in fp32 on the CPU, rounded to T: -0 below the fp32 range of exp, NaN at -inf — the reference's rule, not the kernel's"""
    for T, gates in ((C.BF16, [-88.5, -89.0, -100.0, np.inf, -np.inf, np.nan]), (C.F16, [-20.0, -100.0])):
        g = C.bits_of(gates, T)
        x = _tensor(g, T).float()
        want = _bits((x / (1 + torch.exp(-x))).to(DT[T]))
        lo, hi = C.silu_bounds(g, T)
        assert (C.same(want, lo, T) | C.same(want, hi, T)).all(), (T, want, lo, hi)
        ref = C.rnd(C.silu64(g, T), T)
        if T == C.BF16:
            assert C.same(lo, hi, T).all()
            assert ref[1] == 0x8000 and ref[2] == 0x8000 and ref[3] == 0x7F80 and C.is_nan(ref[4:], T).all()
            assert ref[0] != 0x8000 and C.widen(ref[:1], T)[0] < 0          # -88.5 is inside the range: a normal negative number
        else:
            assert ref[0] == 0x8001 and ref[1] == 0x8000                     # -20: the smallest subnormal; -100: -0


# ---- the checks can fail: each deliberately wrong rule is caught by the cases the GPU test runs ---------------------------------------------------------
@pytest.mark.parametrize("T", TYPES)
def test_mutant_silu_as_x_times_rounded_sigmoid_fails(T):
    pat = C.all_patterns()
    one = np.full(65536, C.bits_of([1.0], T)[0], dtype=np.uint16)
    C.check_silu_gate(C.silu_ref(pat, one, T), pat, T)
    with pytest.raises(AssertionError):
        C.check_silu_gate(C.silu_ref(pat, one, T, rule="sigmoid_rounded"), pat, T)


@pytest.mark.parametrize("rule", ["cos_i_both", "flip_rotate_half"])
@pytest.mark.parametrize("T", TYPES)
def test_mutant_rope_fails(T, rule):
    for kind in ("random", "rotary") if rule == "flip_rotate_half" else ("random",):
        c = C.rope_arith_case(kind, T)
        kc, vc = C.rope_caches(c)
        want, bad = C.rope_expect(c, kc, vc, T), C.rope_expect(c, kc, vc, T, rule=rule)
        C.expect_equal(want[0], want[0], T, "q_out")
        with pytest.raises(AssertionError):
            C.expect_equal(bad[0], want[0], T, "q_out")
        with pytest.raises(AssertionError):
            C.expect_equal(bad[1], want[1], T, "k_cache")
    c = C.rope_geometry_case(3, 1, 6, 16, [0, 15, 16], T)
    kc, vc = C.rope_caches(c)
    with pytest.raises(AssertionError):
        C.expect_equal(C.rope_expect(c, kc, vc, T, rule=rule)[0], C.rope_expect(c, kc, vc, T)[0], T, "q_out")


@pytest.mark.parametrize("T", TYPES)
def test_mutant_rmsnorm_fails(T):
    """dividing by H - 1: caught by the dispatch-edge cases (H = 8) and the random rows; eps dropped: caught by the special rows (the all-zero row turns NaN,
    the row whose mean square is of eps's size moves)"""
    h, d, w = C.rms_edge_case(8, 3, C.RMS_EPS[0], T)
    _, lo, hi, _ = C.rmsnorm_ref(h, d, w, C.RMS_EPS[0], T, exact_sum=True)
    C.check_rmsnorm(lo, lo, hi, T)
    with pytest.raises(AssertionError):
        C.check_rmsnorm(C.rmsnorm_ref(h, d, w, C.RMS_EPS[0], T, exact_sum=True, rule="div_h_minus_1")[1], lo, hi, T)
    H = C.RMS_RANDOM_H[T][1]
    h, d, w = C.rms_random_case(H, T)
    _, lo, hi, _ = C.rmsnorm_ref(h, d, w, C.RMS_EPS[0], T)
    with pytest.raises(AssertionError):
        C.check_rmsnorm(C.rmsnorm_ref(h, d, w, C.RMS_EPS[0], T, rule="div_h_minus_1")[1], lo, hi, T)
    h, w = C.rms_special_rows(T)
    _, lo, hi, _ = C.rmsnorm_ref(h, None, w, C.RMS_EPS[0], T)
    C.check_rmsnorm(hi, lo, hi, T)
    mutant = C.rmsnorm_ref(h, None, w, C.RMS_EPS[0], T, rule="no_eps")[1]
    for row in (0, 3):
        with pytest.raises(AssertionError):
            C.check_rmsnorm(mutant[row], lo[row], hi[row], T)
    assert not C.is_nan(lo[0], T).any() and (C.widen(lo[0], T) == 0).all()
    assert C.is_nan(lo[2], T).all() and C.is_nan(lo[1], T).sum() == 1


@pytest.mark.parametrize("T", TYPES)
def test_argmax_rule_agrees_with_the_constructed_winner_and_last_index_ties_fail(T):
    caught = 0
    for n in C.ARGMAX_N[:-2] + (4096,):
        for name, bits, want in C.argmax_cases(n, T):
            vals = C.widen(bits, T).tolist()
            assert C.argmax_ref(vals) == want, (n, name)
            if name.startswith("tie") or name in ("zeros", "all-ninf", "two-pinf"):
                if n > 1:
                    assert C.argmax_ref(vals, rule="last_tie") != want, (n, name)
                    caught += 1
    assert caught > 40


@pytest.mark.parametrize("T", TYPES)
def test_mutant_mask_below_pos_fails(T):
    embed, ct, st = C.prologue_tables(64, 2056, 96, 48, T)
    tok, pos = C.prologue_tokens(64)[:4], C.prologue_positions(96)
    want = C.prologue_ref(tok, pos, embed, ct, st, 96, T)
    bad = C.prologue_ref(tok, pos, embed, ct, st, 96, T, rule="mask_lt")
    C.expect_equal(bad[0], want[0], T, "h", exact=True)
    with pytest.raises(AssertionError):
        C.expect_equal(bad[3], want[3], T, "mask", exact=True)
    # the documented rule itself: out-of-range rows read the last / first row, the mask takes the raw position
    assert np.array_equal(want[0][2], embed[0]) and np.array_equal(want[0][3], embed[63]) and np.array_equal(want[1][2], ct[95]) and np.array_equal(want[1][3], ct[0])
    assert (want[3][2] == 0).all() and (want[3][3] != 0).all() and np.count_nonzero(want[3][0] == 0) == 1
