"""No GPU: the cases of tests/_tile_cases.py are what they claim to be — every closed form is what fp64 attention gives on the same tensors, the needles win
by more than 100, a host emulation of the kernel's stated arithmetic stays inside the derived band in two block orders, and the band is less than twice the
rounding of P and of the output on every random case — and check_speculation knows the verify_attention keyword."""
import pytest
import torch

import _tile_cases as tc


@pytest.mark.parametrize("dt", tc.DTS)
@pytest.mark.parametrize("hd", tc.HDS)
def test_closed_forms_are_what_fp64_attention_gives(dt, hd):
    cases = tc.closed_cases(dt, hd) + tc.sweep_cases(dt, hd)
    kinds = {c.kind for c in cases}
    assert kinds == {"tier", "needle", "twin", "flat"} and len(cases) > tc.sweep_max_n(hd) + 60
    bad = tc.run(cases, "cpu")
    assert not bad, tc.summary(bad, f"{dt} hd {hd}")


@pytest.mark.parametrize("dt", tc.DTS)
@pytest.mark.parametrize("hd", tc.HDS)
def test_needle_margins(dt, hd):
    """the 32-needle over every background key, and the 64-needle over the 32-needle, by more than 100: the losing keys' probabilities are below e^-100"""
    for case in (tc.tier_cases(dt, hd)[0], tc.sweep_cases(dt, hd)[-1], tc.twin_cases(dt, hd)[0], tc.split_cases(dt, hd, 7)[0]):
        lo, hi = tc.margins(tc.build(case, "cpu"))
        assert lo > 100 and hi > 100, (case.id, lo, hi)


def test_the_sweep_covers_what_it_names():
    for hd in tc.HDS:
        KB = tc.kb(hd)
        cases = tc.sweep_cases("f16", hd)
        assert [c.n_max for c in cases] == list(range(1, 2 * KB + 34))
        last_block = first_block = some_rows = False
        for c in cases:
            for a in c.a:
                last_block |= c.n_max > KB and a // 32 == (c.n_max - 1) // 32
                first_block |= c.n_max > KB and a < 32
                some_rows |= min(c.pos) < a <= max(c.pos)
        assert last_block and first_block and some_rows
    for S in tc.SPLITS:
        cs = tc.split_cases("f16", 64, S)
        assert any(c.n_max < S for c in cs)
        full = [c for c in cs if c.n_max == 2048]
        edges = {p for k0, k1 in tc.shares(2048, S) for p in (k0, k1 - 1)}
        assert edges == {a for c in full for a in c.a}
        assert any(p < tc.shares(2048, S)[-1][0] for p in full[0].pos)     # rows whose later shares are empty


RANDOM = tc.random_cases()


def test_reference_rows_is_the_one_row_reference_row_by_row():
    """the vectorised fp64 reference of this file against _attn_cases.reference, which the one-row kernels' tests use: row i over its own pos[i] + 1 keys"""
    for case in RANDOM[3::11] + [RANDOM[-2]]:
        t = tc.build(case, "cpu")
        scaling = case.hd ** -0.5
        got, _ = tc.reference_rows(t["q"], t["K"], t["V"], t["pos"], scaling)
        for i, p in enumerate(case.pos):
            want, _ = tc.reference(t["q"][i].view(-1, case.hd), t["K"], t["V"], p + 1, scaling)
            torch.testing.assert_close(got[i], want, rtol=1e-12, atol=1e-14)


def test_the_random_grid():
    assert {len(c.pos) for c in RANDOM} >= set(tc.RANDOM_RS) and {c.hd for c in RANDOM} == set(tc.HDS) and {c.heads for c in RANDOM} == set(tc.RANDOM_HEADS)
    for dt in tc.DTS:
        for hd in tc.HDS:
            mine = [c for c in RANDOM if c.dt == dt and c.hd == hd and c.seed < 900]
            assert {c.pos[0] for c in mine} >= {0, 31, 32, 1023} and any(c.pos[-1] == tc.RANDOM_L - 1 for c in mine) and {c.heads for c in mine} == set(tc.RANDOM_HEADS)
    assert any(list(c.pos) != sorted(c.pos) for c in RANDOM) and any(c.S > 1 for c in RANDOM)


@pytest.mark.parametrize("case", RANDOM, ids=lambda c: c.id)
def test_emulation_stays_inside_the_band_and_the_band_is_tight(case):
    t = tc.build(case, "cpu")
    scaling = case.hd ** -0.5
    ref, _ = tc.reference_rows(t["q"], t["K"], t["V"], t["pos"], scaling)
    tol, rest, lead = tc.band(t, ref, scaling)
    assert bool((rest < lead).all()), f"the band condition: rest / lead at most {float((rest / lead).max()):.3f}"
    for order in ("waves", "serial"):
        got = tc.emulate(t, order).view(ref.shape).double()
        err = (got - ref).abs()
        print(f"{order}: largest error / band {float((err / tol).max()):.3f}")
        assert bool((err <= tol).all()), order


def test_check_speculation_knows_the_keyword():
    from hqq_amd.utils.generation import check_speculation
    check_speculation("ngram", 8, 3, False, "rows")
    check_speculation("ngram", 8, 3, False, "tile")
    check_speculation("ngram", 8, 3, False, verify_attention="tile")
    check_speculation(None, 8, 3, False, "rows")
    check_speculation(None, 8, 3, True)
    for bad in ("Tile", "row", "", None, True, 1, "sdpa"):
        with pytest.raises(ValueError, match="verify_attention"):
            check_speculation("ngram", 8, 3, False, bad)
    with pytest.raises(ValueError, match="verify_attention"):
        check_speculation(None, 8, 3, False, "tile")          # as speculate with do_sample: the keyword names a step that will not run
