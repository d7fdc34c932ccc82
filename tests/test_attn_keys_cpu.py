"""Host-side half of the key-by-key decode-attention tests (tests/test_attn_keys_gpu.py): every generated case's closed form holds in fp64
softmax attention over the very tensors the GPU file builds (on the CPU here), the grid reaches the residues, share edges and empty shares it
claims, and no case leaves what the entry points accept.  No device and no library needed."""
import pytest
import torch

import _attn_cases as A

DTS = ("f16", "bf16")


def _split(launches):
    return [l for l in launches if l.kind != "flat"], [l for l in launches if l.kind == "flat"]


def _closed_forms_hold(dt, hd, L, launches, mirror=False):
    keyed, flat = _split(launches)
    bad = A.run(A.Bed(dt, hd, L, "cpu", mirror=mirror), keyed)
    if flat:
        bad += A.run(A.Bed(dt, hd, L, "cpu", flat=True), flat)
    assert not bad, A.summary(bad, f"{dt} hd{hd}")
    return len(keyed) + len(flat)


@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_closed_forms_of_the_one_workgroup_sweep(dt, hd):
    assert _closed_forms_hold(dt, hd, A.sweep_max_n(hd), A.sweep_launches(hd)) >= 3 * A.sweep_max_n(hd) - 1


@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_closed_forms_of_the_long_and_split_cases(dt, hd):
    """one bed of the full cache length serves the long one-workgroup cases and every split count, as in the GPU file"""
    launches = A.long_launches(hd) + [l for S in A.SPLITS for l in A.split_launches(hd, S)]
    _closed_forms_hold(dt, hd, A.MAX_L, launches, mirror=True)


@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_the_needle_outscores_every_background_key_by_more_than_100(dt, hd):
    """so a share without the needle merges with e^(m_s - m) = 0 in fp32 (e^-100 < 2^-144, below the smallest subnormal's half), for every
    place and every n of the grid: the margin is taken over all MAX_L background rows; also at the GQA factor 2 of a group's second head"""
    assert A.needle_margin(A.Bed(dt, hd, A.MAX_L, "cpu")) > 100
    assert A.needle_margin(A.Bed(dt, hd, 2048, "cpu", heads=2, rep=8)) > 100


@pytest.mark.parametrize("dt", DTS)
def test_the_reference_leaves_less_than_1e_9_off_the_needle(dt):
    """hd = 64 (the smallest needle score), n = 30000 (the most background keys)"""
    bed = A.Bed(dt, 64, A.MAX_L, "cpu")
    for place in (0, 15000, 29999):
        assert A.off_needle_mass(bed, A.MAX_L, place) < 1e-9


def test_position_coded_values_tell_every_key_and_head_apart():
    v = A.coded_values(3, 300, 64, "cpu")
    assert bool((v != 0).all()) and float(v.abs().max()) <= 127 and bool((v == v.round()).all())
    assert bool((v[:, 1:] != v[:, :-1]).all()) and bool((v[1:] != v[:-1]).all())
    for dt in DTS:
        assert torch.equal(v.to(A.DT[dt]).float(), v)
        f = A.flat_row(8, 64, "cpu")
        assert torch.equal(f.to(A.DT[dt]).float(), f) and bool((torch.log2(f.abs()) % 1 == 0).all())
        assert float((f.abs() / A.FLAT_MAX_N).min()) > 2.0 ** -14            # V[j*] / n: a normal fp16 number


@pytest.mark.parametrize("hd", A.HDS)
def test_the_sweep_reaches_every_residue_and_every_named_place(hd):
    st = A.step(hd)
    assert st == {64: 64, 128: 32, 256: 16}[hd]
    ls = [l for l in A.sweep_launches(hd) if l.kind == "needle"]
    ns = [l.n for l in ls]
    assert ns == list(range(1, 2 * 4 * st + st + 2))
    assert {n % (4 * st) for n in ns} == set(range(4 * st))
    for l in ls:
        n = l.n
        if n > 4 * st + 1:
            m1, m4 = (n - 1) // st * st, (n - 1) // (4 * st) * (4 * st)
            assert set(l.a) >= {0, n - 1, n - 2, n // 2, m1 - 1, m1, m4 - 1, m4}
    for l in A.sweep_launches(hd):
        assert l.kind != "twin" or all(x != y for x, y in zip(l.a, l.b))
    # the last key sits in every wave and every sub-row of a wave
    kpw = 512 // hd
    assert {((n - 1) % st) // kpw for n in ns} == set(range(8)) and {(n - 1) % kpw for n in ns} == set(range(kpw))


@pytest.mark.parametrize("hd", A.HDS)
def test_the_long_cases_are_the_ones_named(hd):
    ls = A.long_launches(hd)
    assert {l.n for l in ls} == {1024, 1025, 2048, 4001, 8191, 20000, 29999, 30000} and all(l.S == 1 for l in ls)
    assert {l.kind for l in ls} == {"needle", "twin"}
    # with the bed's cache length the scores alone pass 48 KiB of LDS
    assert 64 + hd * 6 + 8 * hd * 4 + (A.MAX_L + 8) * 4 > 48 * 1024


@pytest.mark.parametrize("S", A.SPLITS)
@pytest.mark.parametrize("hd", A.HDS)
def test_the_split_grid_probes_both_ends_of_every_share(hd, S):
    ls = A.split_launches(hd, S)
    assert {l.n for l in ls} == {n for n in (1, 2, S - 1, S, S + 1, 37, 1025, 4001, 20000) if n >= 1}
    empty = past_end = False
    for n in {l.n for l in ls}:
        chunk = -(-n // S)
        probed = {p for l in ls if l.n == n and l.kind == "needle" for p in l.a}
        for s in range(S):
            k0, k1 = s * chunk, min(s * chunk + chunk, n)
            if k0 < k1:
                assert k0 in probed and k1 - 1 in probed, (n, s)
            else:
                empty = True
                past_end |= k0 >= n and chunk * (S - 1) >= n
        share_of = lambda p: p // chunk   # noqa: E731
        for l in ls:
            if l.n == n and l.kind == "twin":
                assert all(share_of(x) != share_of(y) for x, y in zip(l.a, l.b)), l.id
        if n >= 2 and -(-n // chunk) >= 2:
            assert any(l.n == n and l.kind == "twin" for l in ls)
        assert any(l.n == n and l.kind == "flat" for l in ls) == (n <= A.FLAT_MAX_N)
    assert empty and past_end


def test_no_case_leaves_what_the_entry_points_accept():
    for hd in A.HDS:
        assert hd in (64, 128, 256)
        every = A.sweep_launches(hd) + A.long_launches(hd) + [l for S in A.SPLITS for l in A.split_launches(hd, S)]
        for l in every:
            assert 1 <= l.n <= A.MAX_L <= 30000 and 1 <= l.S <= A.MAX_SPLITS <= 64
            assert len(l.a) == len(l.b) == A.HEADS and all(0 <= p < l.n for p in l.a + l.b)
            assert l.kind != "flat" or l.n <= A.FLAT_MAX_N
    assert max(A.LONG_NS) == A.MAX_L
