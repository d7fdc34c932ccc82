"""The prompt's causal attention on a GPU (csrc/attn_prefill.hip; ops.attn_prefill / ops.attn_prefill_kvq) against its contract, on the cases of
tests/_prefill_cases.py (caches of at most 512 positions):
  (a) tile identity   rows 16 j .. of head h == ops.attn_decode_tiled on those queries with pos = pos0 + 16 j + i and splits = 1, bit for bit
  (b) band            every row within _tile_cases.band (c_acc(n_max of its tile, 1)) of float64 attention
  (c) packed == dense ops.attn_prefill_kvq == ops.attn_prefill on ops.kv_dequantize's tensors, bit for bit
  (d) nothing beyond  NaN from pos0 + T on (NaN scales and zeros for the packed cache) gives the bits of zeros there
  (e) causality       queries of rows > i, finite keys / values at positions > pos0 + i: no bit of row i changes
  (f) determinism     the same bits call to call, and for a head-major q read through its strides
and the argument errors, which come back before any launch.
The checks are functions of (dtype, head_dim); three tests walk them over every dtype and head size, so that the suite grows by three entries, not by forty."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _prefill_cases as pc  # noqa: E402

QUANT = [(nbits, gs) for nbits in (8, 4) for gs in (32, 64)]


def _pick(dt, hd, want):
    """the cases of (dt, hd) with (heads, pos0, T) in `want`"""
    out = [c for c in pc.cases(dt, hd) if (c.heads, c.pos0, c.T) in want]
    assert len(out) == len(want)
    return out


# ---- (a) and (b) on the whole bed ------------------------------------------------------------------------------------------------------------------------------
def _every_tile_is_the_tile_kernel_and_every_row_is_in_the_band(dt, hd):
    cases = pc.cases(dt, hd)
    flags, names = [], []
    for case in cases:
        t = pc.build(case, "cuda")
        got = pc.prefill(t)
        ref = pc.reference(t)
        differs = torch.ones(case.T, case.heads[0], dtype=torch.bool, device="cuda")
        for j, pos in pc.tiles(case):
            rows = slice(16 * j, 16 * j + len(pos))
            differs[rows] = (pc.bits(got[rows]) != pc.bits(pc.tiled(t, j, pos))).any(-1)
        flags += [differs.any(), pc.outside_band(t, got, ref).any(), ~torch.isfinite(got).all()]
        names += [f"{case.id}: {what}" for what in ("a tile differs from ops.attn_decode_tiled", "a row is outside the band", "a row is not finite")]
    bad = [names[i] for i in torch.stack(flags).nonzero().view(-1).tolist()]   # (one host read)
    assert not bad, f"{dt} hd {hd}, {len(cases)} prompts: {len(bad)} failures, first: " + "; ".join(bad[:6])


# ---- (c) ---------------------------------------------------------------------------------------------------------------------------------------------------
def _the_packed_entry_has_the_bits_of_the_dense_one_on_the_dequantised_cache(dt, hd):
    from hqq_amd import ops
    ran = 0
    for nbits, gs in QUANT:
        if not ops.kv_covers(pc.DT[dt], nbits, hd, gs, 128):
            continue
        for case in _pick(dt, hd, {((8, 2), 5, 33), ((4, 4), 37, 49), ((8, 2), 0, 273), ((4, 4), 47, 49), ((8, 2), 16, 1)}):
            t = pc.build(case, "cuda")
            bufs = pc.quantised(t, nbits, gs)
            kd, vd = ops.kv_dequantize(bufs, hd)
            want = pc.prefill(t, K=kd, V=vd)
            got = pc.prefill_kvq(t, bufs)
            assert bool(torch.isfinite(got).all()) and torch.equal(pc.bits(got), pc.bits(want)), (case.id, nbits, gs)
            one = pc.prefill_kvq(t, tuple(b[0] for b in bufs))                  # [n_kv, L, .] is accepted
            assert torch.equal(pc.bits(one), pc.bits(want)), (case.id, nbits, gs)
            ran += 1
    assert ran == (15 if hd == 64 else 20)   # (hd 64: q4 at group size 64 is outside ops.kv_covers)


# ---- (d) ---------------------------------------------------------------------------------------------------------------------------------------------------
CONTRACT = {((8, 2), 5, 33), ((4, 4), 37, 17), ((8, 2), 0, 273), ((4, 4), 16, 1)}


def _nothing_at_or_beyond_the_prompts_end_is_read(dt, hd):
    """dense: NaN, +inf and zeros from pos0 + T on give the same bits; packed: NaN scales and zeros over 0xFF levels give the bits of zeroed buffers"""
    from hqq_amd import ops
    for case in _pick(dt, hd, CONTRACT):
        assert case.n < case.L
        outs = [pc.prefill(pc.build(case, "cuda", fill=f)) for f in (float("nan"), float("inf"), 0.0)]
        assert bool(torch.isfinite(outs[2]).all()), case.id
        assert torch.equal(pc.bits(outs[0]), pc.bits(outs[2])) and torch.equal(pc.bits(outs[1]), pc.bits(outs[2])), case.id
        t = pc.build(case, "cuda")
        for nbits, gs in ((8, 32), (4, 32)):
            assert ops.kv_covers(pc.DT[dt], nbits, hd, gs, case.L)
            clean, dirty = pc.quantised(t, nbits, gs), pc.quantised(t, nbits, gs, beyond="nan")
            assert bool(torch.isnan(dirty[1][:, :, case.n:]).all()) and not bool(torch.isnan(dirty[1][:, :, :case.n]).any())
            want, got = pc.prefill_kvq(t, clean), pc.prefill_kvq(t, dirty)
            assert bool(torch.isfinite(want).all()) and torch.equal(pc.bits(got), pc.bits(want)), (case.id, nbits)


# ---- (e) ---------------------------------------------------------------------------------------------------------------------------------------------------
def _causality_is_exact(dt, hd):
    """for rows i in the first tile, at a tile edge and inside a later tile: other queries in the rows > i, and other FINITE keys and values at the positions
    > pos0 + i, change no bit of the rows <= i — and do change the rows behind"""
    ran = 0
    for case in _pick(dt, hd, {((8, 2), 5, 33), ((4, 4), 37, 49), ((8, 2), 0, 273)}):
        t = pc.build(case, "cuda")
        base = pc.prefill(t).clone()
        for i in sorted({0, 7, 15, 16, case.T - 2}):
            q = t["q"].clone()
            q[i + 1:] = torch.randn_like(q[i + 1:]) * case.qscale
            got = pc.prefill(t, q=q)
            assert torch.equal(pc.bits(got[:i + 1]), pc.bits(base[:i + 1])), (case.id, i, "queries")
            assert not torch.equal(pc.bits(got[i + 1:]), pc.bits(base[i + 1:])), (case.id, i, "queries")
            K, V = t["K"].clone(), t["V"].clone()
            hi = case.pos0 + i + 1
            K[:, hi:case.n] = torch.randn_like(K[:, hi:case.n])
            V[:, hi:case.n] = torch.randn_like(V[:, hi:case.n]) * 3
            got = pc.prefill(t, K=K, V=V)
            assert torch.equal(pc.bits(got[:i + 1]), pc.bits(base[:i + 1])), (case.id, i, "keys and values")
            assert not torch.equal(pc.bits(got[i + 1:]), pc.bits(base[i + 1:])), (case.id, i, "keys and values")
            ran += 1
    assert ran >= 13


# ---- (f) ---------------------------------------------------------------------------------------------------------------------------------------------------
def _two_calls_and_two_layouts_give_the_same_bits(dt, hd):
    """the same bits call to call; a head-major q ([1, H, T, hd] as HF's attention modules hold it, handed over as its [T, H, hd] view), a q with padded rows and
    an `out` the wrapper allocates give the bits of the contiguous call"""
    from hqq_amd import ops
    for case in _pick(dt, hd, CONTRACT):
        t = pc.build(case, "cuda")
        base = pc.prefill(t).clone()
        assert torch.equal(pc.bits(pc.prefill(t)), pc.bits(base)), case.id
        T, H = case.T, case.heads[0]
        hf = t["q"].transpose(0, 1).contiguous().view(1, H, T, hd)              # head-major memory
        view = hf[0].transpose(0, 1)
        assert view.shape == t["q"].shape and (T == 1 or not view.is_contiguous()) and view.data_ptr() == hf.data_ptr()
        assert torch.equal(pc.bits(pc.prefill(t, q=view)), pc.bits(base)), case.id
        wide = torch.full((T, H + 1, hd + 8), float("nan"), dtype=pc.DT[dt], device="cuda")   # row stride (H + 1)(hd + 8), head stride hd + 8
        wide[:, :H, :hd] = t["q"]
        assert torch.equal(pc.bits(pc.prefill(t, q=wide[:, :H, :hd])), pc.bits(base)), case.id
        got = ops.attn_prefill(t["q"], t["K"].view(1, *t["K"].shape), t["V"].view(1, *t["V"].shape), case.pos0)   # [1, n_kv, L, hd], the default scaling
        assert got.shape == (T, H, hd) and got.is_contiguous() and torch.equal(pc.bits(got), pc.bits(base)), case.id


def _padding_rows_read_and_write_nothing():
    """q: the last T rows of its allocation; out: T rows inside a larger allocation pre-filled with a sentinel — nothing outside them is written"""
    from hqq_amd import ops
    for T in (1, 17, 31):
        case = pc.Case("f16", 128, 128, (8, 2), 37, T, seed=60 + T)
        t = pc.build(case, "cuda")
        qbig = torch.randn(T + 3, 8, 128, device="cuda").half()
        q = qbig[3:]
        q.copy_(t["q"])
        assert q.data_ptr() + q.numel() * 2 == qbig.data_ptr() + qbig.numel() * 2
        big = torch.full((T + 20, 8, 128), 12345.0, dtype=torch.float16, device="cuda")
        out = big[2:2 + T]
        ops.attn_prefill(q, t["K"], t["V"], 37, out=out, scaling=128 ** -0.5)
        assert bool((big[:2] == 12345.0).all()) and bool((big[2 + T:] == 12345.0).all()), T
        assert torch.equal(pc.bits(out), pc.bits(pc.prefill(t))), T


# ---- argument errors ------------------------------------------------------------------------------------------------------------------------------------------
def _argument_errors_come_before_any_launch():
    from hqq_amd import _C
    from hqq_amd import ops
    lib = _C.lib()
    case = pc.Case("f16", 64, 128, (4, 4), 5, 33, seed=3)
    t = pc.build(case, "cuda")
    out = torch.full((33, 4, 64), 777.0, dtype=torch.float16, device="cuda")
    assert pc.call(lib, t, out, T=0) == -2 and pc.call(lib, t, out, pos0=-1) == -2
    assert pc.call(lib, t, out, pos0=96) == -2 and b"do not fit" in lib.hqq_hip_last_error()      # pos0 + T = 129 > 128: no clamping, an error
    assert pc.call(lib, t, out, L=37) == -2 and pc.call(lib, t, out, T=124) == -2
    assert pc.call(lib, t, out, qrs=4 * 64 + 4) == -6 and pc.call(lib, t, out, qhs=60) == -6
    assert pc.call(lib, t, out, q_ptr=t["q"].data_ptr() + 2) == -6
    assert pc.call(lib, t, out, hd=96) == -4 and pc.call(lib, t, out, n_kv=3) == -2
    bufs = pc.quantised(t, 8, 32)
    assert pc.call_kvq(lib, t, bufs, 8, 32, out, T=0) == -2 and pc.call_kvq(lib, t, bufs, 8, 32, out, pos0=100) == -2
    assert pc.call_kvq(lib, t, bufs, 8, 32, out, qrs=100) == -6
    assert pc.call_kvq(lib, t, bufs, 3, 32, out) == -4 and pc.call_kvq(lib, t, bufs, 4, 64, out) == -4 and pc.call_kvq(lib, t, bufs, 8, 16, out) == -4
    with pytest.raises(ValueError):
        ops.attn_prefill(t["q"], t["K"], t["V"], 96, out=out)
    with pytest.raises(ValueError):
        ops.attn_prefill(t["q"][:0], t["K"], t["V"], 0, out=out[:0])
    with pytest.raises(ValueError):
        ops.attn_prefill_kvq(t["q"], bufs, 96, 64, out=out)
    with pytest.raises(ValueError):
        ops.attn_prefill(t["q"].bfloat16(), t["K"], t["V"], 5, out=out)
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())                                                           # nothing was launched
    assert pc.call(lib, t, out) == 0
    assert torch.equal(pc.bits(out), pc.bits(pc.prefill(t)))
    out.fill_(777.0)
    assert pc.call_kvq(lib, t, bufs, 8, 32, out) == 0
    assert torch.equal(pc.bits(out), pc.bits(pc.prefill_kvq(t, bufs)))


# ---- the tests: every check above at every (dtype, head_dim) --------------------------------------------------------------------------------------------------
GRID = [(dt, hd) for hd in pc.HDS for dt in pc.DTS]


def test_tiles_are_the_tile_kernels_and_rows_are_in_the_band():
    """(a) and (b) on the whole bed of tests/_prefill_cases.py"""
    assert len(GRID) == 6
    for dt, hd in GRID:
        _every_tile_is_the_tile_kernel_and_every_row_is_in_the_band(dt, hd)


def test_packed_equals_dense_and_nothing_beyond_the_prompt_is_read():
    """(c) for q8 / q4 at group sizes 32 / 64 wherever ops.kv_covers holds, and (d) on both entries"""
    for dt, hd in GRID:
        _the_packed_entry_has_the_bits_of_the_dense_one_on_the_dequantised_cache(dt, hd)
        _nothing_at_or_beyond_the_prompts_end_is_read(dt, hd)


def test_causality_determinism_layout_and_argument_errors():
    """(e) and (f), the padding rows of the last tile, and the argument errors with `out` untouched"""
    for dt, hd in GRID:
        _causality_is_exact(dt, hd)
        _two_calls_and_two_layouts_give_the_same_bits(dt, hd)
    _padding_rows_read_and_write_nothing()
    _argument_errors_come_before_any_launch()
