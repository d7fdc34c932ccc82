"""The grouped-query decode attention on a GPU (csrc/attn_gqa.hip; ops.attn_decode_gqa*): the closed-form and random cases of tests/_gqa_cases.py against fp64
attention, the identity with the tile kernel on the transposed problem (which pins the shared body, and is why the tile band applies), the kernel's own contract
(determinism, head and sequence independence, nothing read beyond a sequence's position, nothing written by padding rows, argument errors before any launch) and
the quantised entry against the dense one on the dequantised cache."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _gqa_cases as gc  # noqa: E402
import _tile_cases as tc  # noqa: E402
from _attn_cases import bits  # noqa: E402

SENTINEL = 12345.0


def _kernel(t, S=None):
    from hqq_amd import ops
    case = t["case"]
    out = torch.full((len(case.pos), case.heads[0] * case.hd), float("nan"), dtype=gc.DT[case.dt], device="cuda")
    return ops.attn_decode_gqa_batched(t["q"], t["K"], t["V"], t["pos"], out, case.hd ** -0.5, splits=case.S if S is None else S)


# ---- against fp64 -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", gc.DTS)
def test_closed_forms(dt):
    """needle, twin, flat and ident (the one form that tells the heads of a group apart), every head size and head shape, ragged batches, every split count"""
    for hd in gc.HDS:
        cases = gc.closed_cases(dt, hd)
        bad = gc.run(cases, "cuda", _kernel)
        assert not bad, gc.summary(bad, f"{dt} hd {hd}, {len(cases)} launches")


def test_random_cases_stay_inside_the_band():
    cases = gc.random_cases()
    bad = gc.run(cases, "cuda", _kernel)
    assert not bad, gc.summary(bad, f"{len(cases)} launches")


# ---- the shared body ------------------------------------------------------------------------------------------------------------------------------------------
def test_one_sequence_is_the_tile_kernel_on_the_transposed_problem():
    """for G in (2, 4, 7, 16): ops.attn_decode_gqa on one sequence == ops.attn_decode_tiled with rows = G, n_heads = n_kv_heads = n_kv, every position equal, the
    same splits: bit for bit"""
    shapes = [h for h in gc.HEADS if h[0] != h[1]]
    assert sorted(h[0] // h[1] for h in shapes) == [2, 4, 7, 16]
    for heads in shapes:
        _transposed(heads)


def _transposed(heads):
    from hqq_amd import ops
    n_kv, G = heads[1], heads[0] // heads[1]
    ran = 0
    for dt in gc.DTS:
        for hd in gc.HDS:
            for p, S in ((0, 1), (31, 2), (257, 1), (1023, 3), (2047, 7), (1500, 16)):
                case = gc.Case("random", dt, hd, gc.L_BIG, heads, (p,), S, seed=40 + ran)
                t = gc.build(case, "cuda")
                got = torch.empty(heads[0] * hd, dtype=gc.DT[dt], device="cuda")
                ops.attn_decode_gqa(t["q"][0].view(heads[0], hd), t["K"][0], t["V"][0], t["pos"], got, hd ** -0.5, splits=S)
                v = gc.tile_view(t, 0)
                want = torch.empty(G, n_kv * hd, dtype=gc.DT[dt], device="cuda")
                ops.attn_decode_tiled(v["q"], v["K"], v["V"], v["pos"], want, hd ** -0.5, splits=S)
                assert torch.equal(bits(got.view(n_kv, G, hd)), bits(gc.to_heads(want.view(G, n_kv, hd)).view(n_kv, G, hd))), case.id
                assert torch.equal(bits(got), bits(_kernel(t)[0])), case.id          # the one-sequence wrapper is the batched call
                ran += 1
    assert ran == 36


# ---- the kernel's own contract --------------------------------------------------------------------------------------------------------------------------------
CONTRACT = [c for c in gc.random_cases() if len(c.pos) == 3 and c.G > 1 and c.hd != 256][:10] + [c for c in gc.random_cases() if len(c.pos) == 3 and c.hd == 256][:2]


def test_two_calls_give_the_same_bits():
    assert len(CONTRACT) >= 10 and any(c.S > 1 for c in CONTRACT) and any(c.S == 1 for c in CONTRACT)
    for case in CONTRACT:
        t = gc.build(case, "cuda")
        assert torch.equal(bits(_kernel(t)), bits(_kernel(t))), case.id


def test_a_head_depends_on_no_other_heads_or_sequences_input():
    """another head's query replaced: only that head changes.  Another sequence's query, cache and position replaced: only that sequence changes."""
    for case in CONTRACT:
        t = gc.build(case, "cuda")
        B, (n_heads, _), hd = len(case.pos), case.heads, case.hd
        base = _kernel(t).view(B, n_heads, hd).clone()
        for b, h in ((0, 0), (1, n_heads - 1), (2, n_heads // 2)):
            u = dict(t)
            u["q"] = t["q"].clone()
            u["q"].view(B, n_heads, hd)[b, h] = torch.randn(hd, device="cuda").to(u["q"].dtype)
            got = _kernel(u).view(B, n_heads, hd)
            same = torch.ones(B, n_heads, dtype=torch.bool, device="cuda")
            same[b, h] = False
            assert torch.equal(bits(got[same]), bits(base[same])), (case.id, b, h)
            if case.pos[b] > 0:   # (a single visible key weighs 1 whatever the query)
                assert not torch.equal(bits(got[b, h]), bits(base[b, h])), (case.id, b, h)
        u = dict(t)
        u["q"], u["K"], u["V"], u["pos"] = t["q"].clone(), t["K"].clone(), t["V"].clone(), t["pos"].clone()
        u["q"][1] = torch.randn_like(u["q"][1])
        u["K"][1] = torch.randn_like(u["K"][1])
        u["V"][1] = torch.randn_like(u["V"][1])
        u["pos"][1] = (case.pos[1] + 77) % case.L
        got = _kernel(u).view(B, n_heads, hd)
        assert torch.equal(bits(got[0]), bits(base[0])) and torch.equal(bits(got[2]), bits(base[2])), case.id
        assert not torch.equal(bits(got[1]), bits(base[1])), case.id


def test_garbage_beyond_a_sequences_position_changes_no_bit():
    """every cache row beyond pos[b] of each sequence filled with NaN, with +inf, with zeros: the same bits"""
    ran = 0
    for case in gc.random_cases():
        if all(p == case.L - 1 for p in case.pos) or case.seed % 2:
            continue
        outs = [_kernel(gc.build(case, "cuda", fill=f)) for f in (float("nan"), float("inf"), 0.0)]
        assert bool(torch.isfinite(outs[2]).all()), case.id
        assert torch.equal(bits(outs[0]), bits(outs[2])) and torch.equal(bits(outs[1]), bits(outs[2])), case.id
        ran += 1
    assert ran >= 25


def test_padding_rows_write_nothing():
    """at S = 1 and S = 3: out and the workspace inside guard bands that must come back intact; q ends where its allocation ends (a padding row that read query
    memory would read beyond it)"""
    from hqq_amd import _C, ops
    lib = _C.lib()
    for S, heads in ((S, heads) for S in (1, 3) for heads in ((4, 2), (7, 1), (8, 2))):
        case = gc.Case("random", "f16", 128, gc.L_BIG, heads, (1200, 3, 640), S, seed=60 + heads[0])
        t = gc.build(case, "cuda")
        B, n = 3, heads[0] * 128
        qbig = torch.randn(B + 2, n, device="cuda").half()
        q = qbig[2:]
        q.copy_(t["q"])
        assert q.data_ptr() + q.numel() * 2 == qbig.data_ptr() + qbig.numel() * 2
        big = torch.full((B + 4, n), SENTINEL, dtype=torch.float16, device="cuda")
        out = big[2:2 + B]
        need = int(lib.hqq_hip_attn_decode_workspace_bytes(B * heads[0], 128, S))
        guard = 4096
        wsbig = torch.full((need + 2 * guard,), 0x5A, dtype=torch.uint8, device="cuda")
        ws = wsbig[guard:guard + need] if need else None
        ops.attn_decode_gqa_batched(q, t["K"], t["V"], t["pos"], out, 128 ** -0.5, splits=S, workspace=ws)
        assert bool((big[:2] == SENTINEL).all()) and bool((big[2 + B:] == SENTINEL).all()), heads
        assert bool((wsbig[:guard] == 0x5A).all()) and bool((wsbig[guard + need:] == 0x5A).all()), heads
        assert torch.equal(bits(out), bits(_kernel(t))), heads


def test_positions_outside_the_cache_attend_at_the_last_slot():
    from hqq_amd import ops
    case = gc.Case("random", "bf16", 64, 96, (8, 2), (40, 95, 3), 1, seed=77)
    t = gc.build(case, "cuda")
    want = _kernel(t)
    for wild in (96, -1, 1 << 40):
        pos = torch.tensor([40, wild, 3], dtype=torch.int64, device="cuda")
        for S in (1, 2):
            got = ops.attn_decode_gqa_batched(t["q"], t["K"], t["V"], pos, torch.empty_like(want), 0.125, splits=S)
            assert torch.equal(bits(got), bits(_kernel(t, S))), (wild, S)


# ---- the quantised cache ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_quantised_entry_has_the_dense_entrys_bits_on_the_dequantised_cache():
    """q8 and q4, gs 32 and 64 where kv_covers allows, both dtypes, every head size, S in (1, 3), a ragged batch of 3; the buffers beyond each position hold garbage levels
    and NaN meta, which nothing reads"""
    for nbits in (8, 4):
        assert _quantised_sweep(nbits) >= 20, nbits


def _quantised_sweep(nbits):
    from hqq_amd import ops
    ran = 0
    for dt in gc.DTS:
        T = gc.DT[dt]
        for hd in gc.HDS:
            for gs in (32, 64):
                if not ops.kv_covers(T, nbits, hd, gs, 512):
                    continue
                for S, heads in ((1, (8, 2)), (3, (7, 1))):
                    B, (n_heads, n_kv), L, pos = 3, heads, 512, (300, 0, 511)
                    g = torch.Generator(device="cuda").manual_seed(1000 * nbits + hd + gs + S)
                    k = torch.randn(B, n_kv, L, hd, device="cuda", generator=g).to(T)
                    v = torch.randn(B, n_kv, L, hd, device="cuda", generator=g).to(T)
                    q = (torch.randn(B, n_heads * hd, device="cuda", generator=g) * (0.25 if hd == 256 else 1.0)).to(T)
                    bufs = ops.kv_alloc(B, n_kv, L, hd, nbits, gs, T, "cuda")
                    ops.kv_quantize(k, v, bufs, 0)
                    kd, vd = ops.kv_dequantize(bufs, hd)
                    p = torch.tensor(pos, dtype=torch.int64, device="cuda")
                    want = ops.attn_decode_gqa_batched(q, kd, vd, p, torch.empty_like(q), hd ** -0.5, splits=S)
                    for b, pb in enumerate(pos):                      # nothing beyond pos[b] is read, in levels or in meta
                        for i, t in enumerate(bufs):
                            t[b, :, pb + 1:] = 0xFF if i in (0, 3) else float("nan")
                    got = ops.attn_decode_gqa_kvq_batched(q, bufs, p, torch.full_like(q, float("nan")), hd ** -0.5, hd, splits=S)
                    assert bool(torch.isfinite(want).all()) and torch.equal(bits(got), bits(want)), (dt, hd, gs, S, heads)
                    one = ops.attn_decode_gqa_kvq(q[1], tuple(t[1] for t in bufs), p[1:2], torch.empty_like(q[1]), hd ** -0.5, hd, splits=S)
                    assert torch.equal(bits(one), bits(want[1])), (dt, hd, gs, S, heads)
                    ran += 1
    return ran


# ---- argument errors ----------------------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_come_before_any_launch():
    from hqq_amd import _C, ops
    lib = _C.lib()
    case = gc.Case("random", "f16", 64, 256, (8, 2), (100, 7, 255), 2, seed=3)
    t = gc.build(case, "cuda")
    out = torch.full((3, 8 * 64), 777.0, dtype=torch.float16, device="cuda")
    need = int(lib.hqq_hip_attn_decode_workspace_bytes(3 * 8, 64, 2))
    assert need == 3 * 8 * 2 * 66 * 4
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    ok = dict(ws_ptr=ws.data_ptr(), ws_bytes=need)
    assert gc.call(lib, t, out, ws_ptr=ws.data_ptr(), ws_bytes=need - 1) == -2          # an undersized workspace
    assert gc.call(lib, t, out, ws_ptr=0, ws_bytes=need) == -2                          # a missing one
    assert gc.call(lib, t, out, q_ptr=0, **ok) == -2                                    # a null pointer
    assert gc.call(lib, t, out, q_ptr=t["q"].data_ptr() + 2, **ok) == -6                # misalignment
    assert gc.call(lib, t, out, k_ptr=t["K"].data_ptr() + 8, **ok) == -6
    assert gc.call(lib, t, out, hd=96, **ok) == -4                                      # head_dim 96
    assert gc.call(lib, t, out, heads=(64, 2), **ok) == -4                              # G = 32
    assert b"G = n_heads / n_kv_heads = 32" in lib.hqq_hip_last_error()
    assert gc.call(lib, t, out, heads=(7, 2), **ok) == -2                               # n_heads no multiple of n_kv_heads
    assert gc.call(lib, t, out, S=65, **ok) == -2
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())                                                   # nothing was launched
    assert gc.call(lib, t, out, **ok) == 0
    assert torch.equal(bits(out), bits(_kernel(t)))
    # the quantised entry: G first, then the cache's coverage rule, then the shared checks
    bufs = ops.kv_alloc(3, 2, 256, 64, 8, 32, torch.float16, "cuda")
    st = torch.cuda.current_stream().cuda_stream

    def kvq(nbits=8, n_heads=8, hd=64, gs=32, q_ptr=None):
        return lib.hqq_hip_attn_decode_gqa_kvq_batched(nbits, t["q"].data_ptr() if q_ptr is None else q_ptr, *(b.data_ptr() for b in bufs), t["pos"].data_ptr(), 3,
                                                       out.data_ptr(), n_heads, 2, hd, gs, 256, 0.125, gc.CODE["f16"], 1, 0, 0, st)
    out.fill_(777.0)
    assert kvq(n_heads=64) == -4 and b"= 32" in lib.hqq_hip_last_error()
    assert kvq(nbits=3) == -4 and kvq(hd=96) == -4 and kvq(gs=48) == -4
    assert kvq(q_ptr=0) == -2 and kvq(q_ptr=t["q"].data_ptr() + 2) == -6
    torch.cuda.synchronize()
    assert bool((out == 777.0).all())
    assert kvq() == 0
    with pytest.raises(NotImplementedError):
        ops.attn_decode_gqa_batched(torch.zeros(1, 64 * 64, dtype=torch.float16, device="cuda"), t["K"][:1], t["V"][:1], t["pos"][:1],
                                    torch.zeros(1, 64 * 64, dtype=torch.float16, device="cuda"), 0.125)
