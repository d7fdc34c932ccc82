"""GPU half of the router tests: hqq_hip_moe_router (csrc/moe_router.hip, hqq_amd.ops.moe_router) against the closed forms, the float64 reference and the
derived bounds of tests/_router_cases.py, the properties that hold exactly, the caller's buffers with guard bytes around them, and graph capture."""
import pytest

torch = pytest.importorskip("torch")

import _router_cases as C   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ran():
    """cid -> (host data, idx, weights, logits of one kernel call, on the host): each case runs once and is shared; nothing modifies it"""
    from hqq_amd import ops
    cache = {}

    def get(cid):
        if cid not in cache:
            c = C.BY_ID[cid]
            d = C.build(c)
            logits = torch.empty((c.T, c.E), dtype=c.dt, device="cuda")
            idx, w = ops.moe_router(d["x"].cuda(), d["W"].cuda(), c.k, renorm=c.renorm, round_weights=c.round_w, logits=logits)
            assert idx.dtype == torch.int64 and w.dtype == torch.float32 and tuple(idx.shape) == (c.T, c.k) and tuple(w.shape) == (c.T, c.k)
            cache[cid] = (d, idx.cpu(), w.cpu(), logits.cpu())
        return cache[cid]
    return get


def _inside_weight_bound(c, w, logits, idx, tag):
    w64 = C.ref_weights(logits, idx, c.renorm)
    b = C.weight_bound(logits, w64, c.E, c.k, c.renorm, c.dt if c.round_w else None)
    err = (w.double() - w64).abs()
    print(c.id, tag, "weights: max err / bound", float((err / b).max()))
    return bool((err <= b).all())


# ---- 1. closed forms ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.CLOSED])
def test_closed_form_cases_are_bit_exact(ran, cid):
    c = C.BY_ID[cid]
    d, idx, w, logits = ran(cid)
    assert torch.equal(idx, d["idx"])
    assert torch.equal(logits.float(), d["logits"].float())
    if d["w"] is not None:
        assert torch.equal(w, d["w"])
    else:
        assert _inside_weight_bound(c, w, logits, idx, "closed")
    if c.kind in ("tie_all", "top_equal"):   # equal logits: ascending ids
        assert bool((idx[:, 1:] > idx[:, :-1]).all())


# ---- 2. random cases ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", [c.id for c in C.RANDOM])
def test_random_cases_select_the_reference_experts_inside_the_derived_bounds(ran, cid):
    c = C.BY_ID[cid]
    d, idx, w, logits = ran(cid)
    l64 = C.logits64(d["x"], d["W"])
    assert torch.equal(idx, C.ref_select(l64, c.k))                  # every row: all of them are margin-checked (tests/test_moe_router_cpu.py)
    err, b = (logits.double() - l64).abs(), C.logit_bound(d["x"], d["W"], c.dt)
    print(c.id, "logits: max err / bound", float((err / b).max()))
    assert bool((err <= b).all())
    assert _inside_weight_bound(c, w, logits, idx, "random")
    if c.round_w:
        assert torch.equal(w, w.to(c.dt).float())                    # representable in T
    if c.renorm and not c.round_w:
        assert bool(((w.double().sum(-1) - 1.0).abs() <= (c.k + 2) * C.U32).all())


@pytest.mark.parametrize("cid", [c.id for c in C.RANDOM])
def test_logits_are_the_restatements_bits(ran, cid):
    """the stated summation order (a function of H alone), restated on the host in fp32 with exact products: the same bits, and then the same selection"""
    c = C.BY_ID[cid]
    d, idx, w, logits = ran(cid)
    idx32, w32, l32 = C.model32(d["x"], d["W"], c.k, c.renorm, c.round_w)
    assert torch.equal(logits.float(), l32.float())
    assert torch.equal(idx, idx32)


# ---- 3. what holds exactly ---------------------------------------------------------------------------------------------------------------------------------------
WIDE = [c.id for c in C.RANDOM if c.T == 16]


@pytest.mark.parametrize("cid", WIDE)
def test_two_calls_give_the_same_bits_and_a_row_does_not_depend_on_the_others(ran, cid):
    from hqq_amd import ops
    c = C.BY_ID[cid]
    d, idx, w, logits = ran(cid)
    x, W = d["x"].cuda(), d["W"].cuda()
    l2 = torch.empty((c.T, c.E), dtype=c.dt, device="cuda")
    idx2, w2 = ops.moe_router(x, W, c.k, renorm=c.renorm, round_weights=c.round_w, logits=l2)
    assert torch.equal(idx2.cpu(), idx) and torch.equal(w2.cpu().view(torch.int32), w.view(torch.int32)) and torch.equal(l2.cpu().view(torch.int16), logits.view(torch.int16))
    for t in (0, 7, 15):
        l1 = torch.empty((1, c.E), dtype=c.dt, device="cuda")
        i1, w1 = ops.moe_router(x[t:t + 1], W, c.k, renorm=c.renorm, round_weights=c.round_w, logits=l1)
        assert torch.equal(i1.cpu(), idx[t:t + 1]) and torch.equal(w1.cpu().view(torch.int32), w[t:t + 1].view(torch.int32))
        assert torch.equal(l1.cpu().view(torch.int16), logits[t:t + 1].view(torch.int16))
    i3, w3 = ops.moe_router(x[3:6], W, c.k, renorm=c.renorm, round_weights=c.round_w)   # without logits: the same routing
    assert torch.equal(i3.cpu(), idx[3:6]) and torch.equal(w3.cpu().view(torch.int32), w[3:6].view(torch.int32))


@pytest.mark.parametrize("cid", [next(c.id for c in C.RANDOM if c.E == 60 and c.k == 2), next(c.id for c in C.RANDOM if c.E == 256 and c.k == 8 and c.T == 16),
                                 next(c.id for c in C.RANDOM if c.E == 1)])
def test_callers_buffers_are_used_and_nothing_around_them_is_written(ran, cid):
    from hqq_amd import ops
    c = C.BY_ID[cid]
    d, idx, w, logits = ran(cid)
    G = 64   # guard elements either side
    bi = torch.full((c.T * c.k + 2 * G,), -7, dtype=torch.int64, device="cuda")
    bw = torch.full((c.T * c.k + 2 * G,), -7.0, dtype=torch.float32, device="cuda")
    bl = torch.full((c.T * c.E + 2 * G,), -7.0, dtype=c.dt, device="cuda")
    vi, vw, vl = bi[G:G + c.T * c.k].view(c.T, c.k), bw[G:G + c.T * c.k].view(c.T, c.k), bl[G:G + c.T * c.E].view(c.T, c.E)
    ri, rw = ops.moe_router(d["x"].cuda(), d["W"].cuda(), c.k, renorm=c.renorm, round_weights=c.round_w, idx=vi, weights=vw, logits=vl)
    assert ri.data_ptr() == vi.data_ptr() and rw.data_ptr() == vw.data_ptr()
    assert torch.equal(vi.cpu(), idx) and torch.equal(vw.cpu().view(torch.int32), w.view(torch.int32)) and torch.equal(vl.cpu().view(torch.int16), logits.view(torch.int16))
    for buf in (bi, bw, bl):
        assert bool((buf[:G] == -7).all()) and bool((buf[-G:] == -7).all())


def test_wrapper_checks_its_arguments():
    from hqq_amd import ops
    x, W = torch.zeros(2, 64, dtype=torch.float16, device="cuda"), torch.zeros(8, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        ops.moe_router(x, W[:, :32], 2)
    with pytest.raises(ValueError):
        ops.moe_router(x.t().contiguous().t(), W, 2)
    with pytest.raises(TypeError):
        ops.moe_router(x, W.bfloat16(), 2)
    with pytest.raises(ValueError):
        ops.moe_router(x, W, 2, idx=torch.zeros(2, 2, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        ops.moe_router(x, W, 2, weights=torch.zeros(2, 3, device="cuda"))
    with pytest.raises(ValueError):
        ops.moe_router(x, W, 2, logits=torch.zeros(2, 8, device="cuda"))
    with pytest.raises(NotImplementedError, match="not covered"):
        ops.moe_router(x, W, 9)
    with pytest.raises(NotImplementedError, match="not covered"):
        ops.moe_router(x.float(), W.float(), 2)
    idx, w = ops.moe_router(x, W, 2)   # all logits equal: the tie rule, and 1/2 exactly
    assert idx.tolist() == [[0, 1], [0, 1]] and w.tolist() == [[0.5, 0.5], [0.5, 0.5]]


# ---- 4. graph capture --------------------------------------------------------------------------------------------------------------------------------------------
def test_router_is_captured_and_replayed_on_other_rows_with_another_routing(ran):
    from hqq_amd import ops
    cid = next(c.id for c in C.RANDOM if c.E == 128 and c.k == 8 and c.T >= 3)
    c = C.BY_ID[cid]
    d, idx, w, logits = ran(cid)
    W = d["W"].cuda()
    x1, x2 = d["x"][:2].cuda().contiguous(), d["x"][1:3].cuda().contiguous()
    assert not torch.equal(idx[:2], idx[1:3])
    x = x1.clone()
    bi, bw = torch.zeros(2, c.k, dtype=torch.int64, device="cuda"), torch.zeros(2, c.k, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.moe_router(x, W, c.k, renorm=c.renorm, round_weights=c.round_w, idx=bi, weights=bw)   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.moe_router(x, W, c.k, renorm=c.renorm, round_weights=c.round_w, idx=bi, weights=bw)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bi.cpu(), idx[:2]) and torch.equal(bw.cpu().view(torch.int32), w[:2].view(torch.int32))
    x.copy_(x2)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bi.cpu(), idx[1:3]) and torch.equal(bw.cpu().view(torch.int32), w[1:3].view(torch.int32))
