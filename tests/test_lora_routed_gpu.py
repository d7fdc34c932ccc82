"""GPU tests of the routed adapter kernels (hqq_hip_lora_shrink_routed + hqq_hip_lora_expand_routed, csrc/lora_decode.hip) on the cases of
tests/_lora_bank_cases.py.  The reference of every comparison is the EXISTING pair — ops.lora_shrink + ops.lora_expand on one row with one adapter (and on all
rows where the slots are uniform) — and every comparison is torch.equal on the raw bits: the routed kernels promise that pair's chain of operations per row."""
import ctypes
import functools

import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _lora_bank_cases as C   # noqa: E402

FILL, PAD = 7.0, 64
F32c, F16c, BF16c = 0, 1, 2
UNSUPPORTED, WORKSPACE, SHAPE, ALIGN = -4, -5, -2, -6


def _bits(t):
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


def _guarded(t):
    """a dense CUDA copy of t in the middle of a larger buffer: (the copy, the bands before and after it, which nothing may write)"""
    buf = torch.full((t.numel() + 2 * PAD,), FILL, dtype=t.dtype, device="cuda")
    buf[PAD:PAD + t.numel()] = t.reshape(-1).cuda()
    return buf[PAD:PAD + t.numel()].view(t.shape), (buf[:PAD], buf[PAD + t.numel():])


@functools.lru_cache(maxsize=None)
def _device_inputs(cid):
    x, layers = C.inputs(cid)
    return x.cuda(), [(A.cuda(), B.cuda(), s.cuda(), y0) for A, B, s, y0 in layers]


def _routed(cid, slots=None, ws_fill=0x00, poison_unselected=False):
    """ops.lora_apply_routed on a case: ([y_l] on the CPU, whether every guard band — around each y and behind the workspace — is intact)"""
    from hqq_amd import ops
    case = C.BY_ID[cid]
    slots = C.SLOTS[case.slots] if slots is None else slots
    x, layers = _device_inputs(cid)
    if poison_unselected:   # NaN in A, B and scaling of every adapter that no row selects
        layers = [(A.clone(), B.clone(), s.clone(), y0) for A, B, s, y0 in layers]
        for a in range(C.N_ADAPTERS):
            if a not in slots:
                for A, B, s, _ in layers:
                    A[a] = float("nan")
                    B[a] = float("nan")
                    s[a] = float("nan")
    need = ops.lora_decode_workspace_bytes(case.M, case.K, [r for r, _ in case.layers])
    ws = torch.full((need + 256,), ws_fill, dtype=torch.uint8, device="cuda")
    ws[need:] = 0xA5
    ys, bands = zip(*[_guarded(y0) for _, _, _, y0 in layers])
    sl = torch.tensor(slots, dtype=torch.int64, device="cuda")
    ops.lora_apply_routed(x, [(A, B, s) for A, B, s, _ in layers], sl, list(ys), workspace=ws)
    torch.cuda.synchronize()
    intact = all(bool((t == FILL).all()) for pair in bands for t in pair) and bool((ws[need:] == 0xA5).all())
    return [y.cpu() for y in ys], intact


@functools.lru_cache(maxsize=None)
def _one_row(cid, m, a):
    """the reference: the existing pair on row m alone with adapter a of the bank and its scaling as a host float -> [y_l[m : m + 1]] on the CPU"""
    from hqq_amd import ops
    x, layers = _device_inputs(cid)
    ys = [y0[m:m + 1].contiguous().cuda() for _, _, _, y0 in layers]
    ops.lora_apply(x[m:m + 1].contiguous(), [(A[a].contiguous(), B[a].contiguous(), float(s[a])) for A, B, s, _ in layers], ys)
    return [y.cpu() for y in ys]


def _from_the_existing_pair(cid, slots):
    """[y_l] as the existing pair gives them row by row: row m from _one_row with its adapter, rows without one as they were"""
    _, layers = C.inputs(cid)
    out = [y0.clone() for _, _, _, y0 in layers]
    for m, slot in enumerate(slots):
        if C.valid(slot):
            for y, w in zip(out, _one_row(cid, m, slot)):
                y[m:m + 1] = w
    return out


@functools.lru_cache(maxsize=None)
def _clean(cid):
    got, intact = _routed(cid)
    assert intact
    return got


def _cids(shape, slots=None):
    """the cases of one shape — every dtype pair, every slot pattern (or those named) —: one test serves them in a loop, each assertion naming its case"""
    return [c.id for c in C.CASES if c.shape == shape and (slots is None or c.slots in slots)]


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_every_row_has_the_bits_of_the_one_row_call_with_its_adapter(shape):
    """rows with a slot in [0, n): the existing pair's bits; every other row and every guard band: untouched"""
    cids = _cids(shape)
    assert len(cids) == len(C.PAIRS) * len(C.SLOTS)
    for cid in cids:
        _check_rows(cid)


def _check_rows(cid):
    case = C.BY_ID[cid]
    got, intact = _routed(cid)
    assert intact, (cid, "a guard band around an output or behind the workspace was written")
    _, layers = C.inputs(cid)
    changed = False
    for m, slot in enumerate(C.SLOTS[case.slots]):
        if not C.valid(slot):
            for l, (g, (_, _, _, y0)) in enumerate(zip(got, layers)):
                assert torch.equal(_bits(g[m]), _bits(y0[m])), (cid, "a row without an adapter was written", m, l)
            continue
        want = _one_row(cid, m, slot)
        for l, (g, w) in enumerate(zip(got, want)):
            assert torch.equal(_bits(g[m:m + 1]), _bits(w)), (cid, m, slot, l, int((g[m:m + 1] != w).sum()))
            changed = changed or not torch.equal(g[m], layers[l][3][m])
    assert changed, (cid, "the adapter term changed nothing")


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_uniform_slots_equal_the_existing_call_on_all_rows(shape):
    cids = _cids(shape, ("M5-uniform",))
    assert len(cids) == len(C.PAIRS)
    for cid in cids:
        _check_uniform(cid)


def _check_uniform(cid):
    from hqq_amd import ops
    x, layers = _device_inputs(cid)
    ys = [y0.cuda() for _, _, _, y0 in layers]
    ops.lora_apply(x, [(A[1].contiguous(), B[1].contiguous(), float(s[1])) for A, B, s, _ in layers], ys)
    for l, (g, y) in enumerate(zip(_clean(cid), ys)):
        assert torch.equal(_bits(g), _bits(y.cpu())), (cid, l)


@pytest.mark.parametrize("shape", list(C.SHAPES))
def test_adapters_no_row_selects_change_no_bit(shape):
    """NaN in A, B and scaling of the unselected adapters: not one output bit differs, and nothing turns into a NaN"""
    cids = _cids(shape, ("M1", "M5-uniform", "M5-invalid"))
    assert len(cids) == 3 * len(C.PAIRS)
    for cid in cids:
        _check_unselected(cid)


def _check_unselected(cid):
    case = C.BY_ID[cid]
    assert any(a not in C.SLOTS[case.slots] for a in range(C.N_ADAPTERS))
    got, intact = _routed(cid, poison_unselected=True)
    assert intact
    for l, (g, w) in enumerate(zip(got, _clean(cid))):
        assert torch.equal(_bits(g), _bits(w)) and bool(torch.isfinite(g.float()).all()), (cid, l)


@pytest.mark.parametrize("shape", ["four", "r130"])
def test_the_same_bits_twice_whatever_the_workspace_held(shape):
    """(0xFF: a NaN in every fp32 slot of the workspace, also in the partials of rows without an adapter, which are neither written nor read)"""
    cids = _cids(shape, ("M5-all", "M5-invalid", "M16"))
    assert len(cids) == 3 * len(C.PAIRS)
    for cid in cids:
        _check_workspace(cid)


def _check_workspace(cid):
    a, ia = _routed(cid, ws_fill=0x00)
    b, ib = _routed(cid, ws_fill=0xFF)
    c, ic = _routed(cid, ws_fill=0xFF)
    assert ia and ib and ic
    for l, (p, q, r, w) in enumerate(zip(a, b, c, _clean(cid))):
        assert torch.equal(_bits(p), _bits(q)) and torch.equal(_bits(q), _bits(r)) and torch.equal(_bits(p), _bits(w)), (cid, l)


def test_a_captured_pair_follows_the_slots_without_a_new_capture():
    """one torch.cuda.graph capture of shrink + expand; slots.copy_(other) and a replay: the outputs are those of the other slots"""
    from hqq_amd import ops
    cid = "four-float16xfloat32-M5-all"
    case = C.BY_ID[cid]
    x, layers = _device_inputs(cid)
    first, other = C.SLOTS["M5-all"], C.SLOTS["M5-invalid"]
    slots = torch.tensor(first, dtype=torch.int64, device="cuda")
    y0s = [y0.cuda() for _, _, _, y0 in layers]
    ys = [y.clone() for y in y0s]
    ws = ops.lora_decode_workspace("cuda", case.M, case.K, [r for r, _ in case.layers])
    banks = [(A, B, s) for A, B, s, _ in layers]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):   # (a launch before the capture: nothing is loaded lazily inside it)
        ops.lora_apply_routed(x, banks, slots, ys, workspace=ws)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.lora_apply_routed(x, banks, slots, ys, workspace=ws)
    for pattern in (first, other, first):
        for y, y0 in zip(ys, y0s):
            y.copy_(y0)
        slots.copy_(torch.tensor(pattern, dtype=torch.int64))
        graph.replay()
        torch.cuda.synchronize()
        for l, (y, w) in enumerate(zip(ys, _from_the_existing_pair(cid, pattern))):
            assert torch.equal(_bits(y.cpu()), _bits(w)), (pattern, l)
    a, b = _from_the_existing_pair(cid, first), _from_the_existing_pair(cid, other)
    assert any(not torch.equal(p, q) for p, q in zip(a, b)), "the two slot patterns give different outputs"


# ---- refusals, each before anything is launched ------------------------------------------------------------------------------------------------------
def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_argument_refusals_come_before_any_launch():
    """n_adapters 0 and 257, a null bank entry, a misaligned pointer, a workspace one byte short, fp32 activations, 17 rows: the code and a message, and the
    output the call was given is untouched"""
    from hqq_amd import _C, ops
    lib = _C.lib()
    M, K, r, N, n = 2, 520, 8, 64, 3
    x = torch.randn(M, K, device="cuda").half()
    A = torch.randn(n, K, r, device="cuda")
    B = torch.randn(n, r, N, device="cuda")
    s = torch.ones(n, device="cuda")
    y = torch.full((M, N), FILL, dtype=torch.float16, device="cuda")
    slots = torch.zeros(M, dtype=torch.int64, device="cuda")
    need = ops.lora_decode_workspace_bytes(M, K, [r])
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    VP1 = ctypes.c_void_p * 1
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731

    def shrink(na=n, xp=None, Ap=A.data_ptr(), sl=None, Mr=M, dt=F16c, wsb=need):
        return lib.hqq_hip_lora_shrink_routed(1, p(x) if xp is None else xp, VP1(Ap), _i64(r), na, p(slots) if sl is None else sl, Mr, K, dt, F32c, p(ws), wsb, None)

    def expand(na=n, Bp=B.data_ptr(), sp=s.data_ptr(), Mr=M, dt=F16c, wsb=need):
        return lib.hqq_hip_lora_expand_routed(1, p(ws), wsb, VP1(Bp), VP1(sp), VP1(y.data_ptr()), _i64(N), _i64(r), na, p(slots), Mr, K, dt, F32c, None)

    for na in (0, 257):
        assert lib.hqq_hip_lora_routed_covers(1, _i64(N), _i64(r), na, M, K, F16c, F32c) == 0
        assert shrink(na=na) == UNSUPPORTED and b"adapters" in lib.hqq_hip_last_error()
        assert expand(na=na) == UNSUPPORTED and b"adapters" in lib.hqq_hip_last_error()
        assert not ops.lora_routed_covers(torch.float16, torch.float32, na, M, [N], K, [r])
    assert lib.hqq_hip_lora_routed_covers(1, _i64(N), _i64(r), 256, M, K, F16c, F32c) == 1 and ops.lora_routed_covers(torch.float16, torch.float32, 1, M, [N], K, [r])
    assert shrink(Ap=None) == SHAPE and expand(Bp=None) == SHAPE and expand(sp=None) == SHAPE
    assert shrink(Ap=A.data_ptr() + 2) == ALIGN and shrink(xp=ctypes.c_void_p(x.data_ptr() + 8)) == ALIGN and expand(Bp=B.data_ptr() + 1) == ALIGN
    assert shrink(sl=ctypes.c_void_p(slots.data_ptr() + 4)) == ALIGN
    assert shrink(wsb=need - 1) == WORKSPACE and b"workspace" in lib.hqq_hip_last_error()
    assert expand(wsb=need - 1) == WORKSPACE and b"workspace" in lib.hqq_hip_last_error()
    assert shrink(dt=F32c) == UNSUPPORTED and b"fp32 activations" in lib.hqq_hip_last_error()
    assert expand(dt=F32c) == UNSUPPORTED and b"fp32 activations" in lib.hqq_hip_last_error()
    assert shrink(Mr=17) == UNSUPPORTED and b"17 rows" in lib.hqq_hip_last_error()
    assert expand(Mr=17) == UNSUPPORTED and b"17 rows" in lib.hqq_hip_last_error()
    torch.cuda.synchronize()
    assert bool((y == FILL).all()), "a refused call wrote its output"
    # the wrappers' own checks, with the existing wrappers' exception classes
    with pytest.raises(ValueError, match="one slot per row"):
        ops.lora_shrink_routed(x, [A], slots.int(), ws)
    with pytest.raises(ValueError, match="one slot per row"):
        ops.lora_shrink_routed(x, [A], torch.zeros(M + 1, dtype=torch.int64, device="cuda"), ws)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_shrink_routed(x, [A], slots.cpu(), ws)
    with pytest.raises(ValueError, match="float32 tensors"):
        ops.lora_expand_routed(ws, [B], [1.0], slots, [y], K)
    with pytest.raises(ValueError, match="A banks"):
        ops.lora_shrink_routed(x, [A[0]], slots, ws)
    with pytest.raises(TypeError, match="ONE dtype"):
        ops.lora_shrink_routed(x, [A, A.half()], slots, ws)
    with pytest.raises(NotImplementedError, match="banks per call"):
        ops.lora_shrink_routed(x, [A] * 5, slots, ws)
    with pytest.raises(NotImplementedError, match="fp32 activations"):
        ops.lora_shrink_routed(x.float(), [A], slots, ws)
    assert bool((y == FILL).all())
