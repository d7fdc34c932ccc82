"""CPU half of the un-merged LoRA decode kernels' tests (csrc/lora_decode.hip): the cases of tests/_lora_decode_cases.py checked against their own
premises — the constructed cases are exact and sensitive, the derived bound holds for the reference's arithmetic in another summation order — and
the C ABI's host side: coverage, workspace size, every refusal with its code and message before anything is launched."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")

import _lora_decode_cases as C   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32c, F16c, BF16c = 0, 1, 2
UNSUPPORTED, WORKSPACE, SHAPE = -4, -5, -2


@pytest.mark.parametrize("cid", [c.id for c in C.CONSTRUCTED])
def test_constructed_cases_are_exact(cid):
    case = C.BY_ID[cid]
    w1, w2, w3 = C.exactness(case)
    assert w1 < 2 ** 24 and w2 < 2 ** 24 and w3 < 1, (w1, w2, w3)
    x, layers = C.inputs(cid)   # (asserts that every input is exact in its dtype)
    for (A, B, s, y0), (A64, B64, _, y64) in zip(layers, C.constructed_arrays(case)[1]):
        assert torch.equal(A.double(), torch.from_numpy(A64)) and torch.equal(B.double(), torch.from_numpy(B64)) and torch.equal(y0.double(), torch.from_numpy(y64))
        m, e = torch.frexp(torch.tensor(float(s)))
        assert float(m) == 0.5, "s is a power of two"
    # the adapter term is not lost in y0's rounding: it changes the output somewhere
    assert any(not torch.equal(y, l[3]) for y, l in zip(C.expected(cid), layers))


@pytest.mark.parametrize("cid", [c.id for c in C.CONSTRUCTED])
def test_constructed_cases_are_sensitive(cid):
    """one A row, one B column or one K slice displaced in the closed form changes the expected bits of layer 0"""
    case = C.BY_ID[cid]
    want = C.expected(cid)[0]
    r, N, _ = case.layers[0]
    S = C.slices(case.K, r)
    for disp in [("A_row", 0), ("A_row", case.K - 1), ("A_row", case.K // 2), ("B_col", 0), ("B_col", N - 1)] + [("slice", i) for i in sorted({0, S - 1, S // 2})]:
        assert not torch.equal(C.constructed_expected(case, disp)[0], want), disp


@pytest.mark.parametrize("cid", [c.id for c in C.RANDN])
def test_the_derived_bound_holds_for_another_summation_order(cid):
    x, layers = C.inputs(cid)
    for (A, B, s, y0), (y64, bound) in zip(layers, C.expected(cid)):
        got = C.emulate_fp32(x, A, B, s, y0)
        err = (got.double() - y64).abs()
        assert bool((err <= bound).all()), float((err / bound).max())


def test_case_families_cover_the_kernels_edges():
    names = {c.name for c in C.CASES}
    for need in ("K8", "K256", "K248", "K264", "K840", "K11008", "r1", "r2", "r3", "r8", "r16", "r17", "r64", "r255", "r256", "N8", "N256", "N248", "N264", "N584",
                 "M1", "M2", "M5", "M16", "group3", "base"):
        assert need in names, need
    assert C.KC == 256 and C.kslice(64) == C.KC and C.slices(840, 8) == 4 and C.slices(11008, 64) == 43 and 584 == 2 * C.EN + 72
    for dt, ldt in C.PAIRS:
        for kind in ("constructed", "randn"):
            assert any(c.dt == dt and c.ldt == ldt and c.kind == kind and len(c.layers) == 3 for c in C.CASES)


def test_the_restated_constants_are_the_sources():
    src = open(os.path.join(ROOT, "hqq_amd", "csrc", "lora_decode.hip")).read()
    for name, val in (("LD_THREADS", C.THREADS), ("LD_KC", C.KC), ("LD_EN", C.EN), ("LD_MAX_R", C.MAX_R)):
        assert re.search(rf"constexpr int {name} = {val};", src), name
    assert "return r <= 64 ? 256 : (r <= 128 ? 512 : 1024);" in src
    assert "return M <= 1 ? 1 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16));" in src
    hdr = open(os.path.join(ROOT, "include", "hqq_hip.h")).read()
    assert f"#define HQQ_GEMV_MAX_M {C.MAX_M}\n" in hdr and f"#define HQQ_GEMV_MAX_GROUP {C.MAX_GROUP}\n" in hdr


# ---- the C ABI's host side ---------------------------------------------------------------------------------------------------------------------------
def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    from hqq_amd import _C
    return _C.lib()


def test_header_binding_and_library_agree(lib):
    from hqq_amd import _C
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hqq_hip.h")).read(), flags=re.S)
    for name, nargs in (("hqq_hip_lora_decode_covers", 8), ("hqq_hip_lora_decode_workspace_bytes", 4), ("hqq_hip_lora_shrink", 11), ("hqq_hip_lora_expand", 13)):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs == len(_C.SYMBOLS[name][1]), name
        assert hasattr(lib, name)
    assert lib.hqq_hip_abi_version() == _C.ABI_VERSION == 9


def test_covers_and_workspace_size_are_host_arithmetic(lib):
    from hqq_amd import ops
    cov = lib.hqq_hip_lora_decode_covers
    assert cov(1, _i64(64), _i64(8), 1, 64, F16c, F32c, F32c) == 1
    assert cov(3, _i64(4096, 1024, 1024), _i64(16, 64, 256), 16, 4096, BF16c, BF16c, BF16c) == 1
    assert cov(4, _i64(8, 8, 8, 8), _i64(1, 2, 3, 4), 5, 8, F16c, F16c, F16c) == 1
    for M, K, rs in ((1, 8, (1,)), (2, 520, (8,)), (5, 840, (8, 17, 3)), (16, 11008, (64, 64)), (16, 1032, (256,)), (3, 520, (128, 129))):
        got = lib.hqq_hip_lora_decode_workspace_bytes(len(rs), _i64(*rs), M, K)
        assert got == C.workspace_bytes(M, K, rs) == ops.lora_decode_workspace_bytes(M, K, rs) and got % 16 == 0 and got > 0, (M, K, rs)
    assert ops.lora_decode_covers(torch.float16, torch.float32, 1, [4096, 1024, 1024], 4096, [16, 16, 16])
    assert not ops.lora_decode_covers(torch.float32, torch.float32, 1, [4096], 4096, [16])
    assert not ops.lora_decode_covers(torch.float16, torch.float32, 1, [4096], 4096, [257])
    assert not ops.lora_decode_covers(torch.float16, torch.float32, 1, [4096, 4096], 4096, [16])     # one rank per layer
    # what can be merged can be decoded un-merged: the same ranks
    assert ops.LORA_DECODE_MAX_R == ops.LORA_MERGE_MAX_R == C.MAX_R
    for r in (1, 256):
        assert ops.lora_merge_covers(torch.float16, torch.float32, 64, 64, 64, 4, 1, r) and ops.lora_decode_covers(torch.float16, torch.float32, 1, [64], 64, [r])
    assert not ops.lora_merge_covers(torch.float16, torch.float32, 64, 64, 64, 4, 1, 257)


REFUSALS = [
    # (what, n, Ns, rs, M, K, dtype, a_dtype, b_dtype, a word of the message)
    ("r 0", 1, (64,), (0,), 1, 64, F16c, F32c, F32c, b"rank 0"),
    ("r 257", 1, (64,), (257,), 1, 64, F16c, F32c, F32c, b"rank 257"),
    ("M 0", 1, (64,), (8,), 0, 64, F16c, F32c, F32c, b"0 rows"),
    ("M 17", 1, (64,), (8,), 17, 64, F16c, F32c, F32c, b"17 rows"),
    ("K % 8", 1, (64,), (8,), 1, 68, F16c, F32c, F32c, b"K=68"),
    ("N % 8", 1, (68,), (8,), 1, 64, F16c, F32c, F32c, b"N=68"),
    ("mixed A / B dtypes", 1, (64,), (8,), 1, 64, F16c, F32c, F16c, b"different dtypes"),
    ("fp32 activations", 1, (64,), (8,), 1, 64, F32c, F32c, F32c, b"fp32 activations"),
    ("5 layers", 5, (64,) * 5, (8,) * 5, 1, 64, F16c, F32c, F32c, b"5 layers"),
]


@pytest.mark.parametrize("what,n,Ns,rs,M,K,dt,adt,bdt,word", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_come_with_code_and_message_before_any_launch(lib, what, n, Ns, rs, M, K, dt, adt, bdt, word):
    """(no GPU in this process: a call that got as far as a launch would fail differently)"""
    p16 = ctypes.c_void_p(16)
    VP = ctypes.c_void_p * n
    ptrs = VP(*([16] * n))
    assert lib.hqq_hip_lora_decode_covers(n, _i64(*Ns), _i64(*rs), M, K, dt, adt, bdt) == 0
    assert word in lib.hqq_hip_last_error() and b"not covered" in lib.hqq_hip_last_error(), lib.hqq_hip_last_error()
    big = 1 << 30
    if what != "N % 8":   # (the shrink has no N)
        if what != "mixed A / B dtypes":
            assert lib.hqq_hip_lora_decode_workspace_bytes(n, _i64(*rs), M, K) == 0 or what == "fp32 activations"
        if adt == bdt:
            assert lib.hqq_hip_lora_shrink(n, p16, ptrs, _i64(*rs), M, K, dt, adt, p16, big, None) == UNSUPPORTED
            assert word in lib.hqq_hip_last_error()
    if adt == bdt:
        assert lib.hqq_hip_lora_expand(n, p16, big, ptrs, (ctypes.c_float * n)(*([1.0] * n)), ptrs, _i64(*Ns), _i64(*rs), M, K, dt, bdt, None) == UNSUPPORTED
        assert word in lib.hqq_hip_last_error()


def test_too_small_a_workspace_is_refused_before_any_launch(lib):
    p16 = ctypes.c_void_p(16)
    VP1 = (ctypes.c_void_p * 1)(16)
    need = C.workspace_bytes(2, 520, (8,))
    for ws, nbytes in ((p16, need - 16), (None, need), (ctypes.c_void_p(24), need)):
        assert lib.hqq_hip_lora_shrink(1, p16, VP1, _i64(8), 2, 520, F16c, F32c, ws, nbytes, None) == WORKSPACE
        assert b"workspace" in lib.hqq_hip_last_error() and str(need).encode() in lib.hqq_hip_last_error()
        assert lib.hqq_hip_lora_expand(1, ws, nbytes, VP1, (ctypes.c_float * 1)(1.0), VP1, _i64(64), _i64(8), 2, 520, F16c, F32c, None) == WORKSPACE
        assert b"workspace" in lib.hqq_hip_last_error()
    # null and misaligned arguments
    assert lib.hqq_hip_lora_shrink(1, None, VP1, _i64(8), 2, 520, F16c, F32c, p16, need, None) == SHAPE
    assert lib.hqq_hip_lora_shrink(1, ctypes.c_void_p(8), VP1, _i64(8), 2, 520, F16c, F32c, p16, need, None) == -6
    assert lib.hqq_hip_lora_shrink(1, p16, (ctypes.c_void_p * 1)(18), _i64(8), 2, 520, F16c, F32c, p16, need, None) == -6


def test_ops_refuse_cpu_tensors_and_bad_groups():
    from hqq_amd import ops
    x, A = torch.zeros(1, 64, dtype=torch.float16), torch.zeros(64, 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_shrink(x, [A], torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_apply(x, [(A, torch.zeros(8, 64), 1.0)], [torch.zeros(1, 64, dtype=torch.float16)], workspace=torch.zeros(64, dtype=torch.uint8))
    with pytest.raises(TypeError, match="share a dtype"):
        ops.lora_apply(x, [(A, torch.zeros(8, 64, dtype=torch.float16), 1.0)], [torch.zeros(1, 64, dtype=torch.float16)])
    with pytest.raises(NotImplementedError, match="not covered"):
        ops.lora_decode_workspace("cpu", 17, 64, [8])
