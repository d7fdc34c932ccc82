"""CPU test of the decode-attention entry points' argument checks (csrc/block.hip, csrc/kv_cache.hip, csrc/attn_tile.hip): every call below is well-formed
but for ONE fault and must return that entry point's code for it before anything is launched.  The codes are literals: the routes differ on purpose (the
quantised-cache pair refuses through the cache's coverage rule, HQQ_ERR_UNSUPPORTED, where the dense entries report a bad shape), and a change of the shared
host front must not move any of them.  Nothing is launched: no GPU is needed."""
import ctypes
import os

import pytest

F32, F16 = 0, 1
SHAPE, UNSUPPORTED, ALIGN = -2, -4, -6

P = ctypes.c_void_p(16)      # aligned, never dereferenced: every call below fails its argument checks first
MIS = ctypes.c_void_p(24)    # not 16-byte aligned
N_HEADS, HD, SPLITS = 8, 128, 4

ENTRIES = ("hqq_hip_attn_decode", "hqq_hip_attn_decode_batched", "hqq_hip_attn_decode_shared", "hqq_hip_attn_decode_tiled", "hqq_hip_rope_attn_decode",
           "hqq_hip_rope_attn_decode_batched", "hqq_hip_attn_decode_kvq", "hqq_hip_attn_decode_kvq_batched")
SINGLE = ("hqq_hip_attn_decode", "hqq_hip_rope_attn_decode", "hqq_hip_attn_decode_kvq")   # one sequence: no batch / rows argument
ROWS = 2                     # of the other entries


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    if not os.path.exists(_C.LIB_PATH):
        _C.build()
    return _C.lib()


def _need(entry):
    """bytes of the records of a SPLITS-way launch of the well-formed call"""
    return (1 if entry in SINGLE else ROWS) * N_HEADS * SPLITS * (HD + 2) * 4


def _call(L, entry, q=P, out=P, hd=HD, n_kv=2, cache_len=256, splits=1, ws=None, ws_bytes=0, dtype=F16, rows=ROWS, nbits=8):
    tail = (N_HEADS, n_kv, hd) + ((64,) if "kvq" in entry else ()) + (cache_len, 0.1, dtype, splits, ws, ws_bytes, None)
    batch = () if entry in SINGLE else (rows,)
    if "kvq" in entry:
        args = (nbits, q, P, P, P, P, P, P, P) + batch + (out,)
    elif "rope" in entry:
        args = (q, P, P, P, P, P) + batch + (P, P, out)
    else:
        args = (q, P, P, P) + batch + (out,)
    return getattr(L, entry)(*(args + tail))


# fault -> the arguments that carry it (a callable of the entry where the workspace size matters)
FAULTS = {
    "null q": lambda e: dict(q=None),
    "null out": lambda e: dict(out=None),
    "misaligned q": lambda e: dict(q=MIS),
    "head_dim 96": lambda e: dict(hd=96),
    "n_heads 8, n_kv_heads 3": lambda e: dict(n_kv=3),
    "cache_len 0": lambda e: dict(cache_len=0),
    "cache_len 30001": lambda e: dict(cache_len=30001),
    "splits 0": lambda e: dict(splits=0),
    "splits 65": lambda e: dict(splits=65),
    "splits 4, null workspace": lambda e: dict(splits=SPLITS, ws=None, ws_bytes=_need(e)),
    "splits 4, workspace 4 bytes short": lambda e: dict(splits=SPLITS, ws=P, ws_bytes=_need(e) - 4),
    "dtype fp32": lambda e: dict(dtype=F32),
    "rows 17": lambda e: dict(rows=17),
    "nbits 3": lambda e: dict(nbits=3),
}

S, U, A, _ = SHAPE, UNSUPPORTED, ALIGN, None   # _: the fault does not exist for that entry
# columns: ENTRIES in order —        decode  batched  shared  tiled  rope  rope_batched  kvq  kvq_batched
EXPECT = {
    "null q":                            (S, S, S, S, S, S, S, S),
    "null out":                          (S, S, S, S, S, S, S, S),
    "misaligned q":                      (A, A, A, A, A, A, A, A),
    "head_dim 96":                       (U, U, U, U, U, U, U, U),
    "n_heads 8, n_kv_heads 3":           (S, S, S, S, S, S, S, S),
    "cache_len 0":                       (S, S, S, S, S, S, U, U),
    "cache_len 30001":                   (S, S, S, S, S, S, U, U),
    "splits 0":                          (S, S, S, S, S, S, S, S),
    "splits 65":                         (S, S, S, S, S, S, S, S),
    "splits 4, null workspace":          (S, S, S, S, S, S, S, S),
    "splits 4, workspace 4 bytes short": (S, S, S, S, S, S, S, S),
    "dtype fp32":                        (U, U, U, U, U, U, U, U),
    "rows 17":                           (_, _, _, S, _, _, _, _),
    "nbits 3":                           (_, _, _, _, _, _, U, U),
}

CELLS = [(fault, entry, EXPECT[fault][i]) for fault in FAULTS for i, entry in enumerate(ENTRIES) if EXPECT[fault][i] is not None]


def test_the_table_covers_every_fault_and_entry():
    assert set(EXPECT) == set(FAULTS) and all(len(row) == len(ENTRIES) for row in EXPECT.values())
    from hqq_amd import _C
    assert all(e in _C.SYMBOLS for e in ENTRIES)


@pytest.mark.parametrize("fault,entry,code", CELLS, ids=[f"{e[len('hqq_hip_'):]}-{f}" for f, e, _c in CELLS])
def test_one_fault_one_code(L, fault, entry, code):
    assert _call(L, entry, **FAULTS[fault](entry)) == code
    msg = L.hqq_hip_last_error()
    assert entry.encode() in msg
    if "workspace" in fault:
        assert b"workspace" in msg
    if fault == "head_dim 96":
        assert b"not covered" in msg


def test_workspace_of_exactly_the_records_passes_the_check(L):
    # the size the two workspace cells are short of is the documented one
    for entry in ENTRIES:
        assert L.hqq_hip_attn_decode_workspace_bytes((1 if entry in SINGLE else ROWS) * N_HEADS, HD, SPLITS) == _need(entry)
