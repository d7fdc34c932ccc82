"""The guarded workspace arena of tests/test_workspace_contract_gpu.py (the case table and the calls live in tests/_ws_cases.py).

The contract under test (include/hqq_hip.h, "Workspace"; csrc/hqq_common.h WS_COUNTER_BYTES): a caller passes exactly
`*_workspace_bytes(...)` bytes; the first 256 KiB (the head) are arrival counters, zero before and after every call, which only the
skinny GEMV touches; everything past the head (the body) is written before it is read, whatever it held."""
from __future__ import annotations

import torch

HEAD = 256 << 10            # WS_COUNTER_BYTES
GUARD_MIN = 1 << 20
GUARD_BYTE = 0xA5
BODY_BYTE = 0xFF            # every fp32 a NaN, every int -1
HEAD_SENTINEL = 0x3C        # what a head no kernel may touch is filled with
ERR_SHAPE, ERR_WORKSPACE = -2, -5


# ---- the arena -----------------------------------------------------------------------------------------------------------------
class Arena:
    """[guard | need bytes | guard] in ONE allocation: a kernel that runs past either end of the `need` bytes by up to their own length
    still writes memory this test owns"""

    def __init__(self, need: int, head_fill, device):
        self.need = int(need)
        self.head_bytes = 0 if head_fill is None else HEAD
        assert self.need > self.head_bytes and self.need % 16 == 0
        body = self.need - self.head_bytes
        self.guard = max(GUARD_MIN, (body + 15) // 16 * 16)
        self.buf = torch.empty(self.guard + self.need + self.guard, dtype=torch.uint8, device=device)
        self.lo = self.buf[:self.guard]
        self.inner = self.buf[self.guard:self.guard + self.need]
        self.hi = self.buf[self.guard + self.need:]
        self.head = self.inner[:self.head_bytes]
        self.body = self.inner[self.head_bytes:]
        self.head_fill = head_fill
        self.lo.fill_(GUARD_BYTE)
        self.hi.fill_(GUARD_BYTE)
        self.poison()
        if head_fill is not None:
            self.head.fill_(head_fill)
        self.ptr = self.inner.data_ptr()
        assert self.ptr % 16 == 0

    def poison(self):
        self.body.fill_(BODY_BYTE)

    def check(self, what=""):
        """after a call (synchronises): both guards byte-identical to their pattern, the head as it was"""
        torch.cuda.synchronize()
        for name, g in (("below", self.lo), ("above", self.hi)):
            bad = g != GUARD_BYTE
            n = int(bad.sum())
            if n:
                first = int(bad.nonzero()[0])
                off = first - self.guard if name == "below" else first
                raise AssertionError(f"{what}: {n} bytes of the guard {name} the workspace were overwritten (first at offset {off} from its edge)")
        if self.head_fill == 0:
            n = int(torch.count_nonzero(self.head))
            assert n == 0, f"{what}: {n} bytes of the counter head are not back at zero"
        elif self.head_fill is not None:
            n = int((self.head != self.head_fill).sum())
            assert n == 0, f"{what}: {n} bytes of the counter head were written by a call that is documented to keep out of it"


def arena(need: int, head_fill, device="cuda") -> Arena:
    """head_fill: 0 (the skinny GEMV: the one user of the counters), HEAD_SENTINEL (every other route: must stay untouched), or None (the
    attention record buffer: no head, all body).  Returns the arena: .ptr is the inner pointer, .need the bytes to pass."""
    return Arena(need, head_fill, device)
