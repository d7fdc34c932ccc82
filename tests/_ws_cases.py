"""Shared by tests/test_workspace_contract_cpu.py and tests/test_workspace_contract_gpu.py: the table of split-K cases, the host-side
queries of a case (route, workspace bytes, plan) and the raw C-ABI / hqq_amd.ops calls of one.  The arena they run in: tests/_ws_arena.py."""
from __future__ import annotations

import ctypes
import itertools
from dataclasses import dataclass

import torch

from _ws_arena import BODY_BYTE, ERR_SHAPE, ERR_WORKSPACE, HEAD, HEAD_SENTINEL, arena  # noqa: F401  (the test files reach them through this module)

F16, BF16 = 1, 2
DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f16": F16, "bf16": BF16}

ROUTE_GEMV3_SLABS, ROUTE_SKINNY, ROUTE_GEMM_PIPE = 4, 6, 7
META_SCALABLE, GEMV3_SLABS, NARROW, WIDE, SKINNY_WIDE, W3S = 2, 8, 64, 128, 512, 1024
BLOCK_SILU = 4


def KS(n: int) -> int:
    return int(n) << 24


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    kind: str                 # "skinny" | "gemv3s" | "pipe" | "axis0"
    nbits: int
    dt: str                   # "f16" | "bf16"
    M: int
    Ns: tuple
    K: int
    gs: object = 64           # axis0: 16 / 64 / 128 / None (= N)
    opts: int = 0
    flags: int = 0            # axis0 grouped: BLOCK_SILU
    bias: bool = False
    grouped: bool = False     # the *_grouped entry point (always for more than one layer)
    fp64: bool = False        # also compared with the fp64 reference
    hybrid: bool = False      # pipe: the plan must report full > 0
    integer_zero: bool = False   # zero-points that pass hqq_hip_meta_check (META_SCALABLE cases)

    @property
    def id(self):
        o = self.opts
        bits = [self.kind, f"{self.nbits}b" + ("w3s" if o & W3S else ""), self.dt, f"M{self.M}", "N" + "+".join(map(str, self.Ns)), f"K{self.K}"]
        if self.kind == "axis0":
            bits.append(f"gs{self.gs}")
        if o >> 24:
            bits.append(f"ks{o >> 24}")
        for bit, name in ((SKINNY_WIDE, "wide64"), (NARROW, "nw4"), (WIDE, "nw8"), (META_SCALABLE, "sub")):
            if o & bit:
                bits.append(name)
        if self.flags & BLOCK_SILU:
            bits.append("silu")
        if self.bias:
            bits.append("bias")
        if self.grouped:
            bits.append("grouped")
        if self.hybrid:
            bits.append("hybrid")
        return "-".join(bits)

    @property
    def head_fill(self):
        return 0 if self.kind == "skinny" else HEAD_SENTINEL

    @property
    def gs_eff(self):
        return self.Ns[0] if self.gs is None else self.gs


def _per(nbits, w3s=False):
    return 2 if w3s else 8 // nbits


def _pad(N, per):
    return N + (-N) % per


def _skinny_cases():
    # (N, K, opts, bias): the built-in split on the rule tile; a forced split that does not divide K / 256 with a ragged last panel;
    # K / 256 / 2 forced splits on the forced 64-row tile; the forced tile with the built-in split of a long K
    variants = [(512, 2048, 0, False), (200, 2816, KS(3), True), (328, 2816, KS(5) | SKINNY_WIDE, False), (72, 11008, SKINNY_WIDE, True)]
    out, seen = [], set()
    for i, (nbits, lay) in enumerate([(8, 0), (4, 0), (2, 0), (3, W3S)]):
        for d, dt in enumerate(("f16", "bf16")):
            for j, M in enumerate((5, 16, 17, 33, 64)):
                N, K, opts, bias = variants[(i + j + d) % 4]
                first = (nbits, dt) not in seen
                seen.add((nbits, dt))
                out.append(Case("skinny", nbits, dt, M, (_pad(N, _per(nbits, lay)),), K, opts=opts | lay, bias=bias, fp64=first))
    out += [Case("skinny", 4, "f16", 33, (512, 200, 72), 2816, opts=KS(3), bias=True, grouped=True),
            Case("skinny", 2, "bf16", 17, (512, 136, 64), 2048, grouped=True),
            Case("skinny", 3, "f16", 64, (264, 96, 512), 2816, opts=W3S | KS(5), bias=True, grouped=True),
            Case("skinny", 8, "f16", 16, (96, 200, 40), 1024, opts=SKINNY_WIDE, grouped=True)]
    return out


def _gemv3s_cases():
    # K / 64 = 16 (a multiple of 16), 44 and 32 (tasks straddle output rows at varying offsets); N K / 64 not a multiple of 10 (173, 101: a padded
    # last slab) and ceil(N K / 640) not a multiple of 16 (a ragged last task)
    shapes = [(512, 1024), (173, 2816), (200, 2048), (101, 1024)]
    out = [Case("gemv3s", 3, "f16", M, (N,), K, opts=GEMV3_SLABS, bias=(M + i) % 2 == 0, fp64=(M == 4 and i == 1))
           for M in (1, 2, 3, 4) for i, (N, K) in enumerate(shapes)]
    out += [Case("gemv3s", 3, "f16", 3, (173, 210), 2816, opts=GEMV3_SLABS, bias=True, grouped=True),
            Case("gemv3s", 3, "f16", 1, (101, 512), 1024, opts=GEMV3_SLABS, grouped=True),
            Case("gemv3s", 3, "f16", 2, (173,), 2816, opts=GEMV3_SLABS | META_SCALABLE, integer_zero=True),
            Case("gemv3s", 3, "f16", 4, (512,), 1024, opts=GEMV3_SLABS | META_SCALABLE, bias=True, integer_zero=True),
            Case("gemv3s", 3, "f16", 1, (173, 210), 2816, opts=GEMV3_SLABS | META_SCALABLE, grouped=True, integer_zero=True)]
    return out


def _pipe_cases():
    # (N, K, opts): the planner's own split; a forced split with a ragged last one (20 steps in 3 splits of 8); the forced tile shapes
    variants = [(264, 4096, 0), (200, 1280, KS(3)), (520, 2048, NARROW | KS(2)), (1040, 2048, WIDE | KS(4)), (264, 4096, NARROW | WIDE), (72, 2816, KS(5))]
    out, seen, v = [], set(), 0
    for nbits, lay in [(8, 0), (4, 0), (2, 0), (3, W3S)]:
        for dt in ("f16", "bf16"):
            for M in (65, 128, 200, 640):
                N, K, opts = variants[v % len(variants)]
                v += 1
                first = (nbits, dt) not in seen
                seen.add((nbits, dt))
                out.append(Case("pipe", nbits, dt, M, (_pad(N, 4 * _per(nbits, lay)),), K, opts=opts | lay, bias=v % 2 == 0, fp64=first))
    out += [Case("pipe", 4, "f16", 2176, (4096,), 4096, bias=True, hybrid=True),
            Case("pipe", 4, "f16", 200, (1024, 128, 72), 2048, opts=KS(2), bias=True, grouped=True),
            Case("pipe", 2, "bf16", 65, (256, 64, 528), 4096, grouped=True),
            Case("pipe", 3, "f16", 128, (264, 1040, 96), 1280, opts=W3S | KS(3), grouped=True)]
    return out


def _axis0_cases():
    out, seen, v = [], set(), 0
    gss = (16, 64, 128, None)
    for nbits, dt in [(8, "f16"), (4, "f16"), (2, "f16"), (1, "f16"), (4, "bf16"), (2, "bf16")]:
        for M in (1, 3, 16):
            first = (nbits, dt) not in seen
            seen.add((nbits, dt))
            out.append(Case("axis0", nbits, dt, M, (256,), 1088 if v % 2 else 1024, gs=gss[v % 4], bias=v % 3 == 1, fp64=first))
            v += 1
    out += [Case("axis0", 4, "f16", 3, (256, 128), 1088, gs=64, bias=True, grouped=True, fp64=True),
            Case("axis0", 2, "bf16", 16, (128, 384, 256), 1024, gs=128, grouped=True),
            Case("axis0", 8, "f16", 1, (64, 256, 16), 1088, gs=16, bias=True, grouped=True),
            Case("axis0", 1, "f16", 16, (256, 256), 1024, gs=None, grouped=True),
            Case("axis0", 4, "f16", 1, (256, 256), 1024, gs=64, flags=BLOCK_SILU, grouped=True),
            Case("axis0", 2, "bf16", 3, (384, 384), 1088, gs=128, flags=BLOCK_SILU, bias=True, grouped=True),
            Case("axis0", 4, "f16", 16, (256,), 1024, gs=64, grouped=True)]
    return out


CASES = _skinny_cases() + _gemv3s_cases() + _pipe_cases() + _axis0_cases()
assert len({c.id for c in CASES}) == len(CASES)

# one call per route on ONE arena, every ordered pair (the production situation: one model, one buffer, routes alternating)
MIXED = [Case("skinny", 4, "f16", 33, (512, 200, 72), 2816, opts=KS(3), bias=True, grouped=True),
         Case("gemv3s", 3, "f16", 4, (173,), 2816, opts=GEMV3_SLABS, bias=True),
         Case("pipe", 4, "f16", 200, (528,), 2048, opts=NARROW | KS(2)),
         Case("axis0", 4, "f16", 3, (256,), 1088, gs=64, bias=True),
         Case("axis0", 2, "bf16", 16, (128, 384, 256), 1024, gs=128, grouped=True)]
MIXED_PAIRS = [(a, b) for a, b in itertools.product(range(len(MIXED)), repeat=2) if a != b]

# "a larger workspace is fine" / "a smaller one is refused": one case per route
SIZE_CASES = MIXED


@dataclass(frozen=True)
class AttnCase:
    rope: bool
    dt: str
    n_heads: int
    n_kv: int
    hd: int
    L: int
    pos: tuple                # one position: the batch-1 entry point; several: the *_batched one
    splits: int

    @property
    def batched(self):
        return len(self.pos) > 1

    @property
    def id(self):
        return "-".join([("rope_attn" if self.rope else "attn") + ("_batched" if self.batched else ""), self.dt, f"h{self.n_heads}kv{self.n_kv}", f"hd{self.hd}", f"L{self.L}",
                         "pos" + "+".join(map(str, self.pos)), f"s{self.splits}"])


def _attn_cases():
    # GQA everywhere but one; pos near 0 (most shares empty), pos = L - 1, a ragged batch of positions
    base = [("f16", 8, 2, 64, 512, (3,), 16), ("bf16", 8, 8, 128, 1024, (1023,), 8), ("f16", 4, 2, 256, 768, (700,), 3),
            ("bf16", 8, 2, 128, 640, (0, 639, 300), 8), ("f16", 4, 1, 64, 512, (511, 2, 17, 256), 16), ("bf16", 6, 3, 256, 384, (5, 383), 3)]
    return [AttnCase(rope, *b) for b in base for rope in (False, True)]


ATTN_CASES = _attn_cases()


# ---- host-side queries (no device needed) --------------------------------------------------------------------------------------------
def _i64(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def route(L, c: Case) -> int:
    """hqq_hip_forward_route for the axis-1 routes; axis-0 has no route number: 0"""
    if c.kind == "axis0":
        return 0
    return int(L.hqq_hip_forward_route(c.nbits, len(c.Ns), _i64(c.Ns), c.M, c.K, 64, CODE[c.dt], c.opts))


WANT_ROUTE = {"skinny": ROUTE_SKINNY, "gemv3s": ROUTE_GEMV3_SLABS, "pipe": ROUTE_GEMM_PIPE, "axis0": 0}


def need(L, c: Case) -> int:
    """the workspace query that belongs to the entry point the case calls"""
    n, Ns, dt = len(c.Ns), _i64(c.Ns), CODE[c.dt]
    if c.kind in ("skinny", "gemv3s"):
        return int(L.hqq_hip_gemv_workspace_bytes(c.nbits, n, Ns, c.M, c.K, 64, dt, c.opts))
    if c.kind == "pipe":
        if c.grouped:
            return int(L.hqq_hip_gemm_grouped_workspace_bytes(c.nbits, n, Ns, c.M, c.K, 64, dt, c.opts))
        return int(L.hqq_hip_forward_workspace_bytes(c.nbits, c.M, c.Ns[0], c.K, 64, dt, c.opts))
    if c.grouped:
        return int(L.hqq_hip_gemv_axis0_grouped_workspace_bytes(c.nbits, n, Ns, c.M, c.K, c.gs_eff, dt, c.flags))
    return int(L.hqq_hip_gemv_axis0_workspace_bytes(c.nbits, c.M, c.Ns[0], c.K, c.gs_eff, dt))


def gemm_plan(L, c: Case):
    """hqq_hip_gemm_plan of a single-layer pipe case: [waves, tokens per tile, feature tiles, token tiles, K splits, steps per split, unsplit tiles, workgroups]"""
    out = (ctypes.c_int * 8)()
    rc = L.hqq_hip_gemm_plan(c.nbits, c.M, c.Ns[0], c.K, 64, CODE[c.dt], c.opts, out)
    assert rc == 0, (c.id, rc)
    return list(out)


def attn_need(L, c: AttnCase) -> int:
    return int(L.hqq_hip_attn_decode_workspace_bytes(len(c.pos) * c.n_heads, c.hd, c.splits))


# ---- operands and calls (device) -----------------------------------------------------------------------------------------------------
def operands(ops, c: Case, seed: int):
    """x, per-layer (Wq, scale, zero, bias, N) as the entry point takes them, and the layers' dequantised weights [N, K] (hqq_hip_dequantize)"""
    dt = DT[c.dt]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(c.M, c.K, generator=g).to(dt).cuda()
    layers, Wd = [], []
    for N in c.Ns:
        gs = c.gs_eff
        C = N * c.K // gs
        shape = (gs, C) if c.kind == "axis0" else (C, gs)
        U = torch.randint(0, 2 ** c.nbits, shape, generator=g, dtype=torch.uint8)
        s = (torch.rand(C, generator=g) * 0.004 + 0.001).to(dt)
        z = torch.rand(C, generator=g) * (2 ** c.nbits - 1)
        z = (z.round() if c.integer_zero else z).to(dt)
        b = torch.randn(N, generator=g).to(dt).cuda() if c.bias else None
        s, z = s.cuda(), z.cuda()
        Wq = ops.pack(c.nbits, U.cuda())
        if c.kind == "axis0":
            s, z = s.reshape(1, -1), z.reshape(1, -1)
            Wd.append(ops.dequantize(Wq, s.reshape(-1), z.reshape(-1), N, c.K, gs, c.nbits, 0))
        else:
            s, z = s.reshape(-1, 1), z.reshape(-1, 1)
            Wd.append(ops.dequantize(Wq, s.reshape(-1), z.reshape(-1), N, c.K, gs, c.nbits))
            if c.opts & W3S:
                Wq = ops.w3s_pack(Wq, N, c.K)
        layers.append((Wq, s, z, b, N))
    return x, layers, Wd


def out_Ns(c: Case):
    return c.Ns[:1] if c.flags & BLOCK_SILU else c.Ns


def new_outputs(c: Case, fill=float("nan")):
    return [torch.full((c.M, N), fill, dtype=DT[c.dt], device="cuda") for N in out_Ns(c)]


def _vp(ptrs):
    return (ctypes.c_void_p * len(ptrs))(*ptrs)


def _ptr(t):
    return None if t is None else t.data_ptr()


def call_raw(L, c: Case, x, layers, outs, ws_ptr, ws_bytes) -> int:
    """the C entry point itself, with the caller's workspace pointer and size; returns its return code"""
    st = torch.cuda.current_stream().cuda_stream
    n, dt = len(layers), CODE[c.dt]
    Ns = _i64([l[4] for l in layers])
    if n == 1 and not c.grouped:
        Wq, s, z, b, N = layers[0]
        if c.kind == "axis0":
            return L.hqq_hip_gemv_axis0(c.nbits, _ptr(x), _ptr(Wq), _ptr(s), _ptr(z), _ptr(b), _ptr(outs[0]), c.M, N, c.K, c.gs_eff, dt, c.opts, ws_ptr, ws_bytes, st)
        fn = L.hqq_hip_forward if c.kind == "pipe" else L.hqq_hip_gemv
        return fn(c.nbits, _ptr(x), _ptr(Wq), _ptr(s), _ptr(z), _ptr(b), _ptr(outs[0]), c.M, N, c.K, 64, dt, c.opts, ws_ptr, ws_bytes, st)
    W, S, Z = (_vp([_ptr(l[i]) for l in layers]) for i in range(3))
    B = _vp([_ptr(l[3]) for l in layers]) if c.bias else None
    Y = _vp([_ptr(o) for o in outs] + [None] * (n - len(outs)))
    if c.kind == "axis0":
        return L.hqq_hip_gemv_axis0_grouped(c.nbits, n, _ptr(x), W, S, Z, B, Y, Ns, c.M, c.K, c.gs_eff, dt, c.opts, c.flags, ws_ptr, ws_bytes, st)
    fn = L.hqq_hip_gemm_grouped if c.kind == "pipe" else L.hqq_hip_gemv_grouped
    return fn(c.nbits, n, _ptr(x), W, S, Z, B, Y, Ns, c.M, c.K, 64, dt, c.opts, ws_ptr, ws_bytes, st)


def call_clean(ops, c: Case, x, layers):
    """the same call through hqq_amd.ops: its own zero-filled, oversized, only-ever-growing workspace"""
    if len(layers) == 1 and not c.grouped:
        Wq, s, z, b, N = layers[0]
        if c.kind == "axis0":
            return [ops.gemv_axis0(x, Wq, s, z, b, N, c.K, c.gs, c.nbits, opts=c.opts)]
        if c.kind == "pipe":
            return [ops.forward(x, Wq, s, z, b, N, c.K, 64, c.nbits, fused=True, opts=c.opts)]
        return [ops.gemv(x, Wq, s, z, b, N, c.K, 64, c.nbits, opts=c.opts)]
    if c.kind == "axis0":
        return ops.gemv_axis0_grouped(x, layers, c.K, c.gs, c.nbits, flags=c.flags)
    if c.kind == "pipe":
        return ops.gemm_grouped(x, layers, c.K, 64, c.nbits, opts=c.opts)
    return ops.gemv_grouped(x, layers, c.K, 64, c.nbits, opts=c.opts)


def same_bits(a, b) -> bool:
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))
