"""Tensor-level wrappers over the C ABI (include/hqq_hip.h).  PyTorch only supplies device memory and the
current HIP stream; every function below enqueues hand-written gfx950 kernels from libhqq_hip.so.

No fallbacks: tensors must live on a ROCm device ("cuda" in torch), and a missing library or an
unsupported configuration raises (RuntimeError / NotImplementedError) instead of silently running
eager PyTorch.
"""
from __future__ import annotations

import ctypes
import functools

import torch
from torch import Tensor

from . import _C

F32, F16, BF16, U8 = 0, 1, 2, 3
_DT = {torch.float32: F32, torch.float16: F16, torch.bfloat16: BF16, torch.uint8: U8}
PER = {8: 1, 4: 2, 2: 4, 1: 8, 3: 10}
# Quantizer.bit_to_packing (hqq/core/quantize.py:40-49): container width per nbits
PACK_BITS = {8: 8, 6: 8, 5: 8, 4: 4, 3: 3, 2: 2, 1.58: 2, 1: 1}
GEMV_MAX_M = 16     # HQQ_GEMV_MAX_M
SKINNY_MAX_M = 64   # HQQ_GEMV_MAX_M_SKINNY
GEMV_EXACT, GEMV_FACTORED = 0, 1
GEMV_MAX_GROUP = 4
# per-call option bits of the C ABI (include/hqq_hip.h HQQ_OPT_*)
OPT_FACTORED, OPT_META_SCALABLE, OPT_GEMV3_ROWWISE, OPT_GEMV3_SLABS, OPT_GEMM_REGTILE, OPT_GEMM_CLASSIC, OPT_GEMM_NARROW, OPT_GEMM_WIDE, OPT_GEMM_NOHYBRID, OPT_SKINNY_WIDE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512
OPT_W3S = 1024   # nbits = 3: W_q is the 3-bit stream layout of w3s_pack(), not the reference container
OPT_BATCH_SPLITK = 2048   # LAB builds only (tools/lab_kwave/build.sh): force the split-K kernel where the quarantined no-split kernel would serve


def OPT_SKINNY_KS(n: int) -> int:
    return int(n) << 24


# the kernel a call runs (include/hqq_hip.h HQQ_ROUTE_*, the table of routes); the first six are hqq_hip_gemv's
ROUTE_ROWWISE, ROUTE_ROWWISE_W3S, ROUTE_GEMV3_ROWS, ROUTE_GEMV3_SLABS, ROUTE_MFMA16, ROUTE_SKINNY, ROUTE_GEMM_PIPE, ROUTE_GEMM_TILE = range(1, 9)
DECODE_ROUTES = frozenset(range(ROUTE_ROWWISE, ROUTE_SKINNY + 1))


@functools.lru_cache(maxsize=4096)
def route(dtype, M: int, Ns: tuple, K: int, group_size, nbits: int, opts: int = 0) -> int:
    """hqq_hip_forward_route: the ROUTE_* for x [M, K] through layers of Ns (a tuple) output rows, or the negative HQQ_ERR_* of the refusal"""
    n = len(Ns)
    return int(_C.lib().hqq_hip_forward_route(int(nbits), n, (ctypes.c_int64 * n)(*Ns), int(M), int(K), int(group_size or 0), _DT.get(dtype, -1), int(opts)))


@functools.lru_cache(maxsize=4096)
def prefers_fused(dtype, M: int, N: int, K: int, group_size, nbits: int, w3s: bool = False) -> bool:
    """hqq_hip_forward_prefers_fused: the fused kernels are measured ahead of dequantise + GEMM for this shape (a speed hint).  A layer in the 3-bit
    stream layout runs the 4-bit layer's GEMM plan and is asked as one (the query takes no option bits)."""
    return dtype in _DT and bool(_C.lib().hqq_hip_forward_prefers_fused(4 if w3s else int(nbits), int(M), int(N), int(K), int(group_size or 0), _DT[dtype]))


# Default arithmetic of the decode wrappers below when a call passes no `opts` — a convenience of THIS module (tools, tests,
# bench); the library itself holds no mode.
_default_opts = 0


def is_available() -> bool:
    """True when libhqq_hip.so loads and a ROCm GPU is visible."""
    try:
        _C.lib()
    except (RuntimeError, OSError):
        return False
    return torch.cuda.is_available()


def _dt(t: torch.dtype) -> int:
    try:
        return _DT[t]
    except KeyError:
        raise TypeError(f"hqq_amd: dtype {t} not supported by the HIP kernels") from None


def _dev(*ts: Tensor) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError("hqq_amd: HIP kernels need tensors on the GPU (device='cuda'); there is no CPU path")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def set_gemv_mode(mode: int) -> None:
    """GEMV_EXACT (default): reference-identical weights on the MFMA path; GEMV_FACTORED: fp32-factored dot2 path.  Applies to raw
    ops.* calls that pass no `opts` and to every layer forward (HQQLinear with HQQBackend.HIP, HQQLinearHIP, grouped projections),
    which combine it with their own meta-dependent bits through layer_opts()."""
    global _default_opts
    if mode not in (GEMV_EXACT, GEMV_FACTORED):
        raise ValueError(f"hqq_amd: unknown gemv mode {mode}")
    _default_opts = OPT_FACTORED if mode == GEMV_FACTORED else 0


def get_gemv_mode() -> int:
    return GEMV_FACTORED if (_default_opts & OPT_FACTORED) else GEMV_EXACT


def _opts(opts) -> int:
    return _default_opts if opts is None else int(opts)


def layer_opts(meta_opts: int) -> int:
    """Option bits for a LAYER's forward: its own meta-dependent bits (0 / OPT_META_SCALABLE), unless set_gemv_mode(GEMV_FACTORED) is in
    force — then the factored arithmetic for every layer (the three-op bit belongs to the exact rebuild and is dropped)."""
    if _default_opts & OPT_FACTORED:
        return OPT_FACTORED | (int(meta_opts) & OPT_W3S)   # (the layout bit describes the tensor, not the arithmetic: it always travels)
    return int(meta_opts)


# ---- caller-owned workspace of the split-K / slab-sharing decode launches (include/hqq_hip.h "Workspace") --------------------
# One zero-initialised buffer per device, sized for the largest launch seen so far.  Growing allocates a NEW buffer and keeps
# the old ones alive: a hipGraph captured earlier has the old address baked in and must stay valid (never free what a graph
# may reference).  Growth cannot happen inside stream capture (the new buffer would belong to the graph's private pool).
_ws_cur: dict = {}
_ws_retired: list = []
_WS_MIN = 8 << 20


_ws_last_stream: dict = {}


def _ws_serialise(key: int) -> None:
    """The device's workspace is ONE buffer (arrival counters + parked partial sums) and the C ABI forbids sharing it between calls that
    may run concurrently: a call from another stream than the previous workspace user first waits for everything that stream has
    enqueued.  (Outside stream capture; inside a capture the launches of one capture are ordered by the capture itself unless the
    caller forks streams — then give each branch its own buffer through the C ABI.)"""
    if torch.cuda.is_current_stream_capturing():
        return   # nothing runs during a capture, and a capture stream must not become the "last user" an eager call later waits on
    cur = torch.cuda.current_stream(key)
    last = _ws_last_stream.get(key)
    if last is not None and last != cur:
        cur.wait_stream(last)
    _ws_last_stream[key] = cur


def release_retired_workspaces() -> int:
    """Free the workspace buffers that growth retired.  Only when no captured hipGraph still replays launches that were captured with
    them (the caller knows; the library cannot).  Returns the bytes released."""
    n = sum(t.numel() for t in _ws_retired)
    _ws_retired.clear()
    return n


def reserve_workspace(device, nbytes: int) -> Tensor:
    """make sure the device's decode workspace holds `nbytes`; call it before capturing a graph whose launches need one"""
    dev = torch.device(device)
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    cur = _ws_cur.get(key)
    _ws_serialise(key)
    if cur is not None and cur.numel() >= nbytes:
        return cur
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"hqq_amd: this launch needs {nbytes} bytes of decode workspace, more than was reserved before stream capture; "
                           "run the step once eagerly (or call hqq_amd.ops.reserve_workspace) before capturing")
    new = torch.zeros(max(int(nbytes), _WS_MIN), dtype=torch.uint8, device=torch.device("cuda", key))
    if cur is not None:
        _ws_retired.append(cur)
    _ws_cur[key] = new
    return new


def _workspace(x: Tensor, nbits, Ns, M, K, group_size, opts):
    n = len(Ns)
    need = int(_C.lib().hqq_hip_gemv_workspace_bytes(int(nbits), n, (ctypes.c_int64 * n)(*[int(v) for v in Ns]), int(M), int(K), int(group_size),
                                                     _dt(x.dtype), int(opts)))
    if not need:
        return None, 0
    ws = reserve_workspace(x.device, need)
    return ws.data_ptr(), ws.numel()


def meta_scalable(scale: Tensor, zero: Tensor, N: int, K: int, group_size: int, nbits: int) -> bool:
    """True when every (zero, scale) pair of the layer can take the three-op exact weight rebuild (hqq_hip_meta_check == 0 failing
    groups): pass OPT_META_SCALABLE for it then.  Synchronises (one 4-byte read-back): call it when a layer is prepared, not per forward."""
    _dev(scale, zero)
    if scale.dtype != torch.float16 or zero.dtype != torch.float16 or nbits not in (8, 4, 3, 2, 1) or (nbits != 3 and N % PER[nbits]):
        return False
    cnt = torch.empty(1, dtype=torch.int32, device=scale.device)
    with torch.cuda.device(scale.device):
        rc = _C.lib().hqq_hip_meta_check(int(nbits), _p(scale.contiguous()), _p(zero.contiguous()), int(N), int(K), int(group_size), F16, _p(cnt), _stream())
    _C.check(rc, "hqq_hip_meta_check")
    return int(cnt.item()) == 0


def w3s_covers(N: int, K: int, group_size) -> bool:
    """layers the 3-bit stream layout (csrc/w3s.h) can hold: group_size 64, an even number of output rows"""
    return group_size == 64 and N % 2 == 0 and K % 64 == 0 and N > 0 and K > 0


def w3s_pack(W_q: Tensor, N: int, K: int) -> Tensor:
    """The reference's 3-bit container ([ceil(N K / 640), 64] int32, BitPack.pack_3bit_32) -> the stream layout [N/2, K/16 * 3] int32 that the
    decode / GEMM kernels read with OPT_W3S (hqq_hip_w3s_pack).  What HQQLinearHIP does once when a 3-bit layer is patched — the
    re-layout step of the reference's optimised backends (hqq/backends/torchao.py:202-241, marlin.py:74-123)."""
    _dev(W_q)
    if W_q.dtype != torch.int32 or W_q.numel() != ((N * K // 64 + 9) // 10) * 64:
        raise ValueError(f"hqq_amd: w3s_pack takes the [ceil(N K / 640), 64] int32 container of a {N} x {K} layer")
    out = torch.empty((N // 2, K // 16 * 3), dtype=torch.int32, device=W_q.device)
    with torch.cuda.device(W_q.device):
        rc = _C.lib().hqq_hip_w3s_pack(_p(W_q.contiguous()), _p(out), int(N), int(K), _stream())
    _C.check(rc, "hqq_hip_w3s_pack")
    return out


def w3s_unpack(w3s: Tensor, N: int, K: int) -> Tensor:
    """stream layout -> the reference's container, bit for bit (zero padding rows included): state_dict() / dequantize() of a patched layer"""
    _dev(w3s)
    if w3s.dtype != torch.int32 or w3s.numel() != (N // 2) * (K // 16) * 3:
        raise ValueError(f"hqq_amd: w3s_unpack takes the [N/2, K/16 * 3] int32 stream layout of a {N} x {K} layer")
    out = torch.empty(((N * K // 64 + 9) // 10, 64), dtype=torch.int32, device=w3s.device)
    with torch.cuda.device(w3s.device):
        rc = _C.lib().hqq_hip_w3s_unpack(_p(w3s.contiguous()), _p(out), int(N), int(K), _stream())
    _C.check(rc, "hqq_hip_w3s_unpack")
    return out


def w3s_meta_scalable(scale: Tensor, zero: Tensor, N: int, K: int) -> bool:
    """meta_scalable() for a layer in the 3-bit stream layout (hqq_hip_w3s_meta_check): OPT_META_SCALABLE may accompany OPT_W3S then.  Synchronises."""
    _dev(scale, zero)
    if scale.dtype != torch.float16 or zero.dtype != torch.float16:
        return False
    cnt = torch.empty(1, dtype=torch.int32, device=scale.device)
    with torch.cuda.device(scale.device):
        rc = _C.lib().hqq_hip_w3s_meta_check(_p(scale.contiguous()), _p(zero.contiguous()), int(N), int(K), _p(cnt), _stream())
    _C.check(rc, "hqq_hip_w3s_meta_check")
    return int(cnt.item()) == 0


def packed_rows(nbits: int, rows: int) -> int:
    r = _C.lib().hqq_hip_packed_rows(int(nbits), int(rows))
    if r < 0:
        raise ValueError(f"hqq_amd: {rows} rows cannot be packed at {nbits} bits (rows must divide by {PER.get(nbits)})")
    return int(r)


def pack(nbits: int, W_q: Tensor) -> Tensor:
    """BitPack.pack_{8,4,2,1}bit_u8 / pack_3bit_32 (hqq/core/bitpack.py).  W_q: [rows, cols] integer levels
    (uint8, or float32 as produced by the reference solver)."""
    _dev(W_q)
    if W_q.dtype not in (torch.uint8, torch.float32):
        W_q = W_q.to(torch.uint8)
    W_q = W_q.contiguous()
    rows, cols = W_q.shape
    out = torch.empty((packed_rows(nbits, rows), cols), dtype=torch.int32 if nbits == 3 else torch.uint8, device=W_q.device)
    with torch.cuda.device(W_q.device):
        rc = _C.lib().hqq_hip_pack(nbits, _p(W_q), _dt(W_q.dtype), rows, cols, _p(out), _stream())
    _C.check(rc, "hqq_hip_pack")
    return out


def unpack(nbits: int, W_q: Tensor, dtype: torch.dtype = torch.uint8) -> Tensor:
    """BitPack.unpack_*(W_q, dtype) — returns [per*packed_rows, cols] (3-bit: including the padding rows)."""
    _dev(W_q)
    W_q = W_q.contiguous()
    prow, cols = W_q.shape
    out = torch.empty((PER[nbits] * prow, cols), dtype=dtype, device=W_q.device)
    with torch.cuda.device(W_q.device):
        rc = _C.lib().hqq_hip_unpack(nbits, _p(W_q), prow, cols, _p(out), _dt(dtype), _stream())
    _C.check(rc, "hqq_hip_unpack")
    return out


def dequantize(W_q: Tensor, scale: Tensor, zero: Tensor, N: int, K: int, group_size: int, nbits: int, axis: int = 1) -> Tensor:
    """Quantizer.dequantize / hqq_aten.dequantize: [N,K] in scale.dtype, bit-identical to the reference."""
    _dev(W_q, scale, zero)
    if scale.dtype != zero.dtype:
        raise TypeError("hqq_amd: scale and zero must share the compute dtype")
    groups = (N * K) // int(group_size)
    if scale.numel() != groups or zero.numel() != groups:   # the kernel reads N * K / group_size constants through raw pointers
        raise ValueError(f"hqq_amd: dequantize needs {groups} scale / zero values (N * K / group_size), got {scale.numel()} / {zero.numel()}")
    out = torch.empty((N, K), dtype=scale.dtype, device=W_q.device)
    with torch.cuda.device(W_q.device):
        rc = _C.lib().hqq_hip_dequantize(nbits, _p(W_q.contiguous()), _p(scale.contiguous()), _p(zero.contiguous()), _p(out),
                                         N, K, group_size, axis, _dt(scale.dtype), _stream())
    _C.check(rc, "hqq_hip_dequantize")
    return out


def _fwd(fn_name: str, x: Tensor, W_q: Tensor, scale: Tensor, zero: Tensor, bias, N: int, K: int, group_size: int, nbits: int,
         out: Tensor | None = None, opts=None) -> Tensor:
    _dev(x, W_q, scale, zero, bias)
    if x.dtype != scale.dtype or zero.dtype != scale.dtype or (bias is not None and bias.dtype != scale.dtype):
        raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
    if x.shape[-1] != K:
        raise ValueError(f"hqq_amd: x has {x.shape[-1]} features, layer expects {K}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if M > 0:
        o = _opts(opts)
        with torch.cuda.device(x.device):
            if fn_name == "hqq_hip_gemv":
                ws, ws_bytes = _workspace(x, nbits, [N], M, K, group_size, o)
            else:   # hqq_hip_gemm / hqq_hip_forward
                need = int(getattr(_C.lib(), fn_name + "_workspace_bytes")(int(nbits), M, N, K, group_size, _dt(x.dtype), o))
                ws = reserve_workspace(x.device, need) if need else None
                ws, ws_bytes = (ws.data_ptr(), ws.numel()) if need else (None, 0)
            rc = getattr(_C.lib(), fn_name)(nbits, _p(x2), _p(W_q), _p(scale), _p(zero), _p(bias), _p(out), M, N, K, group_size,
                                            _dt(x.dtype), o, ws, ws_bytes, _stream())
        _C.check(rc, fn_name)
    return out.reshape(*x.shape[:-1], N)


def gemv(x, W_q, scale, zero, bias, N, K, group_size, nbits, out=None, opts=None) -> Tensor:
    """fused unpack->dequant->GEMV for decode-sized batches: the routes of hqq_hip_gemv (route() in DECODE_ROUTES; include/hqq_hip.h)."""
    return _fwd("hqq_hip_gemv", x, W_q, scale, zero, bias, N, K, group_size, nbits, out, opts)


def gemv_grouped(x: Tensor, layers, K: int, group_size: int, nbits: int, outs=None, opts=None):
    """Horizontal fusion: one launch for up to GEMV_MAX_GROUP layers that consume the same x (q/k/v, gate/up, ...).
    layers: sequence of (W_q, scale, zero, bias_or_None, N).  Returns the list of outputs [*, N_i]."""
    n = len(layers)
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise ValueError(f"hqq_amd: a GEMV group holds 1..{GEMV_MAX_GROUP} layers, got {n}")
    if x.shape[-1] != K:
        raise ValueError(f"hqq_amd: x has {x.shape[-1]} features, layers expect {K}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    for (W_q, s, z, b, N) in layers:
        _dev(x, W_q, s, z, b)
        if x.dtype != s.dtype or z.dtype != s.dtype or (b is not None and b.dtype != s.dtype):
            raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
    if outs is None:
        outs = [torch.empty((M, L[4]), dtype=x.dtype, device=x.device) for L in layers]
    if M > 0:
        VP = ctypes.c_void_p * n
        has_bias = any(L[3] is not None for L in layers)
        o = _opts(opts)
        with torch.cuda.device(x.device):
            ws, ws_bytes = _workspace(x, nbits, [L[4] for L in layers], M, K, group_size, o)
            rc = _C.lib().hqq_hip_gemv_grouped(
                nbits, n, _p(x2), VP(*[_p(L[0]) for L in layers]), VP(*[_p(L[1]) for L in layers]), VP(*[_p(L[2]) for L in layers]),
                VP(*[_p(L[3]) for L in layers]) if has_bias else None, VP(*[_p(o_) for o_ in outs]),
                (ctypes.c_int64 * n)(*[int(L[4]) for L in layers]), M, K, group_size, _dt(x.dtype), o, ws, ws_bytes, _stream())
        _C.check(rc, "hqq_hip_gemv_grouped")
    return [o.reshape(*x.shape[:-1], L[4]) for o, L in zip(outs, layers)]


def gemm_grouped_covers(dtype, layers_N, M: int, K: int, group_size, nbits: int, opts=None) -> bool:
    """True when hqq_hip_gemm_grouped serves this group: every layer on the pipelined fused GEMM (ROUTE_GEMM_PIPE)"""
    n = len(layers_N)
    if dtype not in _DT or not 1 <= n <= GEMV_MAX_GROUP or M < 1 or not group_size:
        return False
    return bool(_C.lib().hqq_hip_gemm_grouped_covers(int(nbits), n, (ctypes.c_int64 * n)(*[int(v) for v in layers_N]), int(M), int(K), int(group_size), _dt(dtype), _opts(opts)))


def gemm_grouped(x: Tensor, layers, K: int, group_size: int, nbits: int, outs=None, opts=None):
    """Horizontal fusion beyond the decode rows: ONE launch of the pipelined fused GEMM (+ one split-K reduce) for up to GEMV_MAX_GROUP layers that consume
    the same x (q / k / v, gate / up) — a decoder block at 65..2560 rows is 4 launches instead of 7.  layers: sequence of (W_q, scale, zero, bias_or_None, N).
    Returns the list of outputs [*, N_i].  The K split is chosen for the group's total width: a row can differ in the last bit from the layer launched alone."""
    n = len(layers)
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise ValueError(f"hqq_amd: a GEMM group holds 1..{GEMV_MAX_GROUP} layers, got {n}")
    if x.shape[-1] != K:
        raise ValueError(f"hqq_amd: x has {x.shape[-1]} features, layers expect {K}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    for (W_q, s, z, b, N) in layers:
        _dev(x, W_q, s, z, b)
        if x.dtype != s.dtype or z.dtype != s.dtype or (b is not None and b.dtype != s.dtype):
            raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
    if outs is None:
        outs = [torch.empty((M, L[4]), dtype=x.dtype, device=x.device) for L in layers]
    if M > 0:
        VP = ctypes.c_void_p * n
        has_bias = any(L[3] is not None for L in layers)
        o = _opts(opts)
        Ns = (ctypes.c_int64 * n)(*[int(L[4]) for L in layers])
        with torch.cuda.device(x.device):
            need = int(_C.lib().hqq_hip_gemm_grouped_workspace_bytes(int(nbits), n, Ns, int(M), int(K), int(group_size), _dt(x.dtype), o))
            ws, ws_bytes = (None, 0)
            if need:
                w = reserve_workspace(x.device, need)
                ws, ws_bytes = w.data_ptr(), w.numel()
            rc = _C.lib().hqq_hip_gemm_grouped(
                nbits, n, _p(x2), VP(*[_p(L[0]) for L in layers]), VP(*[_p(L[1]) for L in layers]), VP(*[_p(L[2]) for L in layers]),
                VP(*[_p(L[3]) for L in layers]) if has_bias else None, VP(*[_p(o_) for o_ in outs]), Ns, M, K, group_size, _dt(x.dtype), o, ws, ws_bytes, _stream())
        _C.check(rc, "hqq_hip_gemm_grouped")
    return [o_.reshape(*x.shape[:-1], L[4]) for o_, L in zip(outs, layers)]


BLOCK_NORM, BLOCK_RESID, BLOCK_SILU = 1, 2, 4   # HQQ_BLOCK_* (include/hqq_hip.h)


def block_covers(dtype, K: int, group_size, nbits: int, w3s: bool, norm: bool) -> bool:
    """what hqq_hip_gemv_block serves: one activation row, fp16 / bf16, 4- / 2-bit or the 3-bit stream layout, group_size 64; K <= 8192 with the RMSNorm prologue"""
    return (dtype in (torch.float16, torch.bfloat16) and group_size == 64 and K % 64 == 0 and (nbits in (4, 2) or (nbits == 3 and w3s))
            and (not norm or K <= 8192) and K * 2 <= 144 * 1024 - 4096)


BLOCK_ROPE = 8


def gemv_block(x: Tensor, norm_weight, eps: float, layers, K: int, group_size: int, nbits: int, outs, flags: int, opts=None, rope=None):
    """The decoder block's launches with the glue folded in (csrc/gemv_block.hip; include/hqq_hip.h hqq_hip_gemv_block), ONE activation row:
      BLOCK_NORM               x = the residual stream; layers (W_q, scale, zero, N) like gemv_grouped's; outs[i] [1, N_i]
      BLOCK_NORM | BLOCK_SILU  ONE layer from pair_layers(gate, up): outs[0] [1, N / 2] = silu(gate) * up
      BLOCK_RESID              ONE layer; outs[0] is the residual stream, updated in place: h += layer(x)
      BLOCK_NORM | BLOCK_ROPE  q | k | v with q and k from rotary_pair_layout(): outs = [q_out [n_heads, hd], k_cache, v_cache [n_kv, L, hd]];
                               rope = (cos [hd], sin [hd], pos [1] int64 on the device, head_dim, cache_len): rope_cache() in the launch's epilogue"""
    n = len(layers)
    rp = None
    if flags & BLOCK_ROPE:
        class _Rope(ctypes.Structure):
            _fields_ = [("cos", ctypes.c_void_p), ("sin", ctypes.c_void_p), ("pos", ctypes.c_void_p), ("head_dim", ctypes.c_int64), ("cache_len", ctypes.c_int64)]
        cos, sin, pos, hd, L = rope
        _dev(cos, sin, pos)
        if cos.numel() != hd or sin.numel() != hd or pos.dtype != torch.int64 or cos.dtype != x.dtype or sin.dtype != x.dtype:
            raise ValueError("hqq_amd: rope = (cos [head_dim], sin [head_dim] in the compute dtype, pos int64 on the device, head_dim, cache_len)")
        if outs[1].shape[-1] != hd or outs[1].shape[-2] != L or outs[1].shape != outs[2].shape or not (outs[1].is_contiguous() and outs[2].is_contiguous()):
            raise ValueError("hqq_amd: the caches must be contiguous [n_kv_heads, cache_len, head_dim] tensors")
        rp = ctypes.byref(_Rope(_p(cos), _p(sin), _p(pos), int(hd), int(L)))
    _dev(x, norm_weight, *[t for L in layers for t in L[:3]], *outs)
    if x.numel() != K:
        raise ValueError(f"hqq_amd: gemv_block serves one activation row of {K} features, got {tuple(x.shape)}")
    VP = ctypes.c_void_p * n
    o = _opts(opts)
    with torch.cuda.device(x.device):
        rc = _C.lib().hqq_hip_gemv_block(int(nbits), n, _p(x), _p(norm_weight), float(eps), VP(*[_p(L[0]) for L in layers]), VP(*[_p(L[1]) for L in layers]),
                                         VP(*[_p(L[2]) for L in layers]), VP(*[_p(t) for t in outs]), (ctypes.c_int64 * n)(*[int(L[-1]) for L in layers]),
                                         int(K), int(group_size), _dt(x.dtype), o, int(flags), rp, _stream())
    _C.check(rc, "hqq_hip_gemv_block")
    return outs


def pair_layers(gate, up, K: int, group_size: int, nbits: int, w3s: bool = False):
    """The PAIRED layout of two layers of equal shape that read the same input (LlamaMLP's gate_proj / up_proj): the level matrix of `gate` on top of
    the level matrix of `up`, packed as ONE layer of 2 N rows — BitPack's row slabs then put gate row n and up row n into the same packed row
    (4-bit: byte (n, k) = gate level << 4 | up level), which is what lets hqq_hip_gemv_block's epilogue form silu(gate[n]) * up[n] inside one wave.
    gate / up: (W_q, scale, zero, N) as the layers hold them (3-bit: the stream layout when w3s).  Returns (W_q, scale, zero, 2 N); the originals are
    untouched (state_dict() and the prefill path keep using them).  Levels, scale and zero are the layers' own: the same weights bit for bit."""
    (Wg, sg, zg, N), (Wu, su, zu, Nu) = gate, up
    if N != Nu or sg.dtype != su.dtype:
        raise ValueError("hqq_amd: pair_layers needs two layers of the same shape and compute dtype")
    if w3s:
        Wg, Wu = w3s_unpack(Wg, N, K), w3s_unpack(Wu, N, K)
    R = N * K // group_size
    Ug = unpack(nbits, Wg)[:R]          # level matrix [N K / gs, gs], row (n, g)
    Uu = unpack(nbits, Wu)[:R]
    W = pack(nbits, torch.cat([Ug, Uu], dim=0))
    if w3s:
        W = w3s_pack(W, 2 * N, K)
    return W, torch.cat([sg.reshape(-1), su.reshape(-1)]).contiguous(), torch.cat([zg.reshape(-1), zu.reshape(-1)]).contiguous(), 2 * N


def merge_layers(layers, K: int, group_size: int, nbits: int, w3s: bool = False):
    """ONE layer whose rows are the rows of `layers` in order (q_proj | k_proj | v_proj, gate_proj | up_proj: layers that read the same input): the
    level matrices stacked and packed again, scale / zero concatenated — the same levels and constants bit for bit, so y of the merged layer is the
    concatenation of the layers' outputs.  What it buys: one launch over sum(N) rows instead of one per layer (at 65..2560 activation rows, where
    hqq_hip_gemv_grouped does not reach: a 12288 x 4096 launch at 128 rows takes 29-31 us against 3 x 19-20).
    layers: (W_q, scale, zero, N) as the layers hold them (3-bit: the stream layout when w3s).  Returns (W_q, scale, zero, sum N); the originals are
    untouched.  (The reference has no such helper; vLLM's merged q|k|v / gate|up modules are the same idea: hqq/utils/vllm.py.)"""
    if not layers:
        raise ValueError("hqq_amd: merge_layers needs at least one layer")
    dt = layers[0][1].dtype
    U = []
    for W, s, z, N in layers:
        if s.dtype != dt or z.dtype != dt:
            raise ValueError("hqq_amd: merge_layers needs one compute dtype")
        if (N * K) % group_size or s.numel() != N * K // group_size or z.numel() != s.numel():
            raise ValueError("hqq_amd: merge_layers takes channel-wise layers quantised along axis 1 (one scale / zero per group of a row)")
        if w3s:
            W = w3s_unpack(W, N, K)
        U.append(unpack(nbits, W)[:N * K // group_size])   # level matrix [N K / gs, gs], row (n, g)
    Nt = sum(int(l[3]) for l in layers)
    Wm = pack(nbits, torch.cat(U, dim=0))
    if w3s:
        Wm = w3s_pack(Wm, Nt, K)
    return (Wm, torch.cat([l[1].reshape(-1) for l in layers]).contiguous(), torch.cat([l[2].reshape(-1) for l in layers]).contiguous(), Nt)


def rotary_pair_layout(layer, K: int, group_size: int, nbits: int, head_dim: int, w3s: bool = False):
    """The ROTARY-PAIRED row order of a q_proj / k_proj layer: element i < head_dim / 2 of head h becomes row h head_dim / 2 + i, its rotary partner
    i + head_dim / 2 row N / 2 + h head_dim / 2 + i — so that BitPack's row slabs hold both in ONE packed row and hqq_hip_gemv_block's epilogue can apply
    apply_rotary_pos_emb inside the wave that finishes the row (its outputs are written back in the natural order).  layer: (W_q, scale, zero, N) as the
    layer holds it; returns a permuted copy (the original is untouched: state_dict() and the prefill path keep using it).  Same levels, scale, zero per row."""
    W, s, z, N = layer
    if N % head_dim or head_dim % 2:
        raise ValueError("hqq_amd: rotary_pair_layout needs whole heads of an even size")
    G = K // group_size
    if w3s:
        W = w3s_unpack(W, N, K)
    rows = torch.arange(N, device=s.device).view(N // head_dim, head_dim)
    perm = torch.cat([rows[:, :head_dim // 2].reshape(-1), rows[:, head_dim // 2:].reshape(-1)])
    U = unpack(nbits, W)[:N * G].reshape(N, G * group_size).index_select(0, perm).reshape(N * G, group_size).contiguous()
    Wp = pack(nbits, U)
    if w3s:
        Wp = w3s_pack(Wp, N, K)
    return Wp, s.reshape(N, G).index_select(0, perm).reshape(-1).contiguous(), z.reshape(N, G).index_select(0, perm).reshape(-1).contiguous(), N


EXCHANGE_MAX_RANKS = 16
EXCHANGE_MAX_ROWS = 64


def exchange(y_loc, N_loc, nbits: int, world: int, rank: int, full_ptrs, flag_ptrs, status_ptr: int, spin_limit: int = 0) -> None:
    """One exchange point of a column-sharded decode step (csrc/exchange.hip, hqq_hip_exchange): this rank's [1, N_loc[j]] slices go
    straight into every rank's full row of layer j, in the reference's column order; returns when enqueued (the kernel finishes once all
    `world` ranks have delivered).  full_ptrs[p][j] / flag_ptrs[p]: raw device addresses (see hqq_amd.shard.PeerExchange, which owns them)."""
    n = len(y_loc)
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise ValueError(f"hqq_amd: an exchange point holds 1..{GEMV_MAX_GROUP} layers, got {n}")
    if not 1 <= world <= EXCHANGE_MAX_RANKS or len(full_ptrs) != world or len(flag_ptrs) != world:
        raise ValueError(f"hqq_amd: 1..{EXCHANGE_MAX_RANKS} ranks, one row set and one flag block per rank")
    M = y_loc[0].numel() // int(N_loc[0])
    if not 1 <= M <= EXCHANGE_MAX_ROWS:
        raise ValueError(f"hqq_amd: exchange takes 1..{EXCHANGE_MAX_ROWS} activation rows")
    for t, nl in zip(y_loc, N_loc):
        _dev(t)
        if t.numel() != M * nl or not t.is_contiguous() or t.element_size() != 2:
            raise ValueError("hqq_amd: exchange takes dense 2-byte activations, the same number of rows for every layer: y_loc[j] is [M, N_loc[j]]")
    dt = _dt(y_loc[0].dtype)
    VPn = ctypes.c_void_p * n
    VPf = ctypes.c_void_p * (world * n)
    VPw = ctypes.c_void_p * world
    with torch.cuda.device(y_loc[0].device):
        rc = _C.lib().hqq_hip_exchange(n, VPn(*[_p(t) for t in y_loc]), (ctypes.c_int64 * n)(*[int(v) for v in N_loc]), int(M), int(nbits), dt, int(world), int(rank),
                                       VPf(*[int(full_ptrs[p][j]) for p in range(world) for j in range(n)]), VPw(*[int(v) for v in flag_ptrs]),
                                       ctypes.c_void_p(int(status_ptr)), int(spin_limit), _stream())
    _C.check(rc, "hqq_hip_exchange")


def gemm(x, W_q, scale, zero, bias, N, K, group_size, nbits, out=None, opts=None) -> Tensor:
    """fused unpack->dequant->MFMA GEMM (prefill)."""
    return _fwd("hqq_hip_gemm", x, W_q, scale, zero, bias, N, K, group_size, nbits, out, opts)


# Which path `forward` takes by the number of activation rows M (measured on MI355X, tools/prefill_routes.py -> profiles/r04_prefill_routes_int4.txt):
#   the decode routes (route() in DECODE_ROUTES): the weight-streaming decode kernels;
#   beyond, where hqq_hip_forward_prefers_fused says so (to 2560 rows): the pipelined split-K fused MFMA dequant-GEMM (gemm_pipe.hip);
#   else: the HIP dequantise kernel + the in-tree dense MFMA GEMM (hqq_hip_gemm_dense, gemm_dense.hip) — one extra write + read of the
#       fp16 weights (11-36 us), then the weights are rebuilt once, not once per 256-token tile: 1.0-1.2 PFLOP/s at M = 8192 against
#       0.87-0.95 for the fused kernel.  No library GEMM on any product path (`library_gemm=True` is the bench's comparison leg).
# `fused=True` forces the fused kernels for every M.  LIBRARY_GEMM_MIN_M (a historical name: the composition's GEMM is the in-tree one) applies to
# the decode-sized cases the skinny kernel does not cover.
LIBRARY_GEMM_MIN_M = 17


def skinny_covers(dtype, M, N, K, group_size, nbits, w3s: bool = False) -> bool:
    """a batch that the weight-streaming skinny-GEMM kernel serves (ROUTE_SKINNY); 3-bit layers in the stream layout only (w3s=True)"""
    return route(dtype, M, (N,), K, group_size, nbits, OPT_W3S if w3s else 0) == ROUTE_SKINNY


def decode_covers(dtype, M, N, K, group_size, nbits) -> bool:
    """what hqq_hip_gemv serves for M <= GEMV_MAX_M rows with exact weights; everything else is composed in `forward`.  (bf16 batches of 5..16 rows
    exist only on the skinny route: skinny_covers() reports those.)"""
    r = route(dtype, M, (N,), K, group_size, nbits)
    return M <= GEMV_MAX_M and r in DECODE_ROUTES and not (r == ROUTE_SKINNY and dtype == torch.bfloat16)


def decode_axis0_covers(dtype, M, N, K, group_size, nbits) -> bool:
    """what hqq_hip_gemv_axis0 serves: a layer quantised along axis 0 (group_size None: one group per column, i.e. group_size = N), fp16 at
    8 / 4 / 2 / 1 bits or bf16 at 4 / 2 bits, group_size % 16 == 0 dividing N, K % 64 == 0, 1 <= M <= GEMV_MAX_M"""
    gs = N if group_size is None else int(group_size)
    if not (1 <= M <= GEMV_MAX_M) or N <= 0 or K <= 0 or gs <= 0 or gs % 16 or N % gs or K % 64:
        return False
    if dtype == torch.float16:
        return nbits in (8, 4, 2, 1)
    return dtype == torch.bfloat16 and nbits in (4, 2)


def gemv_axis0(x: Tensor, W_q: Tensor, scale: Tensor, zero: Tensor, bias, N: int, K: int, group_size, nbits: int, out: Tensor | None = None,
               opts=None) -> Tensor:
    """y = x @ dequantize(W_q, axis=0)^T (+ bias) for x [*, K] of 1..GEMV_MAX_M rows (hqq_hip_gemv_axis0): W_q the reference's axis-0 container,
    scale / zero its [1, N * K / group_size] meta (any shape, read flat); group_size None = N.  Raises NotImplementedError outside
    decode_axis0_covers()."""
    _dev(x, W_q, scale, zero, bias)
    if x.dtype != scale.dtype or zero.dtype != scale.dtype or (bias is not None and bias.dtype != scale.dtype):
        raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
    if x.shape[-1] != K:
        raise ValueError(f"hqq_amd: x has {x.shape[-1]} features, layer expects {K}")
    gs = N if group_size is None else int(group_size)
    if scale.numel() != (N * K) // gs or zero.numel() != (N * K) // gs:
        raise ValueError(f"hqq_amd: gemv_axis0 needs {(N * K) // gs} scale / zero values (N * K / group_size), got {scale.numel()} / {zero.numel()}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if M > 0:
        L = _C.lib()
        with torch.cuda.device(x.device):
            need = int(L.hqq_hip_gemv_axis0_workspace_bytes(int(nbits), M, int(N), int(K), gs, _dt(x.dtype)))
            ws = reserve_workspace(x.device, need) if need else None
            rc = L.hqq_hip_gemv_axis0(int(nbits), _p(x2), _p(W_q.contiguous()), _p(scale.contiguous()), _p(zero.contiguous()), _p(bias), _p(out),
                                      M, int(N), int(K), gs, _dt(x.dtype), _opts(opts), _p(ws), 0 if ws is None else ws.numel(), _stream())
        _C.check(rc, "hqq_hip_gemv_axis0")
    return out.reshape(*x.shape[:-1], N)


AXIS0_MAX_GROUP = 3   # layers per hqq_hip_gemv_axis0_grouped call


def axis0_grouped_covers(dtype, M, Ns, K, group_size, nbits, flags: int = 0) -> bool:
    """what hqq_hip_gemv_axis0_grouped serves: 1..AXIS0_MAX_GROUP layers, each one decode_axis0_covers() takes at M rows (group_size None is
    the one-group-per-column setting and needs every N equal, since the group shares one group_size); flags 0, or BLOCK_SILU on two layers
    of equal N"""
    Ns = tuple(int(n) for n in Ns)
    if not 1 <= len(Ns) <= AXIS0_MAX_GROUP:
        return False
    if group_size is None:
        if len(set(Ns)) != 1:
            return False
        group_size = Ns[0]
    if not all(decode_axis0_covers(dtype, M, N, K, group_size, nbits) for N in Ns):
        return False
    flags = int(flags)
    if flags & ~BLOCK_SILU:
        return False
    return not (flags & BLOCK_SILU) or (len(Ns) == 2 and Ns[0] == Ns[1])


def gemv_axis0_grouped(x: Tensor, layers, K: int, group_size, nbits: int, outs=None, flags: int = 0):
    """gemv_axis0 for up to AXIS0_MAX_GROUP axis-0 layers that consume the same x [*, K] of 1..GEMV_MAX_M rows, in one launch + one reduce
    (hqq_hip_gemv_axis0_grouped).  layers: sequence of (W_q, scale, zero, bias_or_None, N), sharing group_size (None = N, all N equal) and
    nbits.  Returns the list of outputs [*, N_i], each the bits gemv_axis0 gives for that layer.  flags=BLOCK_SILU (layers = gate, up of
    equal N): ONE output, silu_mul(gate's output, up's output) bit for bit.  Raises NotImplementedError outside axis0_grouped_covers()."""
    n = len(layers)
    if not 1 <= n <= AXIS0_MAX_GROUP:
        raise ValueError(f"hqq_amd: an axis-0 GEMV group holds 1..{AXIS0_MAX_GROUP} layers, got {n}")
    if x.shape[-1] != K:
        raise ValueError(f"hqq_amd: x has {x.shape[-1]} features, layers expect {K}")
    Ns = [int(L[4]) for L in layers]
    if group_size is None and len(set(Ns)) != 1:
        raise ValueError("hqq_amd: group_size None (one group per column) needs layers of equal N in one group")
    gs = Ns[0] if group_size is None else int(group_size)
    for (W_q, s, z, b, N) in layers:
        _dev(x, W_q, s, z, b)
        if x.dtype != s.dtype or z.dtype != s.dtype or (b is not None and b.dtype != s.dtype):
            raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
        if s.numel() != (N * K) // gs or z.numel() != (N * K) // gs:
            raise ValueError(f"hqq_amd: gemv_axis0_grouped needs {(N * K) // gs} scale / zero values per layer (N * K / group_size), got {s.numel()} / {z.numel()}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    flags = int(flags)
    out_Ns = Ns[:1] if flags & BLOCK_SILU else Ns
    if outs is None:
        outs = [torch.empty((M, N), dtype=x.dtype, device=x.device) for N in out_Ns]
    if len(outs) != len(out_Ns) or any(o.numel() != M * N or o.dtype != x.dtype or not o.is_contiguous() for o, N in zip(outs, out_Ns)):
        raise ValueError(f"hqq_amd: gemv_axis0_grouped writes {len(out_Ns)} dense outputs of {M} x {out_Ns} elements in x's dtype")
    if M > 0:
        L = _C.lib()
        VP = ctypes.c_void_p * n
        Nc = (ctypes.c_int64 * n)(*Ns)
        has_bias = any(Lr[3] is not None for Lr in layers)
        keep = [[t.contiguous() for t in Lr[:3]] for Lr in layers]   # (alive until the launch is enqueued)
        with torch.cuda.device(x.device):
            need = int(L.hqq_hip_gemv_axis0_grouped_workspace_bytes(int(nbits), n, Nc, M, int(K), gs, _dt(x.dtype), flags))
            ws = reserve_workspace(x.device, need) if need else None
            rc = L.hqq_hip_gemv_axis0_grouped(
                int(nbits), n, _p(x2), VP(*[_p(k[0]) for k in keep]), VP(*[_p(k[1]) for k in keep]), VP(*[_p(k[2]) for k in keep]),
                VP(*[_p(Lr[3]) for Lr in layers]) if has_bias else None, VP(*([_p(o) for o in outs] + [None] * (n - len(outs)))), Nc,
                M, int(K), gs, _dt(x.dtype), 0, flags, _p(ws), 0 if ws is None else ws.numel(), _stream())
        _C.check(rc, "hqq_hip_gemv_axis0_grouped")
    return [o.reshape(*x.shape[:-1], N) for o, N in zip(outs, out_Ns)]


GEMM_AXIS0_MAX_M = 256   # HQQ_GEMM_AXIS0_MAX_M
# the last row count at which `forward(axis=0)` takes hqq_hip_gemm_axis0 by default: the largest M of tools/axis0_gemm_bench.py at which the kernel is at
# least 10 % ahead of dequantise + torch.matmul on every measured shape.  profiles/axis0_gemm_summary.md: 1.38x to 5.9x ahead at 17 / 32 / 64 / 128 rows on
# every shape; at 256 rows ahead on the int4 shapes but 0.72x on int2 bf16 4096 x 4096, so the route ends at 128.  (16 would mean "opt-in only".)
AXIS0_GEMM_ROUTE_MAX_M = 128


@functools.lru_cache(maxsize=4096)
def gemm_axis0_covers(dtype, M, N, K, group_size, nbits) -> bool:
    """what hqq_hip_gemm_axis0 serves: the layers of decode_axis0_covers() at GEMV_MAX_M < M <= GEMM_AXIS0_MAX_M rows whose offsets the library accepts —
    its workspace query is 0 exactly where the call refuses, so the answer is the library's (32-bit offset guards included)"""
    if not (GEMV_MAX_M < M <= GEMM_AXIS0_MAX_M and decode_axis0_covers(dtype, 1, N, K, group_size, nbits)):
        return False
    gs = N if group_size is None else int(group_size)
    return int(_C.lib().hqq_hip_gemm_axis0_workspace_bytes(int(nbits), int(M), int(N), int(K), gs, _DT[dtype])) > 0


def gemm_axis0(x: Tensor, W_q: Tensor, scale: Tensor, zero: Tensor, bias, N: int, K: int, group_size, nbits: int, out: Tensor | None = None,
               opts=None) -> Tensor:
    """y = x @ dequantize(W_q, axis=0)^T (+ bias) for x [*, K] of GEMV_MAX_M + 1 .. GEMM_AXIS0_MAX_M rows (hqq_hip_gemm_axis0): arguments as gemv_axis0.
    Raises NotImplementedError outside gemm_axis0_covers()."""
    _dev(x, W_q, scale, zero, bias)
    if x.dtype != scale.dtype or zero.dtype != scale.dtype or (bias is not None and bias.dtype != scale.dtype):
        raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
    if x.shape[-1] != K:
        raise ValueError(f"hqq_amd: x has {x.shape[-1]} features, layer expects {K}")
    gs = N if group_size is None else int(group_size)
    if scale.numel() != (N * K) // gs or zero.numel() != (N * K) // gs:
        raise ValueError(f"hqq_amd: gemm_axis0 needs {(N * K) // gs} scale / zero values (N * K / group_size), got {scale.numel()} / {zero.numel()}")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    elif out.numel() != M * N or out.dtype != x.dtype or not out.is_contiguous():
        raise ValueError(f"hqq_amd: gemm_axis0 writes a dense output of {M} x {N} elements in x's dtype")
    L = _C.lib()
    with torch.cuda.device(x.device):
        need = int(L.hqq_hip_gemm_axis0_workspace_bytes(int(nbits), M, int(N), int(K), gs, _dt(x.dtype)))
        ws = reserve_workspace(x.device, need) if need else None
        rc = L.hqq_hip_gemm_axis0(int(nbits), _p(x2), _p(W_q.contiguous()), _p(scale.contiguous()), _p(zero.contiguous()), _p(bias), _p(out),
                                  M, int(N), int(K), gs, _dt(x.dtype), _opts(opts), _p(ws), 0 if ws is None else ws.numel(), _stream())
    _C.check(rc, "hqq_hip_gemm_axis0")
    return out.reshape(*x.shape[:-1], N)


# The backward of an axis-1 layer with respect to its input, dx = g @ dequantize(W_q) (csrc/gemm_dgrad.hip), against what _MatmulNoCache.backward has always
# run: the HIP dequantise kernel (2 N K bytes written, then read back) + torch.matmul.  HQQLinear._matmul_hip(transpose=False) takes the fused kernel up to
# this many rows of g.  The rule is AXIS0_GEMM_ROUTE_MAX_M's: the largest measured row count at which the fused kernel is at least 10 % ahead on EVERY
# measured shape (tools/dgrad_bench.py; profiles/dgrad_summary.md holds the table: 1.42x to 1.87x ahead at 16 rows on every shape; at 64 rows 1.04x on
# 11008 x 4096, so the route ends at 16; from 1024 rows the composed route is 2x to 3x faster).  0 would mean "opt-in only".
DGRAD_ROUTE_MAX_M = 16


@functools.lru_cache(maxsize=4096)
def gemm_dgrad_covers(dtype, M, N, K, group_size, nbits) -> bool:
    """what hqq_hip_gemm_dgrad serves (the library's own answer, nothing launched): axis-1 byte containers (8 / 4 / 2 bit), fp16 / bf16,
    group_size % 16 == 0 dividing K, K % 64 == 0, N % (8 * per) == 0, M >= 1, sizes within 32-bit offsets"""
    if dtype not in _DT or group_size is None or isinstance(nbits, float) or int(nbits) != nbits:
        return False
    return bool(_C.lib().hqq_hip_gemm_dgrad_covers(int(nbits), int(M), int(N), int(K), int(group_size), _DT[dtype]))


def gemm_dgrad(g: Tensor, W_q: Tensor, scale: Tensor, zero: Tensor, N: int, K: int, group_size, nbits: int, out: Tensor | None = None) -> Tensor:
    """dx = g @ dequantize(W_q, axis=1) for g [*, N] -> [*, K] (hqq_hip_gemm_dgrad): the weights are the bits of dequantize(), accumulation in fp32,
    one rounding; deterministic, on the current stream, no workspace.  `out`: a contiguous buffer of rows x K elements in g's dtype.
    Raises NotImplementedError outside gemm_dgrad_covers()."""
    _dev(g, W_q, scale, zero)
    if g.dtype != scale.dtype or zero.dtype != scale.dtype:
        raise TypeError("hqq_amd: g / scale / zero must share the compute dtype")
    if g.shape[-1] != N:
        raise ValueError(f"hqq_amd: g has {g.shape[-1]} features, layer produces {N}")
    if group_size is None:
        raise NotImplementedError("hqq_amd: gemm_dgrad needs a group size")
    gs = int(group_size)
    if scale.numel() != (N * K) // gs or zero.numel() != (N * K) // gs:
        raise ValueError(f"hqq_amd: gemm_dgrad needs {(N * K) // gs} scale / zero values (N * K / group_size), got {scale.numel()} / {zero.numel()}")
    if W_q.dtype != torch.uint8 or W_q.numel() != (N // PER.get(nbits, 1)) * K:
        raise NotImplementedError(f"hqq_amd: gemm_dgrad reads the byte container [N / per, K] of an axis-1 layer (nbits={nbits})")
    g2 = g.reshape(-1, N)
    if not g2.is_contiguous():
        g2 = g2.contiguous()
    M = g2.shape[0]
    if out is None:
        out = torch.empty((M, K), dtype=g.dtype, device=g.device)
    elif out.numel() != M * K or out.dtype != g.dtype or not out.is_contiguous() or out.device != g.device:
        raise ValueError(f"hqq_amd: gemm_dgrad writes a dense output of {M} x {K} elements in g's dtype")
    with torch.cuda.device(g.device):
        rc = _C.lib().hqq_hip_gemm_dgrad(int(nbits), _p(g2), _p(W_q.contiguous()), _p(scale.contiguous()), _p(zero.contiguous()), _p(out),
                                         M, int(N), int(K), gs, _dt(g.dtype), _stream())
    _C.check(rc, "hqq_hip_gemm_dgrad")
    return out.reshape(*g.shape[:-1], K)


# The same product for a layer quantised along AXIS 0 (csrc/gemm_dgrad_axis0.hip), against ops.dequantize(axis=0) + torch.matmul.
# HQQLinear._matmul_hip(transpose=False) takes the fused kernel up to this many rows of g; the rule is DGRAD_ROUTE_MAX_M's: the largest measured row
# count at which the kernel is at least 10 % ahead on EVERY measured shape (tools/dgrad_axis0_bench.py; profiles/dgrad_axis0_summary.md holds the
# table: ahead on every shape at every measured row count from 1 to 256; at 1024 rows it is within 10 % on 4096 x 11008, so the route ends at 256).
# 0 would mean "opt-in only".  ops.gemm_dgrad_axis0 itself serves any row count.
DGRAD_AXIS0_ROUTE_MAX_M = 256


@functools.lru_cache(maxsize=4096)
def gemm_dgrad_axis0_covers(dtype, M, N, K, group_size, nbits) -> bool:
    """what hqq_hip_gemm_dgrad_axis0 serves (the library's own answer, nothing launched): axis-0 byte containers (8 / 4 / 2 bit), fp16 / bf16,
    group_size % 16 == 0 dividing N (None: one group of N), K % 64 == 0, N % (8 * per) == 0, M >= 1, sizes within 32-bit offsets"""
    if dtype not in _DT or isinstance(nbits, float) or int(nbits) != nbits:
        return False
    gs = int(N) if group_size is None else int(group_size)
    return bool(_C.lib().hqq_hip_gemm_dgrad_axis0_covers(int(nbits), int(M), int(N), int(K), gs, _DT[dtype]))


def gemm_dgrad_axis0(g: Tensor, W_q: Tensor, scale: Tensor, zero: Tensor, N: int, K: int, group_size, nbits: int, out: Tensor | None = None) -> Tensor:
    """dx = g @ dequantize(W_q, axis=0) for g [*, N] -> [*, K] (hqq_hip_gemm_dgrad_axis0): the weights are the bits of dequantize(axis=0), accumulation
    in fp32, one rounding; deterministic, on the current stream, no workspace.  group_size None: one group of N rows.  `out`: a contiguous buffer of
    rows x K elements in g's dtype.  Raises NotImplementedError outside gemm_dgrad_axis0_covers()."""
    _dev(g, W_q, scale, zero)
    if g.dtype != scale.dtype or zero.dtype != scale.dtype:
        raise TypeError("hqq_amd: g / scale / zero must share the compute dtype")
    if g.shape[-1] != N:
        raise ValueError(f"hqq_amd: g has {g.shape[-1]} features, layer produces {N}")
    gs = int(N) if group_size is None else int(group_size)
    if gs < 1 or scale.numel() != (N * K) // gs or zero.numel() != (N * K) // gs:
        raise ValueError(f"hqq_amd: gemm_dgrad_axis0 needs {(N * K) // max(gs, 1)} scale / zero values (N * K / group_size), got {scale.numel()} / {zero.numel()}")
    if W_q.dtype != torch.uint8 or W_q.numel() != (N // PER.get(nbits, 1)) * K:
        raise NotImplementedError(f"hqq_amd: gemm_dgrad_axis0 reads the byte container [N / per, K] of an axis-0 layer (nbits={nbits})")
    g2 = g.reshape(-1, N)
    if not g2.is_contiguous():
        g2 = g2.contiguous()
    M = g2.shape[0]
    if out is None:
        out = torch.empty((M, K), dtype=g.dtype, device=g.device)
    elif out.numel() != M * K or out.dtype != g.dtype or not out.is_contiguous() or out.device != g.device:
        raise ValueError(f"hqq_amd: gemm_dgrad_axis0 writes a dense output of {M} x {K} elements in g's dtype")
    with torch.cuda.device(g.device):
        rc = _C.lib().hqq_hip_gemm_dgrad_axis0(int(nbits), _p(g2), _p(W_q.contiguous()), _p(scale.contiguous()), _p(zero.contiguous()), _p(out),
                                               M, int(N), int(K), gs, _dt(g.dtype), _stream())
    _C.check(rc, "hqq_hip_gemm_dgrad_axis0")
    return out.reshape(*g.shape[:-1], K)


LORA_MERGE_MAX_R = 256


@functools.lru_cache(maxsize=4096)
def lora_merge_covers(dtype, lora_dtype, N, K, group_size, nbits, axis, r) -> bool:
    """what hqq_hip_lora_merge serves (the library's own answer, nothing launched): a compute dtype fp16 / bf16, an adapter in fp32 / fp16 / bf16 of
    rank 1 .. 256, and a base weight that is either packed — every (nbits, axis, group_size, N, K) dequantize() accepts — or dense (nbits = 0;
    group_size and axis are not looked at)"""
    if dtype not in _DT or lora_dtype not in _DT or isinstance(nbits, float) or int(nbits) != nbits:
        return False
    if int(nbits) != 0 and (group_size is None or axis not in (0, 1)):
        return False
    return bool(_C.lib().hqq_hip_lora_merge_covers(int(nbits), int(N), int(K), int(group_size or 0), int(axis or 0), _DT[dtype], _DT[lora_dtype], int(r)))


def _lora_merge(who: str, nbits: int, base: Tensor, scale, zero, N: int, K: int, group_size: int, axis: int, dtype, A: Tensor, B: Tensor, scaling,
                out: Tensor | None) -> Tensor:
    _dev(base, scale, zero, A, B, out)
    if A.dtype != B.dtype:
        raise TypeError(f"hqq_amd: {who}: lora_A and lora_B must share a dtype")
    if A.dim() != 2 or B.dim() != 2 or A.shape[0] != K or B.shape[1] != N or A.shape[1] != B.shape[0]:
        raise ValueError(f"hqq_amd: {who} needs A [K, r] and B [r, N] for a [{N}, {K}] weight, got {tuple(A.shape)} and {tuple(B.shape)}")
    r = A.shape[1]
    if any(t is not None and t.device != base.device for t in (scale, zero, A, B, out)):
        raise ValueError(f"hqq_amd: {who}: every tensor must be on the base weight's device")
    if not lora_merge_covers(dtype, A.dtype, N, K, group_size, nbits, axis, r):
        raise NotImplementedError(f"hqq_amd: {who} is not covered for compute dtype {dtype}, adapter dtype {A.dtype}, rank {r}, nbits {nbits}, "
                                  f"axis {axis}, group_size {group_size}, N {N}, K {K} (fp16 / bf16, rank 1 .. {LORA_MERGE_MAX_R}, what dequantize accepts)")
    if out is None:
        out = torch.empty((N, K), dtype=dtype, device=base.device)
    elif out.numel() != N * K or out.dtype != dtype or not out.is_contiguous():
        raise ValueError(f"hqq_amd: {who} writes a dense output of {N} x {K} elements in the compute dtype")
    with torch.cuda.device(base.device):
        rc = _C.lib().hqq_hip_lora_merge(int(nbits), _p(base.contiguous()), _p(None if scale is None else scale.contiguous()),
                                         _p(None if zero is None else zero.contiguous()), _p(A.contiguous()), _p(B.contiguous()), float(scaling), _p(out),
                                         int(N), int(K), int(group_size), int(axis), _dt(dtype), _dt(A.dtype), int(r), _stream())
    _C.check(rc, "hqq_hip_lora_merge")
    return out.reshape(N, K)


def lora_merge(W_q: Tensor, scale: Tensor, zero: Tensor, N: int, K: int, group_size: int, nbits: int, axis: int, A: Tensor, B: Tensor, scaling: float,
               out: Tensor | None = None) -> Tensor:
    """dequantize(W_q, ...) + ((A @ B) * scaling).t().to(dtype) in one launch (hqq_hip_lora_merge), [N, K] in scale.dtype: the base weight is the bits
    of dequantize(); the rank-r product is an fp32 sum over j = 0 .. r - 1 in that order of separately rounded products, then rounded as the torch
    statements round (adapter dtype, * scaling, adapter dtype, compute dtype, the add).  A [K, r], B [r, N] in fp32 / fp16 / bf16.  Deterministic, on the
    current stream, no workspace.  `out`: a contiguous buffer of N x K elements in scale.dtype.  Raises NotImplementedError outside lora_merge_covers()."""
    _dev(W_q, scale, zero, A, B, out)
    if scale.dtype != zero.dtype:
        raise TypeError("hqq_amd: scale and zero must share the compute dtype")
    if group_size is None:
        raise NotImplementedError("hqq_amd: lora_merge needs a group size")
    if not lora_merge_covers(scale.dtype, A.dtype, N, K, group_size, nbits, axis, A.shape[-1]) or int(nbits) == 0:
        raise NotImplementedError(f"hqq_amd: lora_merge is not covered for compute dtype {scale.dtype}, adapter dtype {A.dtype}, rank {A.shape[-1]}, "
                                  f"nbits {nbits}, axis {axis}, group_size {group_size}, N {N}, K {K}")
    gs = int(group_size)
    groups = (N * K) // gs
    if scale.numel() != groups or zero.numel() != groups:   # the kernel reads N * K / group_size constants through raw pointers
        raise ValueError(f"hqq_amd: lora_merge needs {groups} scale / zero values (N * K / group_size), got {scale.numel()} / {zero.numel()}")
    urows, ucols = (groups, gs) if axis == 1 else (gs, groups)
    want = (torch.int32, packed_rows(nbits, urows) * ucols) if nbits == 3 else (torch.uint8, packed_rows(nbits, urows) * ucols)
    if (W_q.dtype, W_q.numel()) != want:
        raise ValueError(f"hqq_amd: lora_merge reads the reference's container of {want[1]} {want[0]} elements, got {W_q.numel()} of {W_q.dtype}")
    return _lora_merge("lora_merge", nbits, W_q, scale, zero, N, K, gs, axis, scale.dtype, A, B, scaling, out)


def lora_merge_dense(W: Tensor, A: Tensor, B: Tensor, scaling: float, out: Tensor | None = None) -> Tensor:
    """W + ((A @ B) * scaling).t().to(W.dtype) for a dense [N, K] weight in fp16 / bf16, with lora_merge's arithmetic (hqq_hip_lora_merge, dense form).
    W is not modified.  Raises NotImplementedError outside lora_merge_covers(..., nbits=0, ...)."""
    if W.dim() != 2:
        raise ValueError("hqq_amd: lora_merge_dense needs a [N, K] weight")
    N, K = W.shape
    return _lora_merge("lora_merge_dense", 0, W, None, None, N, K, 0, 0, W.dtype, A, B, scaling, out)


# ---- the adapter term of UN-MERGED LoRA layers in the decode step (csrc/lora_decode.hip) ------------------------------------------------------------
LORA_DECODE_MAX_R = 256   # = LORA_MERGE_MAX_R: what can be merged can be decoded un-merged


def _i64s(vals):
    vals = [int(v) for v in vals]
    return (ctypes.c_int64 * max(len(vals), 1))(*vals)


def lora_decode_covers(dtype, lora_dtype, M, Ns, K, rs) -> bool:
    """what hqq_hip_lora_shrink / hqq_hip_lora_expand serve (the library's own answer, nothing launched): a group of 1 .. GEMV_MAX_GROUP layers of ranks
    `rs` (1 .. 256 each) and widths `Ns` on 1 .. GEMV_MAX_M rows of K features, K and every N a multiple of 8, activations in fp16 / bf16, adapters in
    fp32 / fp16 / bf16 (A and B of one dtype: `lora_dtype`)"""
    Ns, rs = tuple(Ns), tuple(rs)
    if dtype not in _DT or lora_dtype not in _DT or len(Ns) != len(rs) or not rs:
        return False
    return bool(_C.lib().hqq_hip_lora_decode_covers(len(rs), _i64s(Ns), _i64s(rs), int(M), int(K), _DT[dtype], _DT[lora_dtype], _DT[lora_dtype]))


def lora_decode_workspace_bytes(M: int, K: int, rs) -> int:
    """bytes of workspace lora_shrink / lora_expand need for layers of ranks `rs` on M rows of K features (0: a group they refuse)"""
    rs = tuple(rs)
    return int(_C.lib().hqq_hip_lora_decode_workspace_bytes(len(rs), _i64s(rs), int(M), int(K))) if rs else 0


def lora_decode_workspace(device, M: int, K: int, rs) -> Tensor:
    """a workspace of lora_decode_workspace_bytes(M, K, rs) bytes on `device` for lora_shrink / lora_expand / lora_apply: the caller's own (a decode step
    keeps one for its lifetime, so that a captured graph replays on a static address), not to be shared by calls that may run concurrently.  It needs
    no clearing: every partial sum is written before it is read."""
    need = lora_decode_workspace_bytes(M, K, rs)
    if not need:
        raise NotImplementedError(f"hqq_amd: lora_shrink / lora_expand do not cover ranks {tuple(rs)} on {M} rows of {K} features: {_C.last_error()}")
    return torch.empty(need, dtype=torch.uint8, device=device)


def _lora_ws(ws: Tensor, who: str) -> None:
    if not isinstance(ws, Tensor) or ws.dtype != torch.uint8 or not ws.is_contiguous():
        raise ValueError(f"hqq_amd: {who} takes the workspace lora_decode_workspace() returns (a dense uint8 tensor)")


def lora_shrink(x: Tensor, As, workspace: Tensor) -> None:
    """t_l = x @ A_l in fp32 for the 1 .. GEMV_MAX_GROUP adapters `As` ([K, r_l] each, one dtype, contiguous) that read the same x [*, K] of 1 .. GEMV_MAX_M
    rows: ONE launch (hqq_hip_lora_shrink), the K slices' partial sums parked in `workspace` for lora_expand.  Deterministic; row m's bits do not
    depend on the other rows.  Raises NotImplementedError outside lora_decode_covers()."""
    As = list(As)
    n = len(As)
    _dev(x, workspace, *As)
    _lora_ws(workspace, "lora_shrink")
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise NotImplementedError(f"hqq_amd: lora_shrink takes 1 .. {GEMV_MAX_GROUP} adapters per call, got {n}")
    K = x.shape[-1]
    if any(A.dim() != 2 or A.shape[0] != K or not A.is_contiguous() for A in As):
        raise ValueError(f"hqq_amd: lora_shrink needs dense A [K, r] matrices for x of {K} features, got {[tuple(A.shape) for A in As]}")
    if len({A.dtype for A in As}) != 1 or any(A.device != x.device for A in As) or workspace.device != x.device:
        raise TypeError("hqq_amd: lora_shrink needs adapters of ONE dtype, on x's device together with the workspace")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    VP = ctypes.c_void_p * n
    with torch.cuda.device(x.device):
        rc = _C.lib().hqq_hip_lora_shrink(n, _p(x2), VP(*[_p(A) for A in As]), _i64s(A.shape[1] for A in As), x2.shape[0], int(K), _dt(x.dtype),
                                          _dt(As[0].dtype), _p(workspace), workspace.numel(), _stream())
    _C.check(rc, "hqq_hip_lora_shrink")


def lora_expand(workspace: Tensor, Bs, scalings, ys, K: int) -> None:
    """y_l <- round(y_l + round(scaling_l * t_l @ B_l)) in place for the group lora_shrink just served: ONE launch (hqq_hip_lora_expand).  Bs: [r_l, N_l]
    each (one dtype, contiguous); scalings: host floats; ys: dense [M, N_l] outputs in fp16 / bf16 that hold the base layers' results; K: the features
    of the x the shrink read (it fixes the number of partial sums).  u is formed in fp32 over j = 0 .. r - 1 in ascending order from the partials summed in
    slice order, rounded once to y's dtype, added with one more rounding: HQQLinearLoRA.forward's `out + forward_lora(x).to(x_dtype)`."""
    Bs, ys, scalings = list(Bs), list(ys), [float(s) for s in scalings]
    n = len(Bs)
    _dev(workspace, *Bs, *ys)
    _lora_ws(workspace, "lora_expand")
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise NotImplementedError(f"hqq_amd: lora_expand takes 1 .. {GEMV_MAX_GROUP} adapters per call, got {n}")
    if len(ys) != n or len(scalings) != n:
        raise ValueError("hqq_amd: lora_expand needs one scaling and one output per adapter")
    if any(B.dim() != 2 or not B.is_contiguous() for B in Bs):
        raise ValueError("hqq_amd: lora_expand needs dense B [r, N] matrices")
    M = ys[0].numel() // Bs[0].shape[1]
    if any(y.numel() != M * B.shape[1] or y.shape[-1] != B.shape[1] or not y.is_contiguous() or y.dtype != ys[0].dtype for y, B in zip(ys, Bs)):
        raise ValueError(f"hqq_amd: lora_expand updates dense [M, N] outputs of one dtype and {M} rows, N that of each B")
    if len({B.dtype for B in Bs}) != 1 or any(t.device != workspace.device for t in Bs + ys):
        raise TypeError("hqq_amd: lora_expand needs adapters of ONE dtype, on the workspace's device together with the outputs")
    VP = ctypes.c_void_p * n
    with torch.cuda.device(workspace.device):
        rc = _C.lib().hqq_hip_lora_expand(n, _p(workspace), workspace.numel(), VP(*[_p(B) for B in Bs]), (ctypes.c_float * n)(*scalings),
                                          VP(*[_p(y) for y in ys]), _i64s(B.shape[1] for B in Bs), _i64s(B.shape[0] for B in Bs), int(M), int(K),
                                          _dt(ys[0].dtype), _dt(Bs[0].dtype), _stream())
    _C.check(rc, "hqq_hip_lora_expand")


def lora_apply(x: Tensor, adapters, ys, workspace: Tensor | None = None):
    """ys[l] += (x @ A_l @ B_l * scaling_l).to(x.dtype) in place for `adapters` = [(A_l, B_l, scaling_l), ...] that share x: lora_shrink, then lora_expand
    (two launches for the whole group).  ys hold the base layers' outputs on the same rows.  workspace: lora_decode_workspace(...) of at least this
    group's size; None allocates one.  Returns ys."""
    adapters = list(adapters)
    As, Bs = [a[0] for a in adapters], [a[1] for a in adapters]
    if any(A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[0] for A, B in zip(As, Bs)):
        raise ValueError("hqq_amd: lora_apply needs A [K, r] and B [r, N] per adapter")
    if any(A.dtype != B.dtype for A, B in zip(As, Bs)):
        raise TypeError("hqq_amd: lora_apply: lora_A and lora_B must share a dtype")
    K = x.shape[-1]
    if workspace is None:
        workspace = lora_decode_workspace(x.device, x.numel() // K, K, [A.shape[1] for A in As])
    lora_shrink(x, As, workspace)
    lora_expand(workspace, Bs, [a[2] for a in adapters], ys, K)
    return ys


# ---- the same pair with one adapter per ROW, picked on the device from banks of stacked adapters (hqq_hip_lora_shrink_routed / _expand_routed) -----------
LORA_MAX_ADAPTERS = 256


def lora_routed_covers(dtype, lora_dtype, n_adapters, M, Ns, K, rs) -> bool:
    """what hqq_hip_lora_shrink_routed / hqq_hip_lora_expand_routed serve (the library's own answer, nothing launched): what lora_decode_covers
    accepts, with 1 .. LORA_MAX_ADAPTERS adapters in the bank"""
    Ns, rs = tuple(Ns), tuple(rs)
    if dtype not in _DT or lora_dtype not in _DT or len(Ns) != len(rs) or not rs:
        return False
    return bool(_C.lib().hqq_hip_lora_routed_covers(len(rs), _i64s(Ns), _i64s(rs), int(n_adapters), int(M), int(K), _DT[dtype], _DT[lora_dtype]))


def _lora_slots(slots: Tensor, M: int, device, who: str) -> None:
    if not isinstance(slots, Tensor) or slots.dtype != torch.int64 or slots.dim() != 1 or slots.numel() != M or not slots.is_contiguous():
        raise ValueError(f"hqq_amd: {who} takes one slot per row: a dense int64 tensor of {M} elements")
    if slots.device != device:
        raise TypeError(f"hqq_amd: {who} reads the slots on the device the rows are on")


def lora_shrink_routed(x: Tensor, A_banks, slots: Tensor, workspace: Tensor) -> None:
    """lora_shrink with one adapter per row: A_banks are [n, K, r_l] each (one dtype, contiguous, the same n), slots int64 [M] on the device; row m
    reads A_banks[l][slots[m]], and a row whose slot is outside [0, n) (-1: no adapter) reads nothing and leaves no partial.  ONE launch
    (hqq_hip_lora_shrink_routed); the slots are read by the kernel only, so a captured call follows a later slots.copy_().  A row's bits are those of
    lora_shrink on that row alone with its adapter.  Raises NotImplementedError outside lora_routed_covers()."""
    As = list(A_banks)
    n = len(As)
    _dev(x, workspace, slots, *As)
    _lora_ws(workspace, "lora_shrink_routed")
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise NotImplementedError(f"hqq_amd: lora_shrink_routed takes 1 .. {GEMV_MAX_GROUP} banks per call, got {n}")
    K = x.shape[-1]
    if any(A.dim() != 3 or A.shape[1] != K or A.shape[0] != As[0].shape[0] or not A.is_contiguous() for A in As):
        raise ValueError(f"hqq_amd: lora_shrink_routed needs dense A banks [n, K, r] of one n for x of {K} features, got {[tuple(A.shape) for A in As]}")
    if len({A.dtype for A in As}) != 1 or any(A.device != x.device for A in As) or workspace.device != x.device:
        raise TypeError("hqq_amd: lora_shrink_routed needs banks of ONE dtype, on x's device together with the workspace")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    _lora_slots(slots, x2.shape[0], x.device, "lora_shrink_routed")
    VP = ctypes.c_void_p * n
    with torch.cuda.device(x.device):
        rc = _C.lib().hqq_hip_lora_shrink_routed(n, _p(x2), VP(*[_p(A) for A in As]), _i64s(A.shape[2] for A in As), int(As[0].shape[0]), _p(slots),
                                                 x2.shape[0], int(K), _dt(x.dtype), _dt(As[0].dtype), _p(workspace), workspace.numel(), _stream())
    _C.check(rc, "hqq_hip_lora_shrink_routed")


def lora_expand_routed(workspace: Tensor, B_banks, scalings, slots: Tensor, ys, K: int) -> None:
    """lora_expand with one adapter per row, for the group lora_shrink_routed just served with the same slots: B_banks [n, r_l, N_l] each (one dtype,
    contiguous), scalings float32 [n] tensors ON THE DEVICE (one per bank: replacing an adapter's scaling does not touch a captured call), ys dense
    [M, N_l] outputs in fp16 / bf16 that hold the base layers' results.  Row m of y_l takes scalings[l][slots[m]] and B_banks[l][slots[m]]; a row whose
    slot is outside [0, n) is not written.  ONE launch (hqq_hip_lora_expand_routed)."""
    Bs, ys, scalings = list(B_banks), list(ys), list(scalings)
    n = len(Bs)
    _dev(workspace, slots, *Bs, *ys)
    _lora_ws(workspace, "lora_expand_routed")
    if not 1 <= n <= GEMV_MAX_GROUP:
        raise NotImplementedError(f"hqq_amd: lora_expand_routed takes 1 .. {GEMV_MAX_GROUP} banks per call, got {n}")
    if len(ys) != n or len(scalings) != n:
        raise ValueError("hqq_amd: lora_expand_routed needs one scaling tensor and one output per bank")
    if any(B.dim() != 3 or B.shape[0] != Bs[0].shape[0] or not B.is_contiguous() for B in Bs):
        raise ValueError("hqq_amd: lora_expand_routed needs dense B banks [n, r, N] of one n")
    na = int(Bs[0].shape[0])
    if any(not isinstance(s, Tensor) or s.dtype != torch.float32 or s.dim() != 1 or s.numel() != na or not s.is_contiguous() for s in scalings):
        raise ValueError(f"hqq_amd: lora_expand_routed needs the scalings as dense float32 tensors of {na} elements")
    M = ys[0].numel() // Bs[0].shape[2]
    if any(y.numel() != M * B.shape[2] or y.shape[-1] != B.shape[2] or not y.is_contiguous() or y.dtype != ys[0].dtype for y, B in zip(ys, Bs)):
        raise ValueError(f"hqq_amd: lora_expand_routed updates dense [M, N] outputs of one dtype and {M} rows, N that of each bank")
    if len({B.dtype for B in Bs}) != 1 or any(t.device != workspace.device for t in Bs + ys + scalings):
        raise TypeError("hqq_amd: lora_expand_routed needs banks of ONE dtype, on the workspace's device together with the scalings and the outputs")
    _lora_slots(slots, M, workspace.device, "lora_expand_routed")
    VP = ctypes.c_void_p * n
    with torch.cuda.device(workspace.device):
        rc = _C.lib().hqq_hip_lora_expand_routed(n, _p(workspace), workspace.numel(), VP(*[_p(B) for B in Bs]), VP(*[_p(s) for s in scalings]),
                                                 VP(*[_p(y) for y in ys]), _i64s(B.shape[2] for B in Bs), _i64s(B.shape[1] for B in Bs), na, _p(slots),
                                                 int(M), int(K), _dt(ys[0].dtype), _dt(Bs[0].dtype), _stream())
    _C.check(rc, "hqq_hip_lora_expand_routed")


def lora_apply_routed(x: Tensor, banks, slots: Tensor, ys, workspace: Tensor | None = None):
    """ys[l][m] += (x[m] @ A_l[a] @ B_l[a] * scaling_l[a]).to(x.dtype) in place with a = slots[m], for `banks` = [(A_bank_l, B_bank_l, scaling_l), ...]
    that share x: lora_shrink_routed, then lora_expand_routed (two launches for the whole group).  Rows whose slot names no adapter keep ys[l][m].
    workspace: lora_decode_workspace(...) of at least this group's size; None allocates one.  Returns ys."""
    banks = list(banks)
    As, Bs = [b[0] for b in banks], [b[1] for b in banks]
    if any(A.dim() != 3 or B.dim() != 3 or A.shape[2] != B.shape[1] or A.shape[0] != B.shape[0] for A, B in zip(As, Bs)):
        raise ValueError("hqq_amd: lora_apply_routed needs A [n, K, r] and B [n, r, N] per bank")
    if any(A.dtype != B.dtype for A, B in zip(As, Bs)):
        raise TypeError("hqq_amd: lora_apply_routed: the A and B banks must share a dtype")
    K = x.shape[-1]
    if workspace is None:
        workspace = lora_decode_workspace(x.device, x.numel() // K, K, [A.shape[2] for A in As])
    lora_shrink_routed(x, As, slots, workspace)
    lora_expand_routed(workspace, Bs, [b[2] for b in banks], slots, ys, K)
    return ys


def _forward_axis0(x, W_q, scale, zero, bias, N, K, group_size, nbits, out, opts, library_gemm: bool = False) -> Tensor:
    """axis-0 layers: decode sizes through hqq_hip_gemv_axis0; GEMV_MAX_M + 1 .. AXIS0_GEMM_ROUTE_MAX_M rows through hqq_hip_gemm_axis0 (unless
    library_gemm); everything else as HQQLinear has always run them — the HIP dequantise kernel (axis 0) + torch.matmul, then `out += bias`
    (quantize.py:880-898)"""
    M = x.numel() // K if K else 0
    if x.is_cuda and decode_axis0_covers(x.dtype, M, N, K, group_size, nbits):
        return gemv_axis0(x, W_q, scale, zero, bias, N, K, group_size, nbits, out=out, opts=opts)
    if x.is_cuda and not library_gemm and M <= AXIS0_GEMM_ROUTE_MAX_M and gemm_axis0_covers(x.dtype, M, N, K, group_size, nbits):
        return gemm_axis0(x, W_q, scale, zero, bias, N, K, group_size, nbits, out=None if out is None else out.reshape(-1, N), opts=opts)
    gs = N if group_size is None else int(group_size)
    W = dequantize(W_q, scale.reshape(-1), zero.reshape(-1), N, K, gs, nbits, 0)
    y = torch.matmul(x.reshape(-1, K), W.t(), out=None if out is None else out.reshape(-1, N))
    if bias is not None:
        y += bias
    return y.reshape(*x.shape[:-1], N)


def gemm_dense(x: Tensor, W: Tensor, bias=None, out: Tensor | None = None) -> Tensor:
    """HQQLinear.matmul on dequantised weights: x [*, K] @ W[N, K].T (+ bias) on the in-tree MFMA GEMM (csrc/gemm_dense.hip), fp16 / bf16"""
    _dev(x, W, bias)
    N, K = W.shape
    if x.shape[-1] != K or x.dtype != W.dtype or (bias is not None and bias.dtype != W.dtype):
        raise TypeError("hqq_amd: gemm_dense takes x [*, K], W [N, K] and bias of one compute dtype")
    x2 = x.reshape(-1, K)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    if M > 0:
        with torch.cuda.device(x.device):
            rc = _C.lib().hqq_hip_gemm_dense(_p(x2), _p(W.contiguous()), _p(bias), _p(out), M, N, K, _dt(x.dtype), _stream())
        _C.check(rc, "hqq_hip_gemm_dense")
    return out.reshape(*x.shape[:-1], N)


def dense_covers(dtype, N, K) -> bool:
    return dtype in (torch.float16, torch.bfloat16) and K % 64 == 0 and K >= 64 and N % 4 == 0


# Every composed forward (what the fused kernels do not cover: group sizes other than 64 outside gemm.hip's 4- / 2-bit fp16 tiles, K % 128 != 0, 8-bit / bf16 with
# other group sizes) runs dequantise kernel + the in-tree MFMA GEMM from 17 rows on — no library GEMM on any fp16 / bf16 axis-1 path (round 6; until then
# 17..2560 rows of such layers went to torch.matmul).  The dense kernel's 256 x 256 tiles leave CUs idle below ~2000 rows (16 workgroups at 256 rows of a
# 4096-wide layer: ~90 us where a library's small-tile kernels take ~40): a known cost on shapes outside BASELINE.json's, `library_gemm=True` is the opt-out.
DENSE_MIN_M = 17


def _compose(x, W, bias, out, N, K, library: bool) -> Tensor:
    """the route after the dequantise kernel: the in-tree MFMA GEMM from DENSE_MIN_M rows on; torch.matmul — what the reference itself calls — below that
    (decode-sized residue), for shapes the in-tree kernel does not cover (K % 64 != 0, N % 4 != 0), or when asked for (library=True)"""
    if not library and dense_covers(x.dtype, N, K) and x.numel() // K >= DENSE_MIN_M:
        return gemm_dense(x, W, bias, out=None if out is None else out.reshape(-1, N))
    y = torch.matmul(x.reshape(-1, K), W.t(), out=out)
    if bias is not None:
        y += bias
    return y.reshape(*x.shape[:-1], N)


def forward(x, W_q, scale, zero, bias, N, K, group_size, nbits, out=None, fused=None, opts=None, library_gemm: bool = False, axis: int = 1) -> Tensor:
    """y = x @ dequantize(W_q)^T (+ bias).  The decode routes (route(); include/hqq_hip.h): weight-streaming decode kernels; larger M: fused MFMA
    dequant-GEMM where hqq_hip_forward_prefers_fused says so, beyond — and for what the fused kernels do not cover, unless fused=True — the dequantise
    kernel + the in-tree dense MFMA GEMM (library_gemm=True: a library GEMM instead, the bench's comparison; also the residual route for
    K % 64 != 0 or N % 4 != 0).  Same dequantised weights either way.  fused=None also composes the decode-sized cases no route covers;
    fused=True never composes: an uncovered configuration raises.
    axis=0: a layer quantised along axis 0 — decode_axis0_covers() shapes through hqq_hip_gemv_axis0, gemm_axis0_covers() shapes up to
    AXIS0_GEMM_ROUTE_MAX_M rows through hqq_hip_gemm_axis0, the rest through the dequantise kernel + torch.matmul (library_gemm=True: that route
    from 17 rows on, the comparison leg; `fused` does not apply)."""
    M = x.numel() // K if K else 0
    if x.dtype != scale.dtype or zero.dtype != scale.dtype or (bias is not None and bias.dtype != scale.dtype):
        raise TypeError("hqq_amd: x / scale / zero / bias must share the compute dtype")
    if axis == 0:
        return _forward_axis0(x, W_q, scale, zero, bias, N, K, group_size, nbits, out, opts, library_gemm)
    if axis != 1:
        raise ValueError(f"hqq_amd: axis must be 0 or 1, got {axis}")
    w3s = nbits == 3 and bool(_opts(opts) & OPT_W3S)   # the 3-bit stream layout (w3s_pack)
    if fused is None:
        # asked for the layer's layout, not its arithmetic bits.  The stream layout composes 5..64 rows outside the skinny kernel.
        r = route(x.dtype, M, (int(N),), int(K), group_size, nbits, OPT_W3S if w3s else 0)
        fused = (r == ROUTE_SKINNY or (r in DECODE_ROUTES and not (LIBRARY_GEMM_MIN_M and M >= LIBRARY_GEMM_MIN_M)) or
                 (r == ROUTE_GEMM_PIPE and M > (SKINNY_MAX_M if w3s else GEMV_MAX_M) and x.is_cuda and prefers_fused(x.dtype, M, int(N), int(K), group_size, nbits, w3s)))
    if fused:
        return _fwd("hqq_hip_forward", x, W_q, scale, zero, bias, N, K, group_size, nbits, out, opts)
    W = dequantize(w3s_unpack(W_q, N, K) if w3s else W_q, scale.reshape(-1), zero.reshape(-1), N, K, group_size, nbits, 1)
    return _compose(x, W, bias, out, N, K, library_gemm)


def _solver_dt(solver_dtype) -> int:
    """the solver precisions the kernels have: float32 (the reference's CPU solver, the default) and float16 (its GPU solver)"""
    if solver_dtype not in (torch.float32, torch.float16):
        raise ValueError(f"hqq_amd: solver_dtype must be torch.float32 or torch.float16, got {solver_dtype}")
    return _DT[solver_dtype]


def quantize(W: Tensor, nbits=4, group_size: int = 64, round_zero: bool = False, optimize: bool = True,
             iters: int = 20, beta: float = 10.0, lp_norm: float = 0.7, return_info: bool = False, axis: int = 1,
             solver_dtype: torch.dtype = torch.float32):
    """Quantizer.quantize(channel_wise=True, bitpack=True) with optimize_weights_proximal_legacy, fused with packing.
    axis=1: groups are runs of `group_size` consecutive elements — returns (W_q packed [packed_rows(R), gs], scale [R,1] f32 (already
    inverted), zero [R,1] f32), R = numel / gs.  axis=0: W is viewed as [gs, C], C = numel / gs, every column a group — returns
    (W_q packed [packed_rows(gs), C], scale [1,C], zero [1,C]).  [+ info int32[2] on device with return_info]
    solver_dtype=torch.float16 runs the reference's GPU solver (fp16 arithmetic, optimize.py:231) instead of its CPU float32 one;
    scale and zero are then fp16, as the reference returns them."""
    sdt = _solver_dt(solver_dtype)
    _dev(W)
    if axis not in (0, 1):
        raise ValueError("axis should be either 0 or 1")
    if W.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        W = W.float()
    W = W.contiguous()
    numel = W.numel()
    if group_size is None or numel % group_size:
        raise ValueError("group_size should be divisble by the total tensor dimensions. shape: "
                         f"{tuple(W.shape)}, group_size: {group_size}")   # quantize.py:94-100
    pack_bits = PACK_BITS[nbits]
    max_v = int(round(2 ** nbits - 1))
    R = numel // group_size
    dev = W.device
    if axis == 1:
        prow = packed_rows(pack_bits, R)
        W_q = torch.empty((prow, group_size), dtype=torch.int32 if pack_bits == 3 else torch.uint8, device=dev)
        scale = torch.empty((R, 1), dtype=solver_dtype, device=dev)
        zero = torch.empty((R, 1), dtype=solver_dtype, device=dev)
    else:
        prow = packed_rows(pack_bits, group_size)
        W_q = torch.empty((prow, R), dtype=torch.int32 if pack_bits == 3 else torch.uint8, device=dev)
        scale = torch.empty((1, R), dtype=solver_dtype, device=dev)
        zero = torch.empty((1, R), dtype=solver_dtype, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    L = _C.lib()
    it = iters if optimize else 0
    ws_bytes = L.hqq_hip_quantize_workspace_bytes(numel, group_size, it)
    if ws_bytes == 0:
        raise ValueError(f"hqq_amd: bad quantize arguments (numel={numel}, group_size={group_size}, iters={it})")
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    fn = L.hqq_hip_quantize_solver if axis == 1 else L.hqq_hip_quantize_axis0_solver
    with torch.cuda.device(dev):
        rc = fn(_p(W), _dt(W.dtype), numel, group_size, max_v, pack_bits, int(bool(round_zero)), int(bool(optimize)),
                it, float(beta), float(lp_norm), sdt, _p(W_q), _p(scale), _p(zero), _p(info), _p(ws), ws_bytes, _stream())
    _C.check(rc, "hqq_hip_quantize" if axis == 1 else "hqq_hip_quantize_axis0")
    if return_info:
        return W_q, scale, zero, info
    return W_q, scale, zero


def optimize(W: Tensor, scale: Tensor, zero: Tensor, max_v: int, axis: int = 1, iters: int = 20, beta: float = 10.0, lp_norm: float = 0.7,
             return_info: bool = False, solver_dtype: torch.dtype = torch.float32):
    """optimize_weights_proximal_legacy on its own (optimize.py:208-255): W is the grouped 2-D view ([groups, gs] for axis=1, [gs, groups] for
    axis=0), scale / zero float32 with one value per group.  Returns (levels uint8 in W's shape, zero float32 in zero's shape)
    [+ info int32[2] on device with return_info].  solver_dtype=torch.float16: the reference's GPU solver; zero is then fp16."""
    sdt = _solver_dt(solver_dtype)
    _dev(W, scale, zero)
    if W.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        W = W.float()
    W = W.contiguous()
    gs = W.shape[1] if axis == 1 else W.shape[0]
    R = W.numel() // gs
    sc, ze = scale.reshape(-1).float().contiguous(), zero.reshape(-1).float().contiguous()
    if sc.numel() != R or ze.numel() != R:
        raise ValueError(f"hqq_amd: scale / zero must hold one value per group ({R}), got {sc.numel()} / {ze.numel()}")
    dev = W.device
    levels = torch.empty(W.shape, dtype=torch.uint8, device=dev)
    zero_out = torch.empty(zero.shape, dtype=solver_dtype, device=dev)
    info = torch.zeros((2,), dtype=torch.int32, device=dev)
    L = _C.lib()
    ws_bytes = int(L.hqq_hip_quantize_workspace_bytes(W.numel(), gs, int(iters))) + 4 * R
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = L.hqq_hip_optimize_solver(_p(W), _dt(W.dtype), W.numel(), gs, int(axis), int(max_v), _p(sc), _p(ze), int(iters), float(beta),
                                       float(lp_norm), sdt, _p(levels), _p(zero_out), _p(info), _p(ws), ws_bytes, _stream())
    _C.check(rc, "hqq_hip_optimize")
    if return_info:
        return levels, zero_out, info
    return levels, zero_out


def quantize_tensorwise(W: Tensor, nbits=4, round_zero: bool = False):
    """Quantizer.quantize(channel_wise=False) (quantize.py:114-116): one scale / zero from the tensor's min and max, no solver; the
    levels packed in the tensor's own 2-D shape.  Returns (W_q packed [packed_rows(rows), cols], scale 0-d f32 (inverted), zero 0-d f32)."""
    _dev(W)
    if W.dim() != 2:
        raise ValueError("hqq_amd: quantize_tensorwise takes a 2-D tensor")
    if W.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        W = W.float()
    W = W.contiguous()
    rows, cols = W.shape
    pack_bits = PACK_BITS[nbits]
    dev = W.device
    W_q = torch.empty((packed_rows(pack_bits, rows), cols), dtype=torch.int32 if pack_bits == 3 else torch.uint8, device=dev)
    meta = torch.empty((2,), dtype=torch.float32, device=dev)
    ws = torch.empty((16384,), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = _C.lib().hqq_hip_quantize_tensor(_p(W), _dt(W.dtype), rows, cols, int(round(2 ** nbits - 1)), pack_bits, int(bool(round_zero)),
                                              _p(W_q), _p(meta), meta.data_ptr() + 4, _p(ws), ws.numel(), _stream())
    _C.check(rc, "hqq_hip_quantize_tensor")
    return W_q, meta[0], meta[1]


# ---- the steps either side of the GEMVs in a decode step (csrc/block.hip; include/hqq_hip.h) --------------------------------------------
def add_rmsnorm(h: Tensor, delta, weight: Tensor, eps: float, out: Tensor | None = None) -> Tensor:
    """h += delta (in place, if delta is given), then LlamaRMSNorm(h) with `weight` — HF's arithmetic, one kernel.  h: [..., H] fp16 / bf16, dense, H a multiple of 8."""
    _dev(h, delta, weight)
    H = h.shape[-1]
    if out is None:
        out = torch.empty_like(h)
    with torch.cuda.device(h.device):
        rc = _C.lib().hqq_hip_add_rmsnorm(_p(h), _p(delta), _p(weight), float(eps), _p(out), h.numel() // H, H, _dt(h.dtype), _stream())
    _C.check(rc, "hqq_hip_add_rmsnorm")
    return out


# ---- the glue kernels of a decode step for B independent sequences (csrc/block.hip, the *_batched entry points: the sequence is a grid index, and row b
#      gives the bits a launch for sequence b alone gives).  tok / pos: int64 [B] on the device; every other tensor is dense, one row (or cache) per
#      sequence.  Each kernel has ONE implementation here, the *_batched function: it validates and calls the library.  The single-sequence function
#      of the same name is that call on views of its arguments as a batch of one ------------------------------------------------------------------
def _batch_of(pos: Tensor, who: str) -> int:
    if pos.dtype != torch.int64 or not pos.is_contiguous() or pos.numel() < 1:
        raise ValueError(f"hqq_amd: {who} takes a dense int64 position tensor of B >= 1 elements")
    return pos.numel()


def _seq1(pos):
    """a single sequence's position tensor (int64 [1]; None stays None) as the batch of one: its first element, the same memory"""
    return None if pos is None else pos.view(-1)[:1]


def _cache1(cache: Tensor) -> Tensor:
    """a single sequence's cache [n_kv_heads, cache_len, head_dim] as the batch of one [1, n_kv_heads, cache_len, head_dim], the same memory"""
    return cache.view(1, *cache.shape[-3:])


def token_prologue_batched(tok: Tensor, pos: Tensor, embed: Tensor, h: Tensor, cos_tab=None, sin_tab=None, cos=None, sin=None, mask=None) -> None:
    """The front of a decode step for B sequences in one launch (hqq_hip_token_prologue_batched): h [B, H] = embed[tok[b]]; cos / sin [B, head_dim] = row pos[b] of the
    rotary tables [L, head_dim] (skipped when the tables are None); mask [B, L] = 0 up to pos[b], -inf beyond (skipped when None).  tok [B] or [B, 1] / pos [B]
    int64 on the device: graph-replay safe.  Copies and compares only: per row the same bits as embed_tokens, index_select and torch.where."""
    _dev(tok, pos, embed, h)
    B = _batch_of(pos, "token_prologue_batched")
    if tok.dtype != torch.int64 or tok.numel() != B or not tok.is_contiguous() or embed.dim() != 2 or not embed.is_contiguous() or \
            h.numel() != B * embed.shape[1] or not h.is_contiguous() or h.dtype != embed.dtype:
        raise ValueError("hqq_amd: token_prologue_batched takes int64 tok / pos of B elements, a dense [vocab, H] embedding and a dense h [B, H] of its dtype")
    L, hd = 1, 0
    if cos_tab is not None:
        _dev(cos_tab, sin_tab, cos, sin)
        if cos_tab.shape != sin_tab.shape or cos_tab.dim() != 2 or not (cos_tab.is_contiguous() and sin_tab.is_contiguous()) or cos.numel() != B * cos_tab.shape[1] or \
                sin.numel() != B * cos_tab.shape[1] or not (cos.is_contiguous() and sin.is_contiguous()) or any(t.dtype != embed.dtype for t in (cos_tab, sin_tab, cos, sin)):
            raise ValueError("hqq_amd: token_prologue_batched takes dense [L, head_dim] rotary tables and dense [B, head_dim] outputs of the compute dtype")
        L, hd = int(cos_tab.shape[0]), int(cos_tab.shape[1])
    if mask is not None:
        _dev(mask)
        if mask.dtype != embed.dtype or not mask.is_contiguous() or mask.numel() % B or (cos_tab is not None and mask.numel() != B * L):
            raise ValueError("hqq_amd: token_prologue_batched's mask is a dense [B, L] tensor of the compute dtype, L the rotary tables' rows")
        L = int(mask.numel() // B)
    with torch.cuda.device(h.device):
        rc = _C.lib().hqq_hip_token_prologue_batched(_p(tok), _p(pos), B, _p(embed), int(embed.shape[0]), int(embed.shape[1]), _p(cos_tab), _p(sin_tab), L, hd, _p(h),
                                                     _p(cos), _p(sin), _p(mask), _dt(embed.dtype), _stream())
    _C.check(rc, "hqq_hip_token_prologue_batched")


def token_prologue(tok: Tensor, pos: Tensor, embed: Tensor, h: Tensor, cos_tab=None, sin_tab=None, cos=None, sin=None, mask=None) -> None:
    """token_prologue_batched for one sequence: tok [1, 1] / pos [1], h [H] (or [1, H]), cos / sin [head_dim], mask [L]"""
    token_prologue_batched(tok, _seq1(pos), embed, h, cos_tab, sin_tab, cos, sin, mask)


def _batched_cache(who: str, k_cache: Tensor, v_cache: Tensor, B: int):
    """the dense caches [B, n_kv, L, hd] of B sequences: (n_kv, L, hd)"""
    if k_cache.dim() != 4 or k_cache.shape[0] != B or v_cache.shape != k_cache.shape or not k_cache.is_contiguous() or not v_cache.is_contiguous():
        raise ValueError(f"hqq_amd: {who} takes dense [B, n_kv_heads, cache_len, head_dim] caches, B the positions' count")
    return tuple(int(x) for x in k_cache.shape[1:])


def _qkv_extents(who: str, n: int, n_kv: int, hd: int, q: Tensor, k: Tensor, v: Tensor, q_out: Tensor, cos: Tensor, sin: Tensor, dt=None, R: str = "B", tail: str = "") -> int:
    """the extents every rotary-and-cache front (`who`) asks of its row tensors, n rows (R in the message, which `tail` ends) against caches of n_kv heads of hd
    values: dense q / q_out [n, n_heads * hd], k / v [n, n_kv * hd] and cos / sin [n, hd], all of dtype dt where one is given.  Returns n_heads."""
    ts = (q, k, v, q_out, cos, sin)
    if hd < 1 or cos.numel() != n * hd or sin.numel() != n * hd or any(t.numel() % (n * hd) or not t.is_contiguous() for t in ts) or \
            k.numel() != n * n_kv * hd or v.numel() != k.numel() or q_out.numel() != q.numel() or (dt is not None and any(t.dtype != dt for t in ts)):
        raise ValueError(f"hqq_amd: {who} takes dense q / q_out [{R}, n_heads * hd], k / v [{R}, n_kv_heads * hd] and cos / sin [{R}, hd]{tail}")
    return q.numel() // (n * hd)


def _rope_cache_args(who: str, q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor, v_cache: Tensor, q_out: Tensor):
    """what rope_cache_batched, qknorm_rope_cache_batched and bias_rope_cache_batched (`who`) all ask of their tensors: dense caches of the positions' batch and
    q / k / v / q_out / cos / sin of matching extents.  Returns (B, head_dim, n_heads, n_kv_heads, cache_len), what the launches are given."""
    B = _batch_of(pos, who)
    n_kv, L, hd = _batched_cache(who, k_cache, v_cache, B)
    return B, hd, _qkv_extents(who, B, n_kv, hd, q, k, v, q_out, cos, sin), n_kv, L


def rope_cache_batched(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor, v_cache: Tensor, q_out: Tensor) -> Tensor:
    """one token of B sequences in one launch: q_out [B, n_heads * hd] = rotary(q [B, n_heads * hd]) with cos / sin [B, hd]; rotary(k) and v ([B, n_kv * hd])
    go into row b of the caches [B, n_kv_heads, cache_len, head_dim] (HF's StaticCache tensors of batch B) at position pos[b]; a position outside the cache writes nothing"""
    _dev(q, k, v, cos, sin, pos, k_cache, v_cache, q_out)
    B, hd, n_heads, n_kv, L = _rope_cache_args("rope_cache_batched", q, k, v, cos, sin, pos, k_cache, v_cache, q_out)
    with torch.cuda.device(q.device):
        rc = _C.lib().hqq_hip_rope_cache_batched(_p(q), _p(k), _p(v), _p(cos), _p(sin), _p(pos), B, _p(q_out), _p(k_cache), _p(v_cache), n_heads, n_kv, hd, L,
                                                 _dt(q.dtype), _stream())
    _C.check(rc, "hqq_hip_rope_cache_batched")
    return q_out


def rope_cache(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor, v_cache: Tensor, q_out: Tensor) -> Tensor:
    """rope_cache_batched for one sequence: cos / sin [hd], the static caches [n_kv_heads, cache_len, head_dim], position pos[0] (device int64)"""
    return rope_cache_batched(q, k, v, cos, sin, _seq1(pos), _cache1(k_cache), _cache1(v_cache), q_out)


def qknorm_rope_cache_batched(q: Tensor, k: Tensor, v: Tensor, q_weight: Tensor, k_weight: Tensor, q_eps: float, k_eps: float, cos: Tensor, sin: Tensor, pos: Tensor,
                              k_cache: Tensor, v_cache: Tensor, q_out: Tensor) -> Tensor:
    """rope_cache_batched with Qwen3Attention's per-head RMSNorms in front of the rotary embedding, one launch (hqq_hip_qknorm_rope_cache_batched): every head of
    q is normalised with q_weight [hd] / q_eps, every head of k with k_weight [hd] / k_eps (Qwen3RMSNorm's roundings), then rotated; q_out, the caches, v and
    the positions as in rope_cache_batched.  head_dim 64 / 128 / 256, fp16 / bf16."""
    _dev(q, k, v, q_weight, k_weight, cos, sin, pos, k_cache, v_cache, q_out)
    B, hd, n_heads, n_kv, L = _rope_cache_args("qknorm_rope_cache_batched", q, k, v, cos, sin, pos, k_cache, v_cache, q_out)
    if any(w.numel() != hd or not w.is_contiguous() for w in (q_weight, k_weight)) or \
            any(t.dtype != q.dtype for t in (k, v, q_weight, k_weight, cos, sin, k_cache, v_cache, q_out)):
        raise ValueError("hqq_amd: qknorm_rope_cache_batched takes dense norm weights of head_dim elements, and every tensor but the positions in q's dtype")
    with torch.cuda.device(q.device):
        rc = _C.lib().hqq_hip_qknorm_rope_cache_batched(_p(q), _p(k), _p(v), _p(q_weight), _p(k_weight), float(q_eps), float(k_eps), _p(cos), _p(sin), _p(pos), B,
                                                        _p(q_out), _p(k_cache), _p(v_cache), n_heads, n_kv, hd, L, _dt(q.dtype), _stream())
    _C.check(rc, "hqq_hip_qknorm_rope_cache_batched")
    return q_out


def qknorm_rope_cache(q: Tensor, k: Tensor, v: Tensor, q_weight: Tensor, k_weight: Tensor, q_eps: float, k_eps: float, cos: Tensor, sin: Tensor, pos: Tensor,
                      k_cache: Tensor, v_cache: Tensor, q_out: Tensor) -> Tensor:
    """qknorm_rope_cache_batched for one sequence: cos / sin [hd], the static caches [n_kv_heads, cache_len, head_dim], position pos[0] (device int64)"""
    return qknorm_rope_cache_batched(q, k, v, q_weight, k_weight, q_eps, k_eps, cos, sin, _seq1(pos), _cache1(k_cache), _cache1(v_cache), q_out)


def bias_rope_cache_batched(q: Tensor, k: Tensor, v: Tensor, q_bias: Tensor, k_bias: Tensor, v_bias: Tensor, cos: Tensor, sin: Tensor, pos: Tensor,
                            k_cache: Tensor, v_cache: Tensor, q_out: Tensor) -> Tensor:
    """rope_cache_batched with Qwen2Attention's projection biases added in front of the rotary embedding, one launch (hqq_hip_bias_rope_cache_batched):
    q + q_bias, k + k_bias, v + v_bias — one rounding each in q's dtype, the `out += bias` of the linears; the biases [n_heads * hd] / [n_kv_heads * hd],
    shared by every sequence —, then q and k rotated; q_out, the caches and the positions as in rope_cache_batched.  Bit for bit gemv_grouped with the biases
    followed by rope_cache_batched.  Any even head_dim, fp16 / bf16."""
    _dev(q, k, v, q_bias, k_bias, v_bias, cos, sin, pos, k_cache, v_cache, q_out)
    B, hd, n_heads, n_kv, L = _rope_cache_args("bias_rope_cache_batched", q, k, v, cos, sin, pos, k_cache, v_cache, q_out)
    if any(bias.numel() * B != t.numel() or not bias.is_contiguous() for bias, t in ((q_bias, q), (k_bias, k), (v_bias, v))) or \
            any(t.dtype != q.dtype for t in (k, v, q_bias, k_bias, v_bias, cos, sin, k_cache, v_cache, q_out)):
        raise ValueError("hqq_amd: bias_rope_cache_batched takes dense biases of one row of q / k / v each, and every tensor but the positions in q's dtype")
    with torch.cuda.device(q.device):
        rc = _C.lib().hqq_hip_bias_rope_cache_batched(_p(q), _p(k), _p(v), _p(q_bias), _p(k_bias), _p(v_bias), _p(cos), _p(sin), _p(pos), B, _p(q_out), _p(k_cache),
                                                      _p(v_cache), n_heads, n_kv, hd, L, _dt(q.dtype), _stream())
    _C.check(rc, "hqq_hip_bias_rope_cache_batched")
    return q_out


def bias_rope_cache(q: Tensor, k: Tensor, v: Tensor, q_bias: Tensor, k_bias: Tensor, v_bias: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor,
                    v_cache: Tensor, q_out: Tensor) -> Tensor:
    """bias_rope_cache_batched for one sequence: cos / sin [hd], the static caches [n_kv_heads, cache_len, head_dim], position pos[0] (device int64)"""
    return bias_rope_cache_batched(q, k, v, q_bias, k_bias, v_bias, cos, sin, _seq1(pos), _cache1(k_cache), _cache1(v_cache), q_out)


def _dense(cache) -> tuple:
    """the tensors of a dense pair (k_cache, v_cache), () for (bufs, head_dim): _kv_bufs looks at the six buffers itself"""
    return tuple(cache) if isinstance(cache[1], Tensor) else ()


def _attn_cache(who: str, cache, B):
    """the cache an attention front (`who`) is given, checked.  cache: the dense pair (k_cache, v_cache), or (bufs, head_dim) for the six buffers of a quantised
    cache (below); B: the sequences of the positions' batch, or None for ONE sequence's cache ([n_kv, L, .] or [1, n_kv, L, .]).  Returns (n_kv, L, hd, dtype,
    head, ptrs, gs): what the library is given in front of q (the width, for the buffers), the cache's pointers, and (the group size,) or ()."""
    if isinstance(cache[1], Tensor):
        k_cache, v_cache = cache
        n_kv, L, hd = _shared_cache(who, k_cache, v_cache) if B is None else _batched_cache(who, k_cache, v_cache, B)
        if v_cache.dtype != k_cache.dtype:
            raise ValueError(f"hqq_amd: {who} takes caches of one dtype (k_cache {k_cache.dtype}, v_cache {v_cache.dtype})")
        return n_kv, L, hd, k_cache.dtype, (), (_p(k_cache), _p(v_cache)), ()
    bufs, hd = cache
    if B is None:
        if len(bufs) != 6 or not all(isinstance(t, Tensor) and t.dim() in (3, 4) and (t.dim() == 3 or t.shape[0] == 1) for t in bufs):
            raise ValueError(f"hqq_amd: {who} takes ONE sequence's six cache buffers (kq, k_scale, k_zero, vq, v_scale, v_zero) [n_kv_heads, cache_len, .] (or [1, ...])")
        bufs = tuple(t.view(1, *t.shape[-3:]) for t in bufs)
    Bc, n_kv, L, nbits, gs, dt = _kv_bufs(bufs, int(hd), who)
    if B is not None and Bc != B:
        raise ValueError(f"hqq_amd: {who} takes buffers of the positions' batch ({Bc} sequences against {B} positions)")
    return n_kv, L, int(hd), dt, (nbits,), tuple(_p(t) for t in bufs), (gs,)


def _attn_args(who: str, q: Tensor, cache, pos: Tensor, out: Tensor, rows: bool = False):
    """what every decode-attention front (`who`) asks of (q, cache, pos, out): tensors on the device, dense int64 positions, the cache of _attn_cache — of the
    positions' batch, or with rows=True ONE sequence's, the positions being R rows of it —, and dense q / out [B, n_heads * hd] of the cache's dtype.
    Returns (B, n_heads) and _attn_cache's tuple."""
    _dev(q, pos, out, *_dense(cache))
    B = _batch_of(pos, who)
    c = _attn_cache(who, cache, None if rows else B)
    hd, dt = c[2], c[3]
    if hd < 1 or q.numel() % (B * hd) or out.numel() != q.numel() or not q.is_contiguous() or not out.is_contiguous() or q.dtype != dt or out.dtype != dt:
        raise ValueError(f"hqq_amd: {who} takes dense q / out [{'R' if rows else 'B'}, n_heads * head_dim] of the cache's dtype")
    return B, q.numel() // (B * hd), c


def attn_splits(kv_len: int) -> int:
    """how many workgroups share a head's keys in the decode-attention kernel when up to kv_len of them are visible (1: no second launch)"""
    return 1 if kv_len <= 1024 else min(16, int(kv_len) // 512)


def attn_workspace_batched(device, batch: int, n_heads: int, head_dim: int, splits: int):
    """the (uninitialised) record buffer of a split launch for `batch` sequences (hqq_hip_attn_decode_workspace_bytes(batch * n_heads, ...)), or None"""
    nb = int(_C.lib().hqq_hip_attn_decode_workspace_bytes(int(batch) * int(n_heads), int(head_dim), int(splits)))
    return torch.empty(nb, dtype=torch.uint8, device=device) if nb else None


def attn_workspace(device, n_heads: int, head_dim: int, splits: int):
    """attn_workspace_batched for one sequence"""
    return attn_workspace_batched(device, 1, n_heads, head_dim, splits)


def _split_workspace(workspace, splits: int, device, rows: int, n_heads: int, head_dim: int):
    """(pointer, bytes, tensor) of the record buffer a decode-attention launch is given: the caller's, or for splits > 1 without one a fresh
    attn_workspace_batched(device, rows, ...) — the tensor is returned so that the allocation lives until the launch is queued"""
    if splits > 1 and workspace is None:
        workspace = attn_workspace_batched(device, rows, n_heads, head_dim, splits)
    return _p(workspace), 0 if workspace is None else workspace.numel(), workspace


def _attn_front(symbol: str, who: str, q: Tensor, cache, pos: Tensor, out: Tensor, scaling: float, splits: int, workspace, rows: bool = False) -> Tensor:
    """the one front of the decode-attention calls on (q, cache, pos, out) — public function `who`, library entry point `symbol`; cache and rows as in
    _attn_args: the checks, the record buffer of a split launch, the call"""
    B, n_heads, (n_kv, L, hd, dt, head, ptrs, gs) = _attn_args(who, q, cache, pos, out, rows)
    ws_ptr, ws_bytes, _ws = _split_workspace(workspace, splits, q.device, B, n_heads, hd)
    with torch.cuda.device(q.device):
        rc = getattr(_C.lib(), symbol)(*head, _p(q), *ptrs, _p(pos), B, _p(out), n_heads, n_kv, hd, *gs, L, float(scaling), _dt(dt), int(splits), ws_ptr, ws_bytes, _stream())
    _C.check(rc, symbol)
    return out


def attn_decode_batched(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, out: Tensor, scaling: float, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """one query per head and sequence against the static KV caches, B sequences in one launch (fp16 / bf16; within rounding of SDPA, not bit-identical):
    q / out [B, n_heads * hd] (any dense view of those values), caches [B, n_kv, cache_len, hd], pos int64 [B] on the device; sequence b attends over its own first
    pos[b] + 1 keys.  splits > 1: the keys of a head shared out over that many workgroups + a merging launch (long caches; attn_splits / attn_workspace_batched).
    splits is one for the whole launch (pick it from the largest position): a sequence with fewer visible keys than splits
    leaves the surplus shares empty, and the merging launch ignores them"""
    return _attn_front("hqq_hip_attn_decode_batched", "attn_decode_batched", q, (k_cache, v_cache), pos, out, scaling, splits, workspace)


def attn_decode(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, out: Tensor, scaling: float, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_batched for one sequence: q [n_heads, hd] (any dense view of n_heads * hd values), k_cache / v_cache [n_kv, cache_len, hd], pos int64[1], out [n_heads * hd]"""
    return attn_decode_batched(q, _cache1(k_cache), _cache1(v_cache), _seq1(pos), out, scaling, splits=splits, workspace=workspace)


def rope_attn_decode_batched(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor, v_cache: Tensor, out: Tensor, scaling: float,
                             splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """rope_cache_batched + attn_decode_batched in one launch: raw q [B, n_heads * hd], k / v [B, n_kv * hd], cos / sin [B, hd]; rotary applied in the kernel, each
    sequence's new key / value used from on-chip memory and written to its own cache row at pos[b] for the following steps (the caches end up bit-identical to
    rope_cache_batched's); splits as in attn_decode_batched"""
    _dev(k, v, cos, sin)
    B, n_heads, (n_kv, L, hd, *_) = _attn_args("rope_attn_decode_batched", q, (k_cache, v_cache), pos, out)
    if cos.numel() != B * hd or sin.numel() != B * hd or k.numel() != B * n_kv * hd or v.numel() != k.numel() or \
            not all(t.is_contiguous() for t in (k, v, cos, sin)):
        raise ValueError("hqq_amd: rope_attn_decode_batched takes dense k / v [B, n_kv_heads * head_dim] and cos / sin [B, head_dim]")
    ws_ptr, ws_bytes, _ws = _split_workspace(workspace, splits, q.device, B, n_heads, hd)
    with torch.cuda.device(q.device):
        rc = _C.lib().hqq_hip_rope_attn_decode_batched(_p(q), _p(k), _p(v), _p(cos), _p(sin), _p(pos), B, _p(k_cache), _p(v_cache), _p(out), n_heads, n_kv, hd, L,
                                                       float(scaling), _dt(q.dtype), int(splits), ws_ptr, ws_bytes, _stream())
    _C.check(rc, "hqq_hip_rope_attn_decode_batched")
    return out


def rope_attn_decode(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor, v_cache: Tensor, out: Tensor, scaling: float,
                     splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """rope_attn_decode_batched for one sequence: cos / sin [hd], caches [n_kv, cache_len, hd], pos int64[1]"""
    return rope_attn_decode_batched(q, k, v, cos, sin, _seq1(pos), _cache1(k_cache), _cache1(v_cache), out, scaling, splits=splits, workspace=workspace)


# ---- speculative greedy decoding (csrc/block.hip's *_shared entry points, csrc/spec.hip; include/hqq_hip.h hqq_hip_spec_*): R rows that are R consecutive
#      positions of ONE sequence on its batch-1 cache, the n-gram proposer in front of them and the accept / commit step behind ----------------------------
SPEC_MAX_ROWS = 16     # rows of a verify step (the decode linears' GEMV_MAX_M)
SPEC_MAX_NGRAM = 4


def _shared_cache(who: str, k_cache: Tensor, v_cache: Tensor):
    """one sequence's caches [n_kv, L, hd] or [1, n_kv, L, hd] (a batch-1 StaticCache's tensors): (n_kv, L, hd)"""
    if k_cache.dim() not in (3, 4) or (k_cache.dim() == 4 and k_cache.shape[0] != 1) or v_cache.shape != k_cache.shape or not k_cache.is_contiguous() or \
            not v_cache.is_contiguous() or v_cache.dtype != k_cache.dtype:
        raise ValueError(f"hqq_amd: {who} takes ONE sequence's dense caches [n_kv_heads, cache_len, head_dim] (or [1, ...]) of one dtype")
    return tuple(int(x) for x in k_cache.shape[-3:])


def rope_cache_shared(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, k_cache: Tensor, v_cache: Tensor, q_out: Tensor) -> Tensor:
    """rope_cache_batched for R rows of ONE sequence (hqq_hip_rope_cache_shared): q / q_out [R, n_heads * hd], k / v [R, n_kv * hd], cos / sin [R, hd], pos int64
    [R]; the caches are that sequence's [n_kv, L, hd] (or [1, n_kv, L, hd]).  Row i's rotated key and its value go to slot pos[i], q_out[i] has the bits of the
    batch-1 rope_cache call; a position outside the cache writes nothing.  The positions of a call must be distinct: equal ones leave that slot unspecified."""
    _dev(q, k, v, cos, sin, pos, k_cache, v_cache, q_out)
    R = _batch_of(pos, "rope_cache_shared")
    n_kv, L, hd = _shared_cache("rope_cache_shared", k_cache, v_cache)
    n_heads = _qkv_extents("rope_cache_shared", R, n_kv, hd, q, k, v, q_out, cos, sin, dt=k_cache.dtype, R="R", tail=" of the caches' dtype")
    with torch.cuda.device(q.device):
        rc = _C.lib().hqq_hip_rope_cache_shared(_p(q), _p(k), _p(v), _p(cos), _p(sin), _p(pos), R, _p(q_out), _p(k_cache), _p(v_cache), n_heads, n_kv, hd, L, _dt(q.dtype), _stream())
    _C.check(rc, "hqq_hip_rope_cache_shared")
    return q_out


def attn_decode_shared(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, out: Tensor, scaling: float, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_batched for R queries of ONE sequence against that sequence's caches [n_kv, L, hd] (or [1, n_kv, L, hd]) (hqq_hip_attn_decode_shared): q / out
    [R, n_heads * hd], pos int64 [R]; row i attends over keys [0, pos[i]] and is bit-identical to attn_decode with row i's query and position and the same
    splits.  Splits and workspace as attn_decode_batched at R rows (attn_workspace_batched(device, R, ...))."""
    return _attn_front("hqq_hip_attn_decode_shared", "attn_decode_shared", q, (k_cache, v_cache), pos, out, scaling, splits, workspace, rows=True)


def attn_decode_tiled(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, out: Tensor, scaling: float, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_shared's arguments and semantics through the kernel that reads each key ONCE for all R <= 16 rows (hqq_hip_attn_decode_tiled, csrc/attn_tile.hip):
    one workgroup per (head, split), the rows as one MFMA tile, flash-decoding over blocks of 32 keys.  Its own contract: deterministic, row i independent of the
    other rows' queries, within a derived band of float64 attention (tests/_tile_cases.py) — NOT bit-identical to attn_decode.  Splits and workspace as
    attn_decode_shared (attn_workspace_batched(device, R, ...))."""
    return _attn_front("hqq_hip_attn_decode_tiled", "attn_decode_tiled", q, (k_cache, v_cache), pos, out, scaling, splits, workspace, rows=True)


def _i64_dev(who: str, **tensors) -> None:
    for name, t in tensors.items():
        if not isinstance(t, Tensor) or t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError(f"hqq_amd: {who} takes `{name}` as a dense int64 tensor on the device")


def spec_propose(hist: Tensor, p: Tensor, tok: Tensor, pos: Tensor, ngram_max: int = 3) -> None:
    """The n-gram proposer of speculative decoding, one workgroup (hqq_hip_spec_propose).  hist int64 [cap]: the sequence's tokens; p: a device int64 scalar, the index
    of the last committed one.  Writes tok / pos (int64, R = 2..16 elements each): tok[0] = hist[p], pos[i] = p + i, tok[1:] the continuation of the latest earlier
    occurrence of the longest n-gram (n <= ngram_max <= 4) the history ends with, extended periodically; hist[p] everywhere when nothing matches.  Graph-replay safe."""
    _dev(hist, p, tok, pos)
    _i64_dev("spec_propose", hist=hist, p=p, tok=tok, pos=pos)
    R = pos.numel()
    if hist.dim() != 1 or p.numel() != 1 or tok.numel() != R or not 2 <= R <= SPEC_MAX_ROWS or isinstance(ngram_max, bool) or not isinstance(ngram_max, int) or \
            not 0 <= ngram_max <= SPEC_MAX_NGRAM:
        raise ValueError(f"hqq_amd: spec_propose takes a 1-D history, a scalar p, tok / pos of 2..{SPEC_MAX_ROWS} elements each and ngram_max in 0..{SPEC_MAX_NGRAM}")
    with torch.cuda.device(hist.device):
        rc = _C.lib().hqq_hip_spec_propose(_p(hist), hist.numel(), _p(p), R, ngram_max, _p(tok), _p(pos), _stream())
    _C.check(rc, "hqq_hip_spec_propose")


def spec_accept(g: Tensor, tok: Tensor, hist: Tensor, p: Tensor, last: Tensor, eos: Tensor, done: Tensor, steps: Tensor, tokens: Tensor) -> None:
    """The accept / commit step of speculative decoding, one wave (hqq_hip_spec_accept).  g / tok int64 of R = 2..16 elements: the rows' argmax and what the rows
    were fed; hist int64 [cap]; p, last, eos, done, steps, tokens: device int64 scalars (last: the index of the last token to emit; eos: -1 for none).  Frozen
    (done != 0 or p >= last): nothing changes.  Otherwise the longest prefix of drafts the model confirms — tok[i] == g[i - 1] —, cut at `last` and at the first
    EOS (done = 1), is committed: hist[p + 1 + i] = g[i] for i = 0..a, p += a + 1, steps += 1, tokens += a + 1.  Graph-replay safe."""
    _dev(g, tok, hist, p, last, eos, done, steps, tokens)
    _i64_dev("spec_accept", g=g, tok=tok, hist=hist, p=p, last=last, eos=eos, done=done, steps=steps, tokens=tokens)
    R = g.numel()
    if hist.dim() != 1 or tok.numel() != R or not 2 <= R <= SPEC_MAX_ROWS or any(t.numel() != 1 for t in (p, last, eos, done, steps, tokens)):
        raise ValueError(f"hqq_amd: spec_accept takes g / tok of 2..{SPEC_MAX_ROWS} elements each, a 1-D history and scalar p / last / eos / done / steps / tokens")
    with torch.cuda.device(hist.device):
        rc = _C.lib().hqq_hip_spec_accept(_p(g), _p(tok), R, _p(hist), hist.numel(), _p(p), _p(last), _p(eos), _p(done), _p(steps), _p(tokens), _stream())
    _C.check(rc, "hqq_hip_spec_accept")


# ---- the quantised static KV cache (csrc/kv_cache.hip; include/hqq_hip.h states the format).  `bufs` is a layer's six buffers in the order
#      (kq, k_scale, k_zero, vq, v_scale, v_zero): kq / vq [B, n_kv, L, head_dim * nbits / 8] uint8, the four meta tensors [B, n_kv, L, head_dim / gs] of the
#      compute dtype; nbits and the group size are read off their shapes against head_dim ----------------------------------------------------------------------
KV_MAX_LEN = 30000   # the decode-attention kernels' limit on cache positions


def kv_group_size(head_dim: int) -> int:
    """the default group size of a quantised cache row: 64, or 32 when head_dim is 64"""
    return 32 if int(head_dim) == 64 else 64


def kv_covers(dtype, nbits, head_dim: int, group_size, cache_len: int = 1) -> bool:
    """what the quantised-cache kernels serve (pure host arithmetic): fp16 / bf16, nbits 8 / 4, head_dim 64 / 128 / 256, group_size 32 / 64 dividing head_dim with
    2 * group_size <= head_dim at 4 bits, 1 <= cache_len <= 30000"""
    if dtype not in (torch.float16, torch.bfloat16) or isinstance(nbits, bool) or not isinstance(nbits, int) or not isinstance(group_size, int):
        return False
    return bool(_C.lib().hqq_hip_kv_covers(int(nbits), int(head_dim), int(group_size), int(cache_len), _DT[dtype]))


def kv_alloc(B: int, n_kv: int, L: int, head_dim: int, nbits: int, group_size: int, dtype, device) -> tuple:
    """a layer's six buffers, zeroed (level 0, scale 0 and zero 0 dequantise to 0: an unwritten position holds finite values, as a zeroed dense cache does)"""
    if not kv_covers(dtype, nbits, head_dim, group_size, L):
        raise ValueError(f"hqq_amd: no quantised KV cache for dtype {dtype}, nbits {nbits}, head_dim {head_dim}, group_size {group_size}, {L} positions (ops.kv_covers)")
    lv = lambda: torch.zeros(B, n_kv, L, head_dim * nbits // 8, dtype=torch.uint8, device=device)   # noqa: E731
    mt = lambda: torch.zeros(B, n_kv, L, head_dim // group_size, dtype=dtype, device=device)        # noqa: E731
    return (lv(), mt(), mt(), lv(), mt(), mt())


def _kv_bufs(bufs, head_dim: int, who: str):
    """the six buffers checked against each other and head_dim.  Returns (B, n_kv, L, nbits, group_size, dtype)."""
    if len(bufs) != 6 or not all(isinstance(t, Tensor) for t in bufs):
        raise ValueError(f"hqq_amd: {who} takes the six cache buffers (kq, k_scale, k_zero, vq, v_scale, v_zero)")
    kq, ks, kz, vq, vs, vz = bufs
    _dev(*bufs)
    if kq.dim() != 4 or kq.dtype != torch.uint8 or vq.dtype != torch.uint8 or vq.shape != kq.shape or ks.dim() != 4 or any(t.shape != ks.shape or t.dtype != ks.dtype for t in (kz, vs, vz)) or \
            ks.shape[:3] != kq.shape[:3] or not all(t.is_contiguous() for t in bufs) or kq.shape[3] < 1 or ks.shape[3] < 1:
        raise ValueError(f"hqq_amd: {who} takes dense uint8 level buffers [B, n_kv_heads, cache_len, head_dim * nbits / 8] and four dense meta tensors "
                         "[B, n_kv_heads, cache_len, head_dim / group_size] of one dtype")
    B, n_kv, L, rb = (int(s) for s in kq.shape)
    G = int(ks.shape[3])
    hd = int(head_dim)
    if hd < 1 or hd % G or rb * 8 % hd or rb * 8 // hd not in (8, 4):
        raise ValueError(f"hqq_amd: {who}: buffers of {rb} bytes and {G} groups per row do not hold rows of {hd} values at 8 or 4 bits")
    nbits, gs = rb * 8 // hd, hd // G
    if not kv_covers(ks.dtype, nbits, hd, gs, L):
        raise NotImplementedError(f"hqq_amd: {who}: not covered: dtype {ks.dtype}, nbits {nbits}, head_dim {hd}, group_size {gs}, {L} positions (ops.kv_covers)")
    return B, n_kv, L, nbits, gs, ks.dtype


def kv_quantize(k: Tensor, v: Tensor, bufs, start=0) -> None:
    """rows k, v [B, n_kv, T, head_dim] (any strides over the first three dimensions that are multiples of 8 elements; head_dim dense) quantised into positions
    p .. p + T - 1 of the six buffers.  start: a host integer p (0 <= p, p + T <= L), or an int64 device tensor — one element: p for every sequence; B elements:
    p[b] for sequence b (graph-replay safe; a position outside [0, L) writes nothing).  Nothing but the addressed positions is written."""
    _dev(k, v)
    if k.dim() != 4 or k.shape[3] < 1:
        raise ValueError("hqq_amd: kv_quantize takes k / v [B, n_kv_heads, T, head_dim]")
    B, n_kv, L, nbits, gs, dt = _kv_bufs(bufs, k.shape[3], "kv_quantize")
    if v.shape != k.shape or k.dtype != dt or v.dtype != dt or tuple(k.shape[:2]) != (B, n_kv) or k.shape[2] < 1 or k.shape[2] > L or \
            (k.shape[3] > 1 and (k.stride(3) != 1 or v.stride(3) != 1)):
        raise ValueError("hqq_amd: kv_quantize takes k / v [B, n_kv_heads, T, head_dim] of the buffers' dtype and batch, 1 <= T <= cache_len, head_dim dense")
    T = int(k.shape[2])
    pos, stride, p0 = None, 0, 0
    if isinstance(start, Tensor):
        _dev(start)
        if start.dtype != torch.int64 or start.numel() not in (1, B) or not start.is_contiguous():
            raise ValueError("hqq_amd: kv_quantize's device positions are a dense int64 tensor of 1 or B elements")
        pos, stride = start, (1 if start.numel() == B and B > 1 else 0)
    else:
        p0 = int(start)
        if p0 < 0 or p0 + T > L:
            raise ValueError(f"hqq_amd: kv_quantize: positions {p0} .. {p0 + T - 1} outside a cache of {L}")
    with torch.cuda.device(k.device):
        rc = _C.lib().hqq_hip_kv_quantize(nbits, _p(k), _p(v), _i64s(k.stride()[:3]), _i64s(v.stride()[:3]), B, n_kv, T, int(k.shape[3]), gs, p0, _p(pos), stride,
                                          *(_p(t) for t in bufs), L, _dt(dt), _stream())
    _C.check(rc, "hqq_hip_kv_quantize")


def kv_dequantize(bufs, head_dim: int, n: int | None = None, out=None):
    """positions 0 .. n - 1 (default: all) of the six buffers as dense tensors (k, v) [B, n_kv, n, head_dim] of the compute dtype: round(round(q - zero) * scale)
    per element, Quantizer.dequantize's two roundings.  out: a pair of dense tensors of that shape to fill."""
    B, n_kv, L, nbits, gs, dt = _kv_bufs(bufs, head_dim, "kv_dequantize")
    n = L if n is None else int(n)
    if n < 1 or n > L:
        raise ValueError(f"hqq_amd: kv_dequantize: n = {n} outside [1, {L}]")
    shape = (B, n_kv, n, int(head_dim))
    if out is None:
        out = (torch.empty(shape, dtype=dt, device=bufs[0].device), torch.empty(shape, dtype=dt, device=bufs[0].device))
    ko, vo = out
    _dev(ko, vo)
    if tuple(ko.shape) != shape or tuple(vo.shape) != shape or ko.dtype != dt or vo.dtype != dt or not ko.is_contiguous() or not vo.is_contiguous():
        raise ValueError(f"hqq_amd: kv_dequantize's outputs are two dense tensors {shape} of the buffers' dtype")
    with torch.cuda.device(ko.device):
        rc = _C.lib().hqq_hip_kv_dequantize(nbits, *(_p(t) for t in bufs), B, n_kv, L, n, int(head_dim), gs, _p(ko), _p(vo), _dt(dt), _stream())
    _C.check(rc, "hqq_hip_kv_dequantize")
    return ko, vo


def rope_kvq_cache_batched(q: Tensor, k: Tensor, v: Tensor, cos: Tensor, sin: Tensor, pos: Tensor, bufs, q_out: Tensor) -> Tensor:
    """rope_cache_batched with a quantised cache write, one launch: q_out [B, n_heads * hd] = rotary(q) (rope_cache_batched's bits); rotary(k) and v
    ([B, n_kv * hd]) are quantised on chip and stored at position pos[b] of sequence b's rows of the six buffers — the bits of rope_cache_batched into a dense
    cache followed by kv_quantize of that row; a position outside the cache writes nothing"""
    _dev(q, k, v, cos, sin, pos, q_out)
    B = _batch_of(pos, "rope_kvq_cache_batched")
    hd = cos.numel() // B
    Bc, n_kv, L, nbits, gs, dt = _kv_bufs(bufs, hd, "rope_kvq_cache_batched")
    if Bc != B:
        raise ValueError(f"hqq_amd: rope_kvq_cache_batched takes buffers of the positions' batch ({Bc} sequences against {B} positions)")
    n_heads = _qkv_extents("rope_kvq_cache_batched", B, n_kv, hd, q, k, v, q_out, cos, sin, dt=dt, tail=" of the buffers' dtype")
    with torch.cuda.device(q.device):
        rc = _C.lib().hqq_hip_rope_kvq_cache_batched(nbits, _p(q), _p(k), _p(v), _p(cos), _p(sin), _p(pos), B, _p(q_out), *(_p(t) for t in bufs), n_heads, n_kv, hd, gs, L,
                                                     _dt(dt), _stream())
    _C.check(rc, "hqq_hip_rope_kvq_cache_batched")
    return q_out


def attn_decode_kvq_batched(q: Tensor, bufs, pos: Tensor, out: Tensor, scaling: float, head_dim: int, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_batched on a quantised cache: q / out [B, n_heads * hd], the six buffers, pos int64 [B] on the device; every row is rebuilt to the compute dtype
    as it is loaded and the rest is attn_decode_batched's arithmetic in its order — the output has the bits of attn_decode_batched on kv_dequantize's tensors with
    the same splits.  Nothing at or beyond pos[b] + 1 is read.  splits / workspace as in attn_decode_batched (attn_workspace_batched)."""
    return _attn_front("hqq_hip_attn_decode_kvq_batched", "attn_decode_kvq_batched", q, (bufs, head_dim), pos, out, scaling, splits, workspace)


def attn_decode_kvq(q: Tensor, bufs, pos: Tensor, out: Tensor, scaling: float, head_dim: int, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_kvq_batched for one sequence: buffers [n_kv, cache_len, ...] (or [1, n_kv, cache_len, ...]), pos int64[1]"""
    return attn_decode_kvq_batched(q, tuple(t.view(1, *t.shape[-3:]) for t in bufs), _seq1(pos), out, scaling, head_dim, splits=splits, workspace=workspace)


# ---- decode attention with one workgroup per KV-head GROUP (csrc/attn_gqa.hip): the arguments of attn_decode_batched / attn_decode_kvq_batched through the kernel
#      that makes the G = n_heads / n_kv_heads query heads of a group one MFMA query tile, so each key is read — and a packed key rebuilt — once per group.
#      Its contract is attn_decode_tiled's (deterministic, a head independent of the other heads' queries, within tests/_tile_cases.py's band of float64
#      attention), NOT attn_decode_batched's bits ---------------------------------------------------------------------------------------------------------------
ATTN_MAX_SPLITS = 64   # csrc/attn_decode_core.h
ATTN_GQA_MAX_G = 16    # the rows of the query tile
ATTN_GQA_SPLITS_CAP = 32   # attn_gqa_splits never asks for more (measured: profiles/gqa_attn_summary.md)


def attn_gqa_covers(n_heads: int, n_kv_heads: int) -> bool:
    """whether the grouped kernels have something to share and a tile to hold it: 2 <= n_heads / n_kv_heads <= 16 (pure host arithmetic)"""
    n_heads, n_kv_heads = int(n_heads), int(n_kv_heads)
    return n_kv_heads >= 1 and n_heads >= 1 and n_heads % n_kv_heads == 0 and 2 <= n_heads // n_kv_heads <= ATTN_GQA_MAX_G


def attn_gqa_splits(kv_len: int, batch: int, n_kv_heads: int) -> int:
    """how many workgroups share a KV group's keys in the grouped kernels when up to kv_len of them are visible.  The grouped grid has G times fewer workgroups
    than the per-head one, so attn_splits is not its rule: the smallest S with batch * n_kv_heads * S >= 256 (a workgroup per CU), capped by kv_len // 256 (every
    wave of a share gets a block of 32 keys), by ATTN_GQA_SPLITS_CAP = 32 and by ATTN_MAX_SPLITS, never below 1.  The cap of 32 is the sweep's correction: at 64
    shares the per-share fixed cost and the merging launch cost more than the idle CUs they fill (28 / 4 heads, B = 1, 16384 positions: 41.9 us dense at 64 shares
    against 29.4 at 32).  With it the rule's time is within 11 % of the best split count measured at every point of profiles/gqa_attn_summary.md, which holds the
    table.  A function of (kv_len, batch, n_kv_heads) alone, so a captured graph keeps its launch shape per bucket as with attn_splits."""
    groups = max(1, int(batch) * int(n_kv_heads))
    want = -(-256 // groups)
    return max(1, min(want, int(kv_len) // 256, ATTN_GQA_SPLITS_CAP, ATTN_MAX_SPLITS))


def attn_decode_gqa_batched(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, out: Tensor, scaling: float, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_batched's arguments through the grouped kernel (hqq_hip_attn_decode_gqa_batched): grid (n_kv, splits, B), the query heads of a KV group as one
    MFMA tile.  n_heads / n_kv_heads up to 16.  Splits and workspace as attn_decode_batched (attn_gqa_splits / attn_workspace_batched)."""
    return _attn_front("hqq_hip_attn_decode_gqa_batched", "attn_decode_gqa_batched", q, (k_cache, v_cache), pos, out, scaling, splits, workspace)


def attn_decode_gqa(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos: Tensor, out: Tensor, scaling: float, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_gqa_batched for one sequence: q [n_heads, hd], k_cache / v_cache [n_kv, cache_len, hd], pos int64[1], out [n_heads * hd]"""
    return attn_decode_gqa_batched(q, _cache1(k_cache), _cache1(v_cache), _seq1(pos), out, scaling, splits=splits, workspace=workspace)


def attn_decode_gqa_kvq_batched(q: Tensor, bufs, pos: Tensor, out: Tensor, scaling: float, head_dim: int, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_kvq_batched's arguments through the grouped kernel (hqq_hip_attn_decode_gqa_kvq_batched): a packed row is rebuilt once per KV group; the output
    has the bits of attn_decode_gqa_batched on kv_dequantize's tensors with the same splits.  Nothing at or beyond pos[b] + 1 is read."""
    return _attn_front("hqq_hip_attn_decode_gqa_kvq_batched", "attn_decode_gqa_kvq_batched", q, (bufs, head_dim), pos, out, scaling, splits, workspace)


def attn_decode_gqa_kvq(q: Tensor, bufs, pos: Tensor, out: Tensor, scaling: float, head_dim: int, splits: int = 1, workspace: Tensor | None = None) -> Tensor:
    """attn_decode_gqa_kvq_batched for one sequence: buffers [n_kv, cache_len, ...] (or [1, n_kv, cache_len, ...]), pos int64[1]"""
    return attn_decode_gqa_kvq_batched(q, tuple(t.view(1, *t.shape[-3:]) for t in bufs), _seq1(pos), out, scaling, head_dim, splits=splits, workspace=workspace)


# ---- a prompt's causal attention on the static cache (csrc/attn_prefill.hip): the T rows of ONE sequence at positions pos0 .. pos0 + T - 1, row t over keys
#      [0, pos0 + t] of a cache that already holds the rows' own keys and values.  Grid (n_heads, ceil(T / 16)): 16 consecutive positions of a query head are one
#      MFMA query tile of attn_decode_tiled's body, one share, no workspace.  The contract, pinned by tests/test_prefill_attn_gpu.py:
#        (a) rows 16 j .. of head h have the bits of attn_decode_tiled on those queries with pos = pos0 + 16 j + i and splits = 1
#        (b) every row lies within tests/_tile_cases.py's band of float64 attention
#        (c) attn_prefill_kvq has the bits of attn_prefill on kv_dequantize's tensors
#        (d) nothing at or beyond pos0 + T is read, in levels, meta or dense rows: it may hold NaN
#        (e) row i depends on no query of a row > i and on no FINITE key / value at a position > pos0 + i (a masked V row inside the tile's range is still
#            multiplied, by an exact 0)
#        (f) the same bits call to call, and whatever q's strides
#        (g) NOT the bits of SDPA: the probabilities are rounded to the tensors' dtype before the product with V, and the keys are blocked
#      Tiles are per query head (the heads of a KV group re-read its rows), 16 rows, one sequence per call ------------------------------------------------------
def _prefill_q(who: str, q: Tensor, pos0, L: int, hd: int, dt, out):
    """q [T, n_heads, hd] with a dense last dimension (any strides of the other two that are multiples of 8 elements) against a cache of L positions of hd values
    of dtype dt: (T, n_heads, pos0, out), out allocated [T, n_heads, hd] where None"""
    if q.dim() != 3 or q.shape[0] < 1 or q.shape[1] < 1 or q.shape[2] != hd or q.stride(2) != 1 or q.stride(0) % 8 or q.stride(1) % 8:
        raise ValueError(f"hqq_amd: {who} takes q [T, n_heads, head_dim] with T >= 1, the caches' head_dim, a dense last dimension and row / head strides that are "
                         "multiples of 8 elements")
    if dt not in (torch.float16, torch.bfloat16) or q.dtype != dt:
        raise ValueError(f"hqq_amd: {who} takes fp16 / bf16 tensors of one dtype (q {q.dtype}, the cache {dt})")
    T, n_heads = int(q.shape[0]), int(q.shape[1])
    if isinstance(pos0, bool) or not isinstance(pos0, int) or pos0 < 0 or pos0 + T > L:
        raise ValueError(f"hqq_amd: {who}: rows at positions pos0 .. pos0 + T - 1 (pos0 = {pos0!r}, a host integer >= 0; T = {T}) do not fit a cache of {L}")
    if out is None:
        out = torch.empty(T, n_heads, hd, dtype=dt, device=q.device)
    elif out.dtype != dt or out.numel() != T * n_heads * hd or not out.is_contiguous():
        raise ValueError(f"hqq_amd: {who} takes out as a dense [T, n_heads, head_dim] tensor of q's dtype")
    return T, n_heads, pos0, out


def _prefill_front(symbol: str, who: str, q: Tensor, cache, pos0, out, scaling) -> Tensor:
    """the one front of the prompt calls — public function `who`, library entry point `symbol`, ONE sequence's cache as in _attn_cache"""
    _dev(q, out, *_dense(cache))
    n_kv, L, hd, dt, head, ptrs, gs = _attn_cache(who, cache, None)
    T, n_heads, pos0, out = _prefill_q(who, q, pos0, L, hd, dt, out)
    with torch.cuda.device(q.device):
        rc = getattr(_C.lib(), symbol)(*head, _p(q), q.stride(0), q.stride(1), *ptrs, pos0, T, _p(out), n_heads, n_kv, hd, *gs, L,
                                       float(hd ** -0.5 if scaling is None else scaling), _dt(dt), _stream())
    _C.check(rc, symbol)
    return out.view(T, n_heads, hd)


def attn_prefill(q: Tensor, k_cache: Tensor, v_cache: Tensor, pos0: int, out: Tensor | None = None, scaling: float | None = None) -> Tensor:
    """Causal attention of a prompt's T rows on ONE sequence's dense static cache (hqq_hip_attn_prefill, csrc/attn_prefill.hip).  q [T, n_heads, hd]: any view
    with a dense last dimension — HF's [1, H, T, hd] query goes in as query[0].transpose(0, 1), through its strides, without a copy; k_cache / v_cache
    [n_kv, L, hd] or [1, n_kv, L, hd], already holding the rows' keys and values at positions pos0 .. pos0 + T - 1; pos0 a host integer.  Row t attends over keys
    [0, pos0 + t].  Returns out [T, n_heads, hd] (dense; allocated when None), the layout o_proj takes.  scaling: hd ** -0.5 when None.
    fp16 / bf16, hd 64 / 128 / 256, n_heads a multiple of n_kv, L <= 30000.  A prompt that does not fit the cache is a ValueError (no clamping).
    Contract (a) - (g) above: per 16-row tile the bits of attn_decode_tiled (splits = 1), within tests/_tile_cases.py's band of float64 attention, nothing at or
    beyond pos0 + T read, exactly causal, deterministic and independent of q's strides — and NOT the bits of SDPA."""
    return _prefill_front("hqq_hip_attn_prefill", "attn_prefill", q, (k_cache, v_cache), pos0, out, scaling)


def attn_prefill_kvq(q: Tensor, bufs, pos0: int, head_dim: int, out: Tensor | None = None, scaling: float | None = None) -> Tensor:
    """attn_prefill on ONE sequence's quantised cache (hqq_hip_attn_prefill_kvq): the six buffers [n_kv, L, ...] (or [1, n_kv, L, ...]), which already hold the
    rows' quantised keys and values; every attended row is rebuilt to the compute dtype as it is loaded and the rest is attn_prefill's arithmetic in its order —
    the output has the bits of attn_prefill on kv_dequantize's tensors (contract (c)), and no full-length dequantised tensor exists.  Nothing at or beyond
    pos0 + T is read, in levels or in meta.  Covered where ops.kv_covers holds (NotImplementedError otherwise)."""
    return _prefill_front("hqq_hip_attn_prefill_kvq", "attn_prefill_kvq", q, (bufs, head_dim), pos0, out, scaling)


def argmax_advance_batched(logits: Tensor, next_tok: Tensor, tok: Tensor | None = None, pos: Tensor | None = None) -> None:
    """The back of a greedy decode step for B sequences in one launch, one workgroup per row (hqq_hip_argmax_advance_batched): next_tok[b] = logits[b].argmax() (the first
    index of the largest value; torch.argmax's tie and NaN rule), tok[b] = the same, pos[b] += 1 (each skipped when None).  logits [B, vocab] dense; int64 tensors of
    B elements on the device: graph-replay safe."""
    _dev(logits, next_tok)
    B = next_tok.numel()
    if logits.dim() != 2 or logits.shape[0] != B or not logits.is_contiguous() or next_tok.dtype != torch.int64 or not next_tok.is_contiguous() or \
            any(t is not None and (t.dtype != torch.int64 or t.numel() != B or not t.is_contiguous()) for t in (tok, pos)):
        raise ValueError("hqq_amd: argmax_advance_batched takes dense logits [B, vocab] and dense int64 token / position tensors of B elements")
    with torch.cuda.device(logits.device):
        rc = _C.lib().hqq_hip_argmax_advance_batched(_p(logits), B, logits.shape[1], _dt(logits.dtype), _p(next_tok), _p(tok), _p(pos), _stream())
    _C.check(rc, "hqq_hip_argmax_advance_batched")


def argmax_advance(logits: Tensor, next_tok: Tensor, tok: Tensor | None = None, pos: Tensor | None = None) -> None:
    """argmax_advance_batched for one sequence: logits of any dense shape holding one row, next_tok / tok [1, 1], pos [1]"""
    argmax_advance_batched(logits.view(1, -1), next_tok, tok, _seq1(pos))


def silu_mul(gate: Tensor, up: Tensor, out: Tensor | None = None) -> Tensor:
    """LlamaMLP's act_fn(gate) * up in one kernel (fp16 / bf16; n a multiple of 8): silu in fp32, x / (1 + exp(-x)), rounded to the dtype, then the product in the
    dtype.  The fp32 formula's range is kept: a gate below about -88.72 gives -0 (exp overflows), -inf gives NaN — torch's own result."""
    _dev(gate, up)
    if out is None:
        out = torch.empty_like(gate)
    with torch.cuda.device(gate.device):
        rc = _C.lib().hqq_hip_silu_mul(_p(gate), _p(up), _p(out), gate.numel(), _dt(gate.dtype), _stream())
    _C.check(rc, "hqq_hip_silu_mul")
    return out


# ---- the routed expert MLP of a mixture-of-experts block (csrc/moe.hip; include/hqq_hip.h hqq_hip_moe_*) ---------------------------------------------
MOE_MAX_T = 16         # tokens one call takes (hqq_hip_moe_covers)
# The largest token count at which HQQExperts takes the fused route on its own (fused=None).  The project's cut-off rule: the largest T <= MOE_MAX_T such that,
# at it and at every smaller measured T, the two launches are at least 10 % ahead of the composed route on every shape, configuration and routing of
# tools/moe_bench.py.  profiles/moe_summary.md: ahead everywhere up to T = 4; at T = 8 Mixtral's shape with every token on the same two experts is 1.10 (int4,
# below the 10 %), at T = 16 the composed route wins there (0.57): the kernel rebuilds an expert's weights once per (token, slot), the composed route once per expert.
# A graph capture cannot take the composed route (it reads the routing on the host): capture at most MOE_ROUTE_MAX_T tokens, or set HQQExperts.fused = True.
MOE_ROUTE_MAX_T = 4


def moe_covers(dtype, T: int, k: int, E: int, H: int, I: int, group_size, nbits, axis: int = 1) -> bool:
    """what hqq_hip_moe_gate_up / hqq_hip_moe_down serve (pure host arithmetic): experts quantised along axis 1 at 4 or 2 bits, fp16 / bf16,
    1..16 tokens, 1..8 experts per token, up to 256 experts, H and I multiples of 64, group_size a multiple of 16 that divides both"""
    if axis != 1 or dtype not in (torch.float16, torch.bfloat16) or not group_size or nbits not in (8, 4, 3, 2, 1):
        return False
    return bool(_C.lib().hqq_hip_moe_covers(int(nbits), int(T), int(k), int(E), int(H), int(I), int(group_size), _DT[dtype]))


def _moe_stack(who: str, layer, E: int, N: int, K: int, group_size: int, nbits: int, dtype):
    """one role's stacks (W_q [E, ...] uint8, scale [E, ...], zero [E, ...]) checked against the sizes the kernel reads through raw pointers"""
    W_q, scale, zero = layer
    _dev(W_q, scale, zero)
    groups = N * K // group_size
    if W_q.dtype != torch.uint8 or W_q.numel() != E * N * K // PER[nbits] or scale.numel() != E * groups or zero.numel() != E * groups:
        raise ValueError(f"hqq_amd: {who} takes stacks of {E} experts of a {N} x {K} layer: {E * N * K // PER[nbits]} packed bytes and {E * groups} scale / zero values")
    if scale.dtype != dtype or zero.dtype != dtype:
        raise TypeError("hqq_amd: x / scale / zero must share the compute dtype")
    if not (W_q.is_contiguous() and scale.is_contiguous() and zero.is_contiguous()):
        raise ValueError(f"hqq_amd: {who} takes dense (contiguous) expert stacks")
    return W_q, scale, zero


def _moe_routing(who: str, idx: Tensor, weights, T: int):
    _dev(idx, weights)
    if idx.dtype != torch.int64 or idx.dim() != 2 or idx.shape[0] != T or not idx.is_contiguous():
        raise ValueError(f"hqq_amd: {who} takes top_k_index [T, k] int64, contiguous")
    if weights is not None and (weights.dtype != torch.float32 or weights.shape != idx.shape or not weights.is_contiguous()):
        raise ValueError(f"hqq_amd: {who} takes top_k_weights [T, k] float32, contiguous")
    return int(idx.shape[1])


def moe_gate_up(x: Tensor, idx: Tensor, gate, up, E: int, H: int, I: int, group_size: int, nbits: int, a: Tensor | None = None) -> Tensor:
    """a[t, s] = act_fn(gate_e(x_t)) * up_e(x_t), e = idx[t, s] read on the device (hqq_hip_moe_gate_up).  gate / up: (W_q, scale, zero) stacks over the
    E experts.  Returns a [T, k, I] (the caller's buffer when given).  The part of `a` that belongs to an id outside [0, E) is left unwritten."""
    _dev(x)
    if x.dim() != 2 or x.shape[1] != H or not x.is_contiguous():
        raise ValueError(f"hqq_amd: moe_gate_up takes hidden_states [T, {H}], contiguous")
    T = int(x.shape[0])
    k = _moe_routing("moe_gate_up", idx, None, T)
    g = _moe_stack("moe_gate_up", gate, E, I, H, group_size, nbits, x.dtype)
    u = _moe_stack("moe_gate_up", up, E, I, H, group_size, nbits, x.dtype)
    if a is None:
        a = torch.empty((T, k, I), dtype=x.dtype, device=x.device)
    elif a.dtype != x.dtype or a.numel() != T * k * I or not a.is_contiguous() or not a.is_cuda:
        raise ValueError(f"hqq_amd: moe_gate_up's buffer must be [T, k, I] = [{T}, {k}, {I}] of the compute dtype, contiguous")
    with torch.cuda.device(x.device):
        rc = _C.lib().hqq_hip_moe_gate_up(int(nbits), _p(x), _p(idx), _p(g[0]), _p(g[1]), _p(g[2]), _p(u[0]), _p(u[1]), _p(u[2]), _p(a), T, k, int(E), int(H),
                                          int(I), int(group_size), _dt(x.dtype), _stream())
    _C.check(rc, "hqq_hip_moe_gate_up")
    return a


def moe_down(a: Tensor, idx: Tensor, weights: Tensor, down, E: int, H: int, I: int, group_size: int, nbits: int, out: Tensor | None = None) -> Tensor:
    """out[t] = the token's slots s in ascending (expert, slot): out[t] += (down_e(a[t, s]) * weights[t, s]).to(dtype) (hqq_hip_moe_down): the combine in the
    launch's epilogue, in the order of HF's loop over the experts hit.  Returns out [T, H]."""
    _dev(a)
    T = int(idx.shape[0]) if idx.dim() == 2 else -1
    k = _moe_routing("moe_down", idx, weights, T)
    if a.numel() != T * k * I or not a.is_contiguous():
        raise ValueError(f"hqq_amd: moe_down takes a [T, k, I] = [{T}, {k}, {I}], contiguous")
    d = _moe_stack("moe_down", down, E, H, I, group_size, nbits, a.dtype)
    if out is None:
        out = torch.empty((T, H), dtype=a.dtype, device=a.device)
    elif out.dtype != a.dtype or out.numel() != T * H or not out.is_contiguous() or not out.is_cuda:
        raise ValueError(f"hqq_amd: moe_down's output must be [T, H] = [{T}, {H}] of the compute dtype, contiguous")
    with torch.cuda.device(a.device):
        rc = _C.lib().hqq_hip_moe_down(int(nbits), _p(a), _p(idx), _p(weights), _p(d[0]), _p(d[1]), _p(d[2]), _p(out), T, k, int(E), int(H), int(I),
                                       int(group_size), _dt(a.dtype), _stream())
    _C.check(rc, "hqq_hip_moe_down")
    return out


def moe_router_covers(dtype, T: int, k: int, E: int, H: int) -> bool:
    """what hqq_hip_moe_router serves (pure host arithmetic): fp16 / bf16, 1..16 rows, 1..8 experts per token, k..256 experts, H a multiple of 8 up to 65536"""
    if dtype not in (torch.float16, torch.bfloat16):
        return False
    return bool(_C.lib().hqq_hip_moe_router_covers(int(T), int(k), int(E), int(H), _DT[dtype]))


def moe_router(x: Tensor, weight: Tensor, k: int, renorm: bool = True, round_weights: bool = False, idx: Tensor | None = None, weights: Tensor | None = None,
               logits: Tensor | None = None):
    """a router's whole forward in one launch (hqq_hip_moe_router): logits = x @ weight.T rounded to the compute dtype, softmax in fp32, the k largest LOGITS
    in descending order with equal logits by ascending expert id (this library's own rule: torch.topk leaves the order among equal values open), their
    probabilities, divided by their sum with `renorm` (Mixtral always; Qwen3-MoE's norm_topk_prob) and rounded to the compute dtype with `round_weights`
    (Qwen3-MoE).  x [T, H] and weight [E, H] dense, of one dtype.  Returns (idx [T, k] int64, weights [T, k] float32) — what moe_gate_up / moe_down read —
    in the caller's buffers when given; `logits` [T, E] of the compute dtype is filled when given."""
    _dev(x, weight, idx, weights, logits)
    if x.dim() != 2 or weight.dim() != 2 or weight.shape[1] != x.shape[1] or not x.is_contiguous() or not weight.is_contiguous():
        raise ValueError("hqq_amd: moe_router takes hidden_states [T, H] and a router weight [E, H], contiguous")
    if weight.dtype != x.dtype:
        raise TypeError("hqq_amd: x and the router weight must share the compute dtype")
    T, H, E, k = int(x.shape[0]), int(x.shape[1]), int(weight.shape[0]), int(k)
    if idx is None:
        idx = torch.empty((T, k), dtype=torch.int64, device=x.device)
    if weights is None:
        weights = torch.empty((T, k), dtype=torch.float32, device=x.device)
    if tuple(idx.shape) != (T, k) or tuple(weights.shape) != (T, k):
        raise ValueError(f"hqq_amd: moe_router's idx and weights must be [T, k] = [{T}, {k}]")
    _moe_routing("moe_router", idx, weights, T)
    if logits is not None and (logits.dtype != x.dtype or tuple(logits.shape) != (T, E) or not logits.is_contiguous()):
        raise ValueError(f"hqq_amd: moe_router's logits must be [T, E] = [{T}, {E}] of the compute dtype, contiguous")
    with torch.cuda.device(x.device):
        rc = _C.lib().hqq_hip_moe_router(_p(x), _p(weight), _p(idx), _p(weights), _p(logits), T, k, E, H, int(bool(renorm)), int(bool(round_weights)),
                                         _dt(x.dtype), _stream())
    _C.check(rc, "hqq_hip_moe_router")
    return idx, weights


def moe_forward(x: Tensor, idx: Tensor, weights: Tensor, gate, up, down, E: int, H: int, I: int, group_size: int, nbits: int,
                a: Tensor | None = None, out: Tensor | None = None) -> Tensor:
    """the experts module's forward in two launches (moe_gate_up, moe_down): no host read of the routing, nothing allocated but `out` and `a` when the
    caller gives none — a step a graph can capture"""
    a = moe_gate_up(x, idx, gate, up, E, H, I, group_size, nbits, a=a)
    return moe_down(a, idx, weights, down, E, H, I, group_size, nbits, out=out)
