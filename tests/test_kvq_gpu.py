"""GPU half of the quantised KV cache's kernel tests (csrc/kv_cache.hip through hqq_amd.ops): kv_quantize against ops.quantize(optimize=False) and the numpy
restatement of tests/_kvq_cases.py, kv_dequantize against ops.dequantize and that restatement, rope_kvq_cache_batched against rope_cache_batched followed by
kv_quantize, and attn_decode_kvq_batched against attn_decode_batched on the dequantised cache.  Every comparison is torch.equal: the format has one
definition and the attention kernel's contract is bit identity."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _attn_cases as A   # noqa: E402
import _kvq_cases as C    # noqa: E402

DT = {"f16": torch.float16, "bf16": torch.bfloat16}
CODE = {"f16": C.F16, "bf16": C.BF16}
GRID = [(hd, gs, nbits, dt) for hd, gs in C.SHAPES for nbits in (8, 4) for dt in ("f16", "bf16")]
IDS = [f"hd{hd}-gs{gs}-q{nbits}-{dt}" for hd, gs, nbits, dt in GRID]
B, N_KV, L = 3, 2, 96
SENT = 0xA5            # sentinel byte of the level buffers
SENT_META = -1234.0    # sentinel of the meta tensors (exact in fp16 and bf16)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _sentinel_bufs(hd, gs, nbits, dt, batch=B):
    from hqq_amd import ops
    bufs = ops.kv_alloc(batch, N_KV, L, hd, nbits, gs, DT[dt], "cuda")
    for i, t in enumerate(bufs):
        t.fill_(SENT if i in (0, 3) else SENT_META)
    return bufs


def _rows(hd, gs, nbits, dt, shape, seed):
    """dense rows of T [*shape, hd]: the special rows of _kvq_cases (constant, tiny-range, clamped, one-signed groups) among randn ones"""
    n = int(np.prod(shape))
    sp = C.special_rows(hd, gs, nbits, CODE[dt], seed)
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(n, hd, generator=g) * 2.0).to(DT[dt])
    k = min(n, sp.shape[0])
    spt = torch.from_numpy(sp[:k].view(np.int16).copy()).view(DT[dt])
    x[torch.randperm(n, generator=g)[:k]] = spt
    return x.view(*shape, hd).cuda()


def _levels(q, nbits):
    """stored bytes [..., hd * nbits / 8] -> levels [..., hd]"""
    return q if nbits == 8 else torch.cat([q >> 4, q & 0xF], dim=-1)


def _reference(x, gs, nbits):
    """ops.quantize(optimize=False) on the same rows: levels [..., hd] (unpacked: a whole-tensor call pairs bytes differently), scale and zero [..., hd / gs] cast to T"""
    from hqq_amd import ops
    hd = x.shape[-1]
    Wq, sc, ze = ops.quantize(x.reshape(-1, gs), nbits=nbits, group_size=gs, round_zero=False, optimize=False)
    lv = ops.unpack(nbits, Wq)[: x.numel() // gs]
    return lv.view(*x.shape), sc.to(x.dtype).view(*x.shape[:-1], hd // gs), ze.to(x.dtype).view(*x.shape[:-1], hd // gs)


@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_kv_quantize_equals_ops_quantize_and_touches_nothing_else(hd, gs, nbits, dt):
    from hqq_amd import ops
    T, start = 7, 5
    k = _rows(hd, gs, nbits, dt, (B, T, N_KV), 1).transpose(1, 2)     # a strided source, as HF hands its key / value states over
    v = _rows(hd, gs, nbits, dt, (B, N_KV, T), 2)
    bufs = _sentinel_bufs(hd, gs, nbits, dt)
    ops.kv_quantize(k, v, bufs, start=start)
    for src, (q, s, z) in ((k, bufs[:3]), (v, bufs[3:])):
        lv, sc, ze = _reference(src.contiguous(), gs, nbits)
        assert torch.equal(_levels(q[:, :, start:start + T], nbits), lv)
        assert torch.equal(_bits(s[:, :, start:start + T]), _bits(sc)) and torch.equal(_bits(z[:, :, start:start + T]), _bits(ze))
        # the numpy restatement, on the same rows
        x_np = src.contiguous().view(torch.int16).cpu().numpy().view(np.uint16).reshape(-1, hd)
        nl, ns, nz = C.quantize_rows(x_np if dt == "bf16" else x_np.view(np.float16), CODE[dt], nbits, gs)
        assert np.array_equal(q[:, :, start:start + T].cpu().numpy().reshape(-1, hd * nbits // 8), C.pack_rows(nl, nbits))
        assert np.array_equal(_bits(s[:, :, start:start + T]).cpu().numpy().view(np.uint16).reshape(-1, hd // gs), np.asarray(ns).view(np.uint16))
        assert np.array_equal(_bits(z[:, :, start:start + T]).cpu().numpy().view(np.uint16).reshape(-1, hd // gs), np.asarray(nz).view(np.uint16))
        # sentinels before and after the addressed positions survive
        for lo, hi in ((0, start), (start + T, L)):
            assert bool((q[:, :, lo:hi] == SENT).all()) and bool((s[:, :, lo:hi] == SENT_META).all()) and bool((z[:, :, lo:hi] == SENT_META).all())
    # the same positions from ONE device position for every sequence (the composed route's form): the same buffers
    again = _sentinel_bufs(hd, gs, nbits, dt)
    ops.kv_quantize(k, v, again, start=torch.tensor([start], device="cuda"))
    assert all(torch.equal(_bits(a) if a.dtype != torch.uint8 else a, _bits(b) if b.dtype != torch.uint8 else b) for a, b in zip(again, bufs))


@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_kv_quantize_at_device_positions(hd, gs, nbits, dt):
    """T = 1 at pos[b]: sequence b's row lands at its own position, a position outside [0, L) writes nothing, every other byte keeps its sentinel"""
    from hqq_amd import ops
    k, v = _rows(hd, gs, nbits, dt, (B, N_KV, 1), 3), _rows(hd, gs, nbits, dt, (B, N_KV, 1), 4)
    for positions in ((3, L - 1, 0), (L, 17, -1), (2 ** 40, -2 ** 40, L + 1)):
        bufs = _sentinel_bufs(hd, gs, nbits, dt)
        ops.kv_quantize(k, v, bufs, start=torch.tensor(positions, device="cuda"))
        want = _sentinel_bufs(hd, gs, nbits, dt)
        for b, p in enumerate(positions):
            if 0 <= p < L:
                one = tuple(t[b:b + 1] for t in want)
                ops.kv_quantize(k[b:b + 1], v[b:b + 1], one, start=int(p))   # (the host-start form, checked against ops.quantize above)
        for got, exp in zip(bufs, want):
            assert torch.equal(got if got.dtype == torch.uint8 else _bits(got), exp if exp.dtype == torch.uint8 else _bits(exp))
        wrote = sum(0 <= p < L for p in positions)
        assert int((bufs[0] != SENT).any(dim=-1).sum()) <= wrote * N_KV


@functools.lru_cache(maxsize=None)
def _filled(hd, gs, nbits, dt):
    """a full cache of B sequences: dense rows, their six buffers, and the dequantised dense tensors — computed once, shared, never modified"""
    from hqq_amd import ops
    k, v = _rows(hd, gs, nbits, dt, (B, N_KV, L), 5), _rows(hd, gs, nbits, dt, (B, N_KV, L), 6)
    bufs = ops.kv_alloc(B, N_KV, L, hd, nbits, gs, DT[dt], "cuda")
    ops.kv_quantize(k, v, bufs, start=0)
    return k, v, bufs, ops.kv_dequantize(bufs, hd)


@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_kv_dequantize_equals_ops_dequantize_and_the_restatement(hd, gs, nbits, dt):
    from hqq_amd import ops
    _, _, bufs, (kd, vd) = _filled(hd, gs, nbits, dt)
    G = hd // gs
    for (q, s, z), dense in ((bufs[:3], kd), (bufs[3:], vd)):
        lv = _levels(q, nbits).cpu().numpy().reshape(-1, hd)
        sn, zn = (_bits(t).cpu().numpy().view(np.uint16).reshape(-1, G) for t in (s, z))
        if dt == "f16":
            sn, zn = sn.view(np.float16), zn.view(np.float16)
        want = np.asarray(C.dequantize_rows(lv, sn, zn, CODE[dt], gs)).view(np.uint16)
        assert np.array_equal(_bits(dense).cpu().numpy().view(np.uint16).reshape(-1, hd), want)
        for b, h, p in ((0, 0, 0), (1, 1, 41), (2, 0, L - 1), (2, 1, 7)):   # Quantizer.dequantize on a row's own packed [hd / gs, gs] level matrix
            row = ops.dequantize(q[b, h, p].view(-1, gs), s[b, h, p].view(G, 1), z[b, h, p].view(G, 1), 1, hd, gs, nbits)
            assert torch.equal(_bits(row.view(-1)), _bits(dense[b, h, p]))
    kn, vn = ops.kv_dequantize(bufs, hd, n=40)
    assert tuple(kn.shape) == (B, N_KV, 40, hd) and torch.equal(_bits(kn), _bits(kd[:, :, :40])) and torch.equal(_bits(vn), _bits(vd[:, :, :40]))


def _angles(hd, positions, dt):
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    ang = torch.tensor(positions, dtype=torch.float32).clamp(0, 4096)[:, None] * inv[None, :]
    emb = torch.cat([ang, ang], dim=-1)
    return emb.cos().to(DT[dt]).cuda(), emb.sin().to(DT[dt]).cuda()


@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_rope_kvq_cache_equals_rope_cache_then_kv_quantize(hd, gs, nbits, dt):
    from hqq_amd import ops
    n_heads = 4
    q, k, v = (_rows(hd, gs, nbits, dt, (B, n), s).view(B, -1) for n, s in ((n_heads, 7), (N_KV, 8), (N_KV, 9)))
    for positions in ((0, 41, L - 1), (L, 5, -1)):
        cos, sin = _angles(hd, positions, dt)
        pos = torch.tensor(positions, device="cuda")
        kc, vc = (torch.zeros(B, N_KV, L, hd, dtype=DT[dt], device="cuda") for _ in range(2))
        q_ref = ops.rope_cache_batched(q, k, v, cos, sin, pos, kc, vc, torch.empty_like(q))
        bufs = _sentinel_bufs(hd, gs, nbits, dt)
        q_out = ops.rope_kvq_cache_batched(q, k, v, cos, sin, pos, bufs, torch.empty_like(q))
        assert torch.equal(_bits(q_out), _bits(q_ref))
        want = _sentinel_bufs(hd, gs, nbits, dt)
        idx = pos.clamp(0, L - 1).view(B, 1, 1, 1).expand(B, N_KV, 1, hd)
        ops.kv_quantize(kc.gather(2, idx), vc.gather(2, idx), want, start=pos)   # the dense kernel's rows, at the same positions (outside the cache: nothing)
        for got, exp in zip(bufs, want):   # the whole buffers: the stored rows, and every neighbouring position untouched
            assert torch.equal(got if got.dtype == torch.uint8 else _bits(got), exp if exp.dtype == torch.uint8 else _bits(exp))
        assert int((bufs[0] != SENT).any(dim=-1).sum()) <= sum(0 <= p < L for p in positions) * N_KV


def _positions(hd):
    """the key places tests/_attn_cases.py probes in a cache of L keys (both sides of the last multiples of STEP and 4 STEP, first, last, middle) and the
    visible-key counts it runs the split launches at, as positions"""
    ps = set(A.places(L, hd)) | {n - 1 for S in (3, 64) for n in A.split_ns(S) if n <= L}
    return sorted(ps)


def _poisoned(bufs, positions):
    """copies of the buffers with 0xFF levels and NaN meta beyond each sequence's position"""
    out = tuple(t.clone() for t in bufs)
    for b, p in enumerate(positions):
        for i, t in enumerate(out):
            t[b, :, p + 1:] = 0xFF if i in (0, 3) else float("nan")
    return out


@pytest.mark.parametrize("rep", [2, 1])
@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_attn_decode_kvq_has_the_bits_of_attn_decode_on_the_dequantised_cache(hd, gs, nbits, dt, rep):
    from hqq_amd import ops
    _, _, bufs, _ = _filled(hd, gs, nbits, dt)
    n_heads = N_KV * rep
    q = (torch.randn(B, n_heads * hd, generator=torch.Generator().manual_seed(11)) * 0.5).to(DT[dt]).cuda()
    scaling = hd ** -0.5
    ps = _positions(hd)
    triples = [(ps[i], ps[(i + 5) % len(ps)], ps[(2 * i + 3) % len(ps)]) for i in range(len(ps))]
    for splits in (1, 3, 64):   # (64: more shares than visible keys at most positions: the surplus shares are empty)
        for positions in triples:
            pb = _poisoned(bufs, positions)
            kd, vd = ops.kv_dequantize(pb, hd)
            pos = torch.tensor(positions, device="cuda")
            want = ops.attn_decode_batched(q, kd, vd, pos, torch.empty_like(q), scaling, splits=splits)
            got = ops.attn_decode_kvq_batched(q, pb, pos, torch.empty_like(q), scaling, hd, splits=splits)
            assert bool(torch.isfinite(got.float()).all()), (splits, positions)
            assert torch.equal(_bits(got), _bits(want)), (splits, positions)
    # the same bits call to call, and a batch row equals its one-row call
    positions = triples[1]
    pos = torch.tensor(positions, device="cuda")
    pb = _poisoned(bufs, positions)
    for splits in (1, 3):
        a = ops.attn_decode_kvq_batched(q, pb, pos, torch.empty_like(q), scaling, hd, splits=splits)
        b2 = ops.attn_decode_kvq_batched(q, pb, pos, torch.empty_like(q), scaling, hd, splits=splits)
        assert torch.equal(_bits(a), _bits(b2))
        for b in range(B):
            one = ops.attn_decode_kvq(q[b], tuple(t[b] for t in pb), pos[b:b + 1], torch.empty_like(q[b]), scaling, hd, splits=splits)
            assert torch.equal(_bits(one), _bits(a[b]))


def test_the_wrappers_refuse_what_the_kernels_do_not_cover():
    from hqq_amd import ops
    with pytest.raises(ValueError):
        ops.kv_alloc(1, 2, L, 128, 4, 128, torch.float16, "cuda")
    bufs = ops.kv_alloc(1, 2, L, 64, 8, 32, torch.float16, "cuda")
    x = torch.zeros(1, 2, 4, 64, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError):
        ops.kv_quantize(x, x, bufs, start=L - 3)                      # runs past the cache
    with pytest.raises(ValueError):
        ops.kv_quantize(x.bfloat16(), x.bfloat16(), bufs, start=0)    # another dtype than the buffers'
    with pytest.raises(ValueError):
        ops.kv_quantize(x, x, bufs[:5], start=0)
    with pytest.raises(ValueError):
        ops.kv_dequantize(bufs, 64, n=L + 1)
    with pytest.raises(ValueError):
        ops.kv_dequantize(bufs, 96)                                   # 64-byte rows hold no 96 values at 8 or 4 bits
    q = torch.zeros(1, 4 * 64, dtype=torch.float16, device="cuda")
    pos = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):              # a caller-provided workspace that is too small: the library's own check
        ops.attn_decode_kvq_batched(q, bufs, pos, torch.empty_like(q), 0.125, 64, splits=4, workspace=torch.empty(16, dtype=torch.uint8, device="cuda"))
