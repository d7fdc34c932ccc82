"""The caller-owned workspace contract of every split-K route (include/hqq_hip.h "Workspace"), exercised at the raw C ABI as an outside caller
would: the workspace is EXACTLY the bytes the query returned, fenced by guard bands (tests/_ws_arena.py), its body NaN-poisoned, its counter
head zero (the skinny GEMV) or a sentinel (every route documented to keep out of it).  Per case:
  (a) both guards byte-identical afterwards, the head zero again / untouched;
  (b) the output finite;
  (c) the output bit-identical to the same call through hqq_amd.ops (one zero-filled, oversized, shared workspace) — every route sums in a
      fixed order, so no tolerance applies;
  (d) on the flagged cases the clean call against an fp64 matmul on hqq_hip_dequantize's weights, with the tolerance of the route's own oracle
      test (test_skinny_gemm_vs_oracle / _bf16_, test_gemv_3bit_slab_sharing_kernel, test_pipelined_gemm_vs_oracle / _bf16, test_gemv_axis0_vs_oracle,
      test_decode_attention_with_the_keys_shared_out_over_workgroups).
No out-of-bounds write of up to twice the size can leave the arena's allocation."""
import pytest
import torch

import _ws_cases as W
from test_hip_parity import assert_forward_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import ops as o
    assert o.is_available(), "libhqq_hip.so must load on the GPU box (no fallback)"
    return o


@pytest.fixture(scope="module")
def L():
    from hqq_amd import _C
    return _C.lib()


def _seed(c):
    return sum(map(ord, c.id)) % 100003


def _checked_case(L, c):
    """a planner change must not turn a case into a no-op: the intended route, and partial sums behind the head"""
    assert W.route(L, c) == W.WANT_ROUTE[c.kind], L.hqq_hip_last_error()
    need = W.need(L, c)
    assert need > W.HEAD
    return need


def _assert_vs_fp64(c, y, x, Wd, bias):
    """the clean output against fp64 accumulation over the dequantise kernel's weights, rounded as the kernels round: once to the dtype, once
    more for the bias add"""
    dt = W.DT[c.dt]
    acc = (x.double() @ Wd.double().t()).to(dt)
    want = (acc if bias is None else acc + bias).float()
    y = y.float()
    if c.kind == "skinny" and c.dt == "f16":      # test_skinny_gemm_vs_oracle's own check
        return assert_forward_parity(y, want, c.id)
    err = (y - want).abs()
    if c.kind == "pipe" and c.dt == "f16":      # test_pipelined_gemm_vs_oracle
        tol = 2e-3 + 1e-3 * want.abs()
    elif c.kind == "pipe":                        # test_pipelined_gemm_bf16: one bf16 ulp of the result BEFORE the bias add
        tol = 2.0 ** -7 * (want.abs() + (0 if bias is None else bias.float().abs()[None, :])) + 2e-3
    elif c.dt == "f16":                           # test_gemv_3bit_slab_sharing_kernel, test_gemv_axis0_vs_oracle
        tol = 1e-3 + 1e-3 * want.abs()
    else:                                         # test_skinny_gemm_bf16_vs_oracle, test_gemv_axis0_vs_oracle (bf16)
        tol = 2e-3 + 2.0 ** -7 * want.abs()
    bad = err > tol
    assert not bool(bad.any()), f"{c.id}: {int(bad.sum())} of {bad.numel()} outside the route's tolerance, worst {float((err - tol).max()):.3e} over"


@pytest.mark.parametrize("c", W.CASES, ids=lambda c: c.id)
def test_exact_workspace(ops, L, c):
    need = _checked_case(L, c)
    x, layers, Wd = W.operands(ops, c, _seed(c))
    if c.opts & W.META_SCALABLE:
        assert all(ops.meta_scalable(s.reshape(-1), z.reshape(-1), N, c.K, 64, c.nbits) for (_, s, z, _, N) in layers)
    a = W.arena(need, c.head_fill)
    outs = W.new_outputs(c)
    rc = W.call_raw(L, c, x, layers, outs, a.ptr, a.need)
    assert rc == 0, L.hqq_hip_last_error()
    a.check(c.id)                                                                        # (a)
    for o in outs:
        assert bool(torch.isfinite(o).all()), f"{c.id}: {int((~torch.isfinite(o)).sum())} outputs are not finite"   # (b)
    clean = W.call_clean(ops, c, x, layers)
    for i, (o, want) in enumerate(zip(outs, clean)):                                     # (c)
        assert W.same_bits(o, want.reshape(o.shape)), f"{c.id}: layer {i}: {int((o != want.reshape(o.shape)).sum())} outputs differ from the clean call"
    if c.fp64:                                                                           # (d)
        assert not c.flags
        for (Wq, s, z, b, N), y, wd in zip(layers, clean, Wd):
            _assert_vs_fp64(c, y.reshape(c.M, N), x, wd, b)


# ---- one arena, every route in turn ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(ops, L):
    """the five calls' operands and what each gives run alone on a fresh exact arena"""
    out = []
    for c in W.MIXED:
        need = _checked_case(L, c)
        x, layers, _ = W.operands(ops, c, _seed(c))
        a = W.arena(need, c.head_fill)
        alone = W.new_outputs(c)
        assert W.call_raw(L, c, x, layers, alone, a.ptr, a.need) == 0, L.hqq_hip_last_error()
        a.check(c.id)
        assert all(bool(torch.isfinite(o).all()) for o in alone)
        out.append((c, need, x, layers, alone))
    return out


@pytest.mark.parametrize("ia,ib", W.MIXED_PAIRS, ids=lambda i: W.MIXED[i].kind + ("g" if W.MIXED[i].grouped else ""))
def test_routes_alternate_on_one_workspace(L, mixed, ia, ib):
    """one model, one buffer: B after A on the same workspace, nothing re-poisoned in between — B's bits are those of B alone (on its own
    exact arena), and the counter head reads zero after each call.  The buffer is sized for the LARGEST of the five calls and every call is
    given that size, so the smaller routes run oversized here; exact sizes are test_exact_workspace's and the `alone` baselines'.  The head is
    zero, as the skinny GEMV needs it: a route that wrongly wrote zeros there would pass here and is caught by test_exact_workspace's sentinel head."""
    a = W.arena(max(m[1] for m in mixed), 0)
    for i in (ia, ib):
        c, need, x, layers, alone = mixed[i]
        outs = W.new_outputs(c)
        assert W.call_raw(L, c, x, layers, outs, a.ptr, a.need) == 0, L.hqq_hip_last_error()
        a.check(f"{c.id} ({'first' if i == ia else 'second'} of the pair)")
        if i == ib:
            for o, want in zip(outs, alone):
                assert W.same_bits(o, want), f"{c.id} after {mixed[ia][0].id}: {int((o != want).sum())} outputs differ from the call run alone"


# ---- "a larger workspace than asked for is fine"; a smaller one is refused ---------------------------------------------------------------
@pytest.mark.parametrize("c", W.SIZE_CASES, ids=lambda c: c.id)
def test_larger_is_fine_smaller_is_refused(ops, L, c):
    need = _checked_case(L, c)
    x, layers, _ = W.operands(ops, c, _seed(c))
    clean = W.call_clean(ops, c, x, layers)
    a = W.arena(need + 4096, c.head_fill)
    outs = W.new_outputs(c)
    assert W.call_raw(L, c, x, layers, outs, a.ptr, a.need) == 0, L.hqq_hip_last_error()
    a.check(c.id)
    for o, want in zip(outs, clean):
        assert W.same_bits(o, want.reshape(o.shape))
    # sixteen bytes short: refused before anything is launched
    a = W.arena(need, c.head_fill)
    outs = W.new_outputs(c, fill=7.0)
    assert W.call_raw(L, c, x, layers, outs, a.ptr, need - 16) == W.ERR_WORKSPACE
    assert b"workspace" in L.hqq_hip_last_error()
    a.check(c.id)
    assert bool((a.body == W.BODY_BYTE).all()) and all(bool((o == 7.0).all()) for o in outs)


# ---- the record buffer of the split decode attention ----------------------------------------------------------------------------------
def _attn_operands(c, seed):
    dt = W.DT[c.dt]
    B = len(c.pos)
    g = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *shape: torch.randn(*shape, device="cuda", generator=g).to(dt)   # noqa: E731
    t = {"q": r(B, c.n_heads * c.hd), "k": r(B, c.n_kv * c.hd), "v": r(B, c.n_kv * c.hd), "kc": r(B, c.n_kv, c.L, c.hd), "vc": r(B, c.n_kv, c.L, c.hd)}
    ang = torch.rand(B, c.hd // 2, device="cuda", generator=g) * 6.28
    t["cos"], t["sin"] = torch.cat([ang.cos(), ang.cos()], -1).to(dt).contiguous(), torch.cat([ang.sin(), ang.sin()], -1).to(dt).contiguous()
    t["pos"] = torch.tensor(c.pos, device="cuda", dtype=torch.int64)
    for b, p in enumerate(c.pos):      # nothing past the visible keys may be read (rotary form: the new key / value come from the call)
        t["kc"][b, :, p + (0 if c.rope else 1):] = float("nan")
        t["vc"][b, :, p + (0 if c.rope else 1):] = float("nan")
    return t


def _attn_raw(L, c, t, kc, vc, out, ws_ptr, ws_bytes):
    st = torch.cuda.current_stream().cuda_stream
    B, p = len(c.pos), lambda n: t[n].data_ptr()   # noqa: E731
    tail = (c.n_heads, c.n_kv, c.hd, c.L, c.hd ** -0.5, W.CODE[c.dt], c.splits, ws_ptr, ws_bytes, st)
    if c.rope:
        head = (p("q"), p("k"), p("v"), p("cos"), p("sin"), p("pos"))
        if c.batched:
            return L.hqq_hip_rope_attn_decode_batched(*head, B, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), *tail)
        return L.hqq_hip_rope_attn_decode(*head, kc.data_ptr(), vc.data_ptr(), out.data_ptr(), *tail)
    if c.batched:
        return L.hqq_hip_attn_decode_batched(p("q"), kc.data_ptr(), vc.data_ptr(), p("pos"), B, out.data_ptr(), *tail)
    return L.hqq_hip_attn_decode(p("q"), kc.data_ptr(), vc.data_ptr(), p("pos"), out.data_ptr(), *tail)


def _attn_clean(ops, c, t, kc, vc, out, ws):
    sc = c.hd ** -0.5
    if c.rope and c.batched:
        return ops.rope_attn_decode_batched(t["q"], t["k"], t["v"], t["cos"], t["sin"], t["pos"], kc, vc, out, sc, splits=c.splits, workspace=ws)
    if c.rope:
        return ops.rope_attn_decode(t["q"], t["k"], t["v"], t["cos"], t["sin"], t["pos"], kc[0], vc[0], out, sc, splits=c.splits, workspace=ws)
    if c.batched:
        return ops.attn_decode_batched(t["q"], kc, vc, t["pos"], out, sc, splits=c.splits, workspace=ws)
    return ops.attn_decode(t["q"], kc[0], vc[0], t["pos"], out, sc, splits=c.splits, workspace=ws)


@pytest.mark.parametrize("c", W.ATTN_CASES, ids=lambda c: c.id)
def test_attention_record_buffer_exact(ops, L, c):
    need = W.attn_need(L, c)
    assert need > 0
    t = _attn_operands(c, _seed(c))
    B = len(c.pos)
    a = W.arena(need, None)
    kc, vc = t["kc"].clone(), t["vc"].clone()
    out = torch.full((B, c.n_heads * c.hd), float("nan"), dtype=W.DT[c.dt], device="cuda")
    assert _attn_raw(L, c, t, kc, vc, out, a.ptr, a.need) == 0, L.hqq_hip_last_error()
    a.check(c.id)
    assert bool(torch.isfinite(out).all())
    # the clean call: a zero-filled, oversized record buffer
    kc2, vc2 = t["kc"].clone(), t["vc"].clone()
    out2 = torch.empty_like(out)
    _attn_clean(ops, c, t, kc2, vc2, out2, torch.zeros(need + (1 << 20), dtype=torch.uint8, device="cuda"))
    assert W.same_bits(out, out2), f"{c.id}: {int((out != out2).sum())} outputs differ from the clean call"
    for b, p in enumerate(c.pos):
        assert torch.equal(kc[b, :, :p + 1], kc2[b, :, :p + 1]) and torch.equal(vc[b, :, :p + 1], vc2[b, :, :p + 1])
    # fp64 softmax attention over the visible keys (the rotary form: over what hqq_hip_rope_cache writes, and its rotated query)
    q = t["q"].view(B, c.n_heads, c.hd)
    if c.rope:
        kc3, vc3 = t["kc"].clone(), t["vc"].clone()
        q = torch.empty_like(t["q"])
        ops.rope_cache_batched(t["q"], t["k"], t["v"], t["cos"], t["sin"], t["pos"], kc3, vc3, q)
        q = q.view(B, c.n_heads, c.hd)
        for b, p in enumerate(c.pos):
            assert torch.equal(kc2[b, :, :p + 1], kc3[b, :, :p + 1]) and torch.equal(vc2[b, :, :p + 1], vc3[b, :, :p + 1])
    rep = c.n_heads // c.n_kv
    ulp = 2.0 ** -10 if c.dt == "f16" else 2.0 ** -7
    for b, p in enumerate(c.pos):
        kk = kc2[b, :, :p + 1].repeat_interleave(rep, 0).double()
        vv = vc2[b, :, :p + 1].repeat_interleave(rep, 0).double()
        want = torch.einsum("hj,hjd->hd", torch.softmax(torch.einsum("hd,hjd->hj", q[b].double(), kk) * c.hd ** -0.5, -1), vv)
        tol = 1e-3 + 1e-3 * want.abs() + want.abs() * ulp
        assert bool(((out2[b].view(c.n_heads, c.hd).double() - want).abs() <= tol).all()), (c.id, b)
    # larger is fine, sixteen bytes short is refused with the entry's own code (an argument error: HQQ_ERR_SHAPE) and nothing is written
    a = W.arena(need + 4096, None)
    kc4, vc4, out4 = t["kc"].clone(), t["vc"].clone(), torch.empty_like(out)
    assert _attn_raw(L, c, t, kc4, vc4, out4, a.ptr, a.need) == 0
    a.check(c.id)
    assert W.same_bits(out4, out)
    a = W.arena(need, None)
    out5 = torch.full_like(out, 7.0)
    assert _attn_raw(L, c, t, kc4, vc4, out5, a.ptr, need - 16) == W.ERR_SHAPE
    assert b"workspace" in L.hqq_hip_last_error()
    a.check(c.id)
    assert bool((a.body == W.BODY_BYTE).all()) and bool((out5 == 7.0).all())
