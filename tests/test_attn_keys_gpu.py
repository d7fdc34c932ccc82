"""attn_decode_kernel / attn_combine_kernel (csrc/block.hip) pinned key by key: constructed inputs in which one key decides the output
(tests/_attn_cases.py: needle, twin needles, flat scores), at every ragged tail of the one-workgroup loops, at long caches (the > 48 KiB LDS
path), at the first and last key of every share of every split count, under GQA, through the batched entries and at positions outside the cache.
Every result is compared with fp64 softmax attention over the same tensors: bit equality for a needle, one ulp of T for twins, one fp32
division plus one rounding to T for flat scores — no other tolerance.  The constructions themselves are proven on the CPU by
tests/test_attn_keys_cpu.py.  The calls go through the raw C ABI; a split launch gets a record buffer of exactly
hqq_hip_attn_decode_workspace_bytes bytes, 0xFF-filled, between guard bands (tests/_ws_arena.py)."""
import pytest
import torch

import _attn_cases as A
from _ws_arena import arena

pytestmark = pytest.mark.gpu

DTS = ("f16", "bf16")
NAN = float("nan")


@pytest.fixture(scope="module")
def L():
    assert torch.cuda.is_available(), "gpu tests need a ROCm device"
    from hqq_amd import _C
    return _C.lib()


class Kernel:
    """what A.run calls per launch: the entry point on the patched bed.  The rotary form gets cos = 1 / sin = 0, the key and value of position
    n - 1 as the raw projections and a NaN row in their place, and must leave exactly them there.  `written(bed, l, pos, k, v)`, if set, sees
    the caches as the rotary call left them, before the bed gets its row back."""

    def __init__(self, lib, rope, written=None):
        self.lib, self.rope, self.arenas, self.written = lib, rope, {}, written

    def workspace(self, bed, S, batch=1):
        if S == 1:
            return None, 0
        key = (bed.n_heads * batch, bed.hd, S)
        if key not in self.arenas:
            self.arenas[key] = arena(A.workspace_bytes(self.lib, *key), None)
        a = self.arenas[key]
        a.poison()
        return a.ptr, a.need

    def __call__(self, bed, l, pos):
        out = torch.full((bed.n_heads, bed.hd), NAN, dtype=bed.T, device="cuda")
        ws_ptr, ws_bytes = self.workspace(bed, l.S)
        kw, extra = {}, None
        if self.rope:
            k, v = bed.kc[:, l.n - 1].clone(), bed.vc[:, l.n - 1].clone()
            bed.kc[:, l.n - 1] = NAN
            bed.vc[:, l.n - 1] = NAN
            cos, sin = A.unit_angles(bed.hd, bed.T, "cuda")
            kw = dict(k=k, v=v, cos=cos, sin=sin)
        rc = A.call(self.lib, rope=self.rope, dt=bed.dt, q=bed.q, kc=bed.kc, vc=bed.vc, pos=pos, out=out, S=l.S, ws_ptr=ws_ptr, ws_bytes=ws_bytes, **kw)
        assert rc == 0, (l.id, self.lib.hqq_hip_last_error())
        if self.rope:
            extra = (A.bits(bed.kc[:, l.n - 1]) != A.bits(k)).any() | (A.bits(bed.vc[:, l.n - 1]) != A.bits(v)).any()
            if self.written is not None:
                self.written(bed, l, pos, k, v)
            bed.kc[:, l.n - 1] = k
            bed.vc[:, l.n - 1] = v
        return out, extra

    def check_arenas(self, what):
        for a in self.arenas.values():
            a.check(what)


def _run(lib, rope, dt, hd, cache_len, launches, what, **bed_kw):
    kern = Kernel(lib, rope)
    keyed, flat = [l for l in launches if l.kind != "flat"], [l for l in launches if l.kind == "flat"]
    bad = A.run(A.Bed(dt, hd, cache_len, "cuda", **bed_kw), keyed, kern)
    if flat:
        bad += A.run(A.Bed(dt, hd, cache_len, "cuda", flat=True, **bed_kw), flat, kern)
    kern.check_arenas(what)
    assert not bad, A.summary(bad, what)


@pytest.mark.parametrize("rope", [False, True], ids=["attn", "rope_attn"])
@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_one_workgroup_at_every_tail(L, dt, hd, rope):
    """splits = 1, every n = pos + 1 from 1 to 2 * 4 STEP + STEP + 1: needles at key 0, n - 1, n - 2, the middle and both sides of the last
    multiple of STEP and of 4 STEP; twins; flat scores.  The cache is as long as the longest n: the scores fit 48 KiB of LDS"""
    _run(L, rope, dt, hd, A.sweep_max_n(hd), A.sweep_launches(hd), f"sweep {dt} hd{hd} rope={rope}")


@pytest.mark.parametrize("rope", [False, True], ids=["attn", "rope_attn"])
@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_long_caches_and_every_share_edge(L, dt, hd, rope):
    """a cache of the full 30000 positions (the scores pass 48 KiB of LDS at one workgroup per head): n in LONG_NS with one workgroup, and
    S in SPLITS at n in {1, 2, S - 1, S, S + 1, 37, 1025, 4001, 20000} with a needle at the first and the last key of every non-empty share
    (every other share's maximum is lower by more than 100: e^(m_s - m) = 0), twins in two different shares (equal maxima), flat scores up
    to n = 1025, empty shares and shares that start past n"""
    launches = A.long_launches(hd) + [l for S in A.SPLITS for l in A.split_launches(hd, S)]
    _run(L, rope, dt, hd, A.MAX_L, launches, f"long / split {dt} hd{hd} rope={rope}")


@pytest.mark.parametrize("rope", [False, True], ids=["attn", "rope_attn"])
@pytest.mark.parametrize("rep", [1, 4, 8])
@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_gqa_groups_share_their_needle(L, dt, hd, rep, rope):
    """n_heads / n_kv in {1, 4, 8}, a needle per KV head: every query head of a group (the group's q times 1 or 2) returns the group's V[needle];
    the rotary form leaves both caches — compared whole, as the call left them — bit-identical to what hqq_hip_rope_cache makes of the same
    NaN-rowed caches: the new row is rope_cache's, nothing else is touched"""
    from hqq_amd import ops
    cache_len, n_kv = 2048, 2
    launches = [A.Launch("needle", n, S, a, a) for n in (2048, 1025, 300, 37, 5) for S in (1, 4) for a in ((n - 1, 0), (n // 2, n - 1), (n - 2, n // 3))]
    mismatch = []

    def written(bed, l, pos, k, v):
        kc, vc = bed.kc.clone(), bed.vc.clone()
        kc[:, l.n - 1] = NAN
        vc[:, l.n - 1] = NAN
        cos, sin = A.unit_angles(hd, bed.T, "cuda")
        ops.rope_cache(bed.q, k, v, cos, sin, pos, kc, vc, torch.empty_like(bed.q))
        mismatch.append((A.bits(kc) != A.bits(bed.kc)).any() | (A.bits(vc) != A.bits(bed.vc)).any())

    kern = Kernel(L, rope, written)
    bad = A.run(A.Bed(dt, hd, cache_len, "cuda", heads=n_kv, rep=rep), launches, kern)
    kern.check_arenas("gqa")
    assert not bad, A.summary(bad, f"gqa {dt} hd{hd} rep{rep} rope={rope}")
    if rope:
        assert not bool(torch.stack(mismatch).any()), "the caches differ from hqq_hip_rope_cache's"


@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_rotary_form_with_real_angles(L, dt, hd, S):
    """real cos / sin.  Three KV heads have their needle in the cache: C times the rotated query hqq_hip_rope_cache returns.  The fourth has it
    as the call's own new key (position pos, served from LDS): the raw key C q_raw, which the rotation turns into C rot(q_raw) up to the
    roundings of subnormal products — parallel enough to the rotated query to outscore every other key by far.  The fp64 reference is taken
    over the rotated query and the caches hqq_hip_rope_cache actually writes, and is first checked to round to V[needle]; so the output must
    equal it bit for bit.  Also bit for bit: rope_cache + attn_decode, and both caches as rope_cache leaves them"""
    from hqq_amd import ops
    n, n_kv, rep = 300, 4, 2
    bed = A.Bed(dt, hd, 512, "cuda", heads=n_kv, rep=rep)
    T = bed.T
    g = torch.Generator(device="cuda").manual_seed(hd + S)
    ang = torch.rand(hd // 2, device="cuda", generator=g) * 6.28
    cos, sin = torch.cat([ang.cos(), ang.cos()]).to(T).view(1, hd), torch.cat([ang.sin(), ang.sin()]).to(T).view(1, hd)
    pos = torch.tensor([n - 1], device="cuda")
    bed.shrink(n - 1)                                                          # row n - 1 is the call's to write
    k_raw, v_raw = torch.randn(n_kv, hd, device="cuda", generator=g).to(T), A.coded_values(n_kv, n, hd, "cuda")[:, n - 1].to(T).contiguous()
    q_group = bed.q.view(n_kv, rep, hd)[:, 0]
    k_raw[3] = (q_group[3].float() * A.C_NEEDLE).to(T)
    # the two launches it replaces, once for the rotated query, then with the cache needles in place
    kc1, vc1, qr = bed.kc.clone(), bed.vc.clone(), torch.empty_like(bed.q)
    ops.rope_cache(bed.q, k_raw, v_raw, cos, sin, pos, kc1, vc1, qr)
    needle_at = (0, 150, n - 2, n - 1)
    for kvh in range(3):
        row = (qr.view(n_kv, rep, hd)[kvh, 0].float() * A.C_NEEDLE).to(T)
        bed.kc[kvh, needle_at[kvh]] = row
        kc1[kvh, needle_at[kvh]] = row
    want = torch.empty_like(bed.q)
    ws = torch.full((A.workspace_bytes(L, bed.n_heads, hd, S) + 16,), 0xFF, dtype=torch.uint8, device="cuda")
    ops.attn_decode(qr, kc1, vc1, pos, want, bed.scaling, splits=S, workspace=ws)
    ref, _ = A.reference(qr, kc1, vc1, n, bed.scaling)
    closed = torch.stack([vc1[kvh, needle_at[kvh]] for kvh in range(n_kv)]).repeat_interleave(rep, 0)
    assert torch.equal(A.bits(ref.to(T)), A.bits(closed)), "the fp64 reference misses the closed form"
    got = torch.full_like(bed.q, NAN)
    kern = Kernel(L, True)
    ws_ptr, ws_bytes = kern.workspace(bed, S)
    rc = A.call(L, rope=True, dt=dt, q=bed.q, kc=bed.kc, vc=bed.vc, pos=pos, out=got, S=S, ws_ptr=ws_ptr, ws_bytes=ws_bytes, k=k_raw, v=v_raw, cos=cos, sin=sin)
    assert rc == 0, L.hqq_hip_last_error()
    kern.check_arenas("real angles")
    assert torch.equal(A.bits(got), A.bits(ref.to(T))), f"{int((A.bits(got) != A.bits(ref.to(T))).sum())} elements differ from the fp64 reference"
    assert torch.equal(A.bits(got), A.bits(want)), "differs from rope_cache + attn_decode"
    assert torch.equal(A.bits(bed.kc), A.bits(kc1)) and torch.equal(A.bits(bed.vc), A.bits(vc1)), "the caches differ from hqq_hip_rope_cache's"


@pytest.mark.parametrize("rope", [False, True], ids=["attn_batched", "rope_attn_batched"])
@pytest.mark.parametrize("S", [1, 8])
@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_batched_rows_keep_their_own_position_and_needle(L, dt, hd, S, rope):
    """B = 5, each row its own pos and its own needles (key 0, n - 1, the middle, n - 2): pos = 0 and rows with fewer visible keys than S included"""
    cache_len, heads = 1100, 4
    ns = (1, 4, 38, 601, 1100)
    B = len(ns)
    beds = [A.Bed(dt, hd, cache_len, "cuda", heads=heads, seed=b + 1) for b in range(B)]
    T = beds[0].T
    needles = [torch.tensor([0, n - 1, n // 2, max(n - 2, 0)], device="cuda") for n in ns]
    for bed, n, a in zip(beds, ns, needles):
        bed.shrink(n)
        bed.apply(a, a)
    q = torch.stack([bed.q.view(-1) for bed in beds]).contiguous()
    kc, vc = torch.stack([bed.kc for bed in beds]).contiguous(), torch.stack([bed.vc for bed in beds]).contiguous()
    pos = torch.tensor([n - 1 for n in ns], device="cuda")
    out = torch.full((B, heads * hd), NAN, dtype=T, device="cuda")
    kern = Kernel(L, rope)
    ws_ptr, ws_bytes = kern.workspace(beds[0], S, batch=B)
    kw = {}
    if rope:
        k = torch.stack([kc[b, :, n - 1] for b, n in enumerate(ns)]).reshape(B, heads * hd).contiguous()
        v = torch.stack([vc[b, :, n - 1] for b, n in enumerate(ns)]).reshape(B, heads * hd).contiguous()
        for b, n in enumerate(ns):
            kc[b, :, n - 1] = NAN
            vc[b, :, n - 1] = NAN
        cos, sin = A.unit_angles(hd, T, "cuda", B)
        kw = dict(k=k, v=v, cos=cos, sin=sin)
    before_k, before_v = kc.clone(), vc.clone()
    rc = A.call(L, rope=rope, dt=dt, q=q, kc=kc, vc=vc, pos=pos, out=out, S=S, ws_ptr=ws_ptr, ws_bytes=ws_bytes, batch=B, **kw)
    assert rc == 0, L.hqq_hip_last_error()
    kern.check_arenas("batched")
    if rope:
        for b, n in enumerate(ns):
            before_k[b, :, n - 1] = k[b].view(heads, hd)
            before_v[b, :, n - 1] = v[b].view(heads, hd)
    assert torch.equal(A.bits(kc), A.bits(before_k)) and torch.equal(A.bits(vc), A.bits(before_v)), "the caches are not what they were (plus the new rows)"
    for b, (bed, n, a) in enumerate(zip(beds, ns, needles)):
        ref, _ = bed.reference(n)
        assert not bool(A.closed_form_bad(bed, "needle", n, a, a, ref).any()), f"row {b}: the fp64 reference misses the closed form"
        bad = A.kernel_bad(bed, "needle", out[b].view(heads, hd), ref)
        assert not bool(bad.any()), f"row {b} (n = {n}): heads {bad.nonzero().view(-1).tolist()} differ from the fp64 reference"
        bed.restore()


def _fenced(shape, T, guard_elems=1 << 16):
    """a tensor of `shape` inside one allocation, guard_elems elements of 0x5A5A either side; returns (whole int16 buffer, the view, guard_elems)"""
    numel = 1
    for s in shape:
        numel *= s
    buf = torch.full((guard_elems + numel + guard_elems,), 0x5A5A, dtype=torch.int16, device="cuda")
    view = buf[guard_elems:guard_elems + numel].view(T).view(*shape)
    assert view.data_ptr() % 16 == 0
    return buf, view, guard_elems


def _guards_intact(buf, g):
    return bool((buf[:g] == 0x5A5A).all()) and bool((buf[-g:] == 0x5A5A).all())


@pytest.mark.parametrize("batched", [False, True], ids=["one", "batched"])
@pytest.mark.parametrize("rope", [False, True], ids=["attn", "rope_attn"])
@pytest.mark.parametrize("S", [1, 4])
@pytest.mark.parametrize("hd", A.HDS)
@pytest.mark.parametrize("dt", DTS)
def test_positions_outside_the_cache(L, dt, hd, S, rope, batched):
    """block.hip: "a position outside [0, L) must not index the cache or the score buffer: attend as if at the last slot, write nothing".  pos in
    {-1, L, L + 5} (cache_len is the caches' true length; they and the output sit between guard bands): the output is, bit for bit, that of
    pos = L - 1 — itself checked against fp64 through its needles — and the rotary forms leave both caches as they were.
    In the rotary forms row L - 1 of both caches is NaN and stays NaN: the last slot's key and value must come from the call itself.  In range
    the NaN row of the other rotary tests is overwritten by the kernel's own write-back before or while it is read (the same workgroup at
    splits = 1 without GQA, a race otherwise), so a kernel that read position pos from the cache is caught with certainty only here"""
    cache_len, heads = 200, 4
    outside = (-1, cache_len, cache_len + 5)
    bed = A.Bed(dt, hd, cache_len, "cuda", heads=heads)
    T = bed.T
    a = torch.tensor([cache_len - 1, 0, cache_len // 2, cache_len - 2], device="cuda")
    bed.apply(a, a)
    ref, _ = bed.reference(cache_len)
    assert not bool(A.closed_form_bad(bed, "needle", cache_len, a, a, ref).any())
    kw = {}
    if rope:
        k, v = bed.kc[:, cache_len - 1].clone().view(1, -1), bed.vc[:, cache_len - 1].clone().view(1, -1)
        bed.kc[:, cache_len - 1] = NAN       # the last slot's key and value come from the call (LDS), never from the cache
        bed.vc[:, cache_len - 1] = NAN
    kern = Kernel(L, rope)
    for group in ([outside] if batched else [(p,) for p in outside]):
        B = len(group)
        if rope:
            cos, sin = A.unit_angles(hd, T, "cuda", B)
            kw = dict(k=k.expand(B, -1).contiguous(), v=v.expand(B, -1).contiguous(), cos=cos, sin=sin)
        q = bed.q.view(1, -1).expand(B, -1).contiguous()
        ws_ptr, ws_bytes = kern.workspace(bed, S, batch=B)
        # at the last slot, on plain copies
        kc1, vc1 = (t.unsqueeze(0).expand(B, -1, -1, -1).clone() for t in (bed.kc, bed.vc))   # (copies also at B = 1: the rotary call writes row L - 1)
        want = torch.full((B, heads * hd), NAN, dtype=T, device="cuda")
        last = torch.full((B,), cache_len - 1, dtype=torch.int64, device="cuda")
        rc = A.call(L, rope=rope, dt=dt, q=q, kc=kc1, vc=vc1, pos=last, out=want, S=S, ws_ptr=ws_ptr, ws_bytes=ws_bytes, batch=B if batched else None, **kw)
        assert rc == 0, L.hqq_hip_last_error()
        for b in range(B):
            assert not bool(A.kernel_bad(bed, "needle", want[b].view(heads, hd), ref).any()), "pos = L - 1 differs from the fp64 reference"
        # outside the cache, between guard bands
        kbuf, kc2, kg = _fenced((B, heads, cache_len, hd), T)
        vbuf, vc2, vg = _fenced((B, heads, cache_len, hd), T)
        obuf, got, og = _fenced((B, heads * hd), T)
        for b in range(B):
            kc2[b] = bed.kc
            vc2[b] = bed.vc
        kbefore, vbefore = kbuf.clone(), vbuf.clone()
        ws_ptr, ws_bytes = kern.workspace(bed, S, batch=B)
        pos = torch.tensor(group, dtype=torch.int64, device="cuda")
        rc = A.call(L, rope=rope, dt=dt, q=q, kc=kc2, vc=vc2, pos=pos, out=got, S=S, ws_ptr=ws_ptr, ws_bytes=ws_bytes, batch=B if batched else None, **kw)
        assert rc == 0, L.hqq_hip_last_error()
        kern.check_arenas(f"pos {group}")
        assert torch.equal(A.bits(got), A.bits(want)), f"pos {group}: {int((A.bits(got) != A.bits(want)).sum())} outputs differ from those at pos = L - 1"
        assert torch.equal(kbuf, kbefore) and torch.equal(vbuf, vbefore), f"pos {group}: a cache (or a guard band around it) was written"
        assert _guards_intact(obuf, og) and _guards_intact(kbuf, kg) and _guards_intact(vbuf, vg), f"pos {group}: a guard band was written"


def test_dense_batched_fronts_refuse_a_cache_of_another_dtype():
    """An fp16 q against a bf16 cache, then against an fp16 k_cache with only v_cache in bf16: each dense batched front raises ValueError before anything is
    launched (the kernel would read the cache's 16-bit words as q's type), and out stays untouched."""
    from hqq_amd import ops

    hd, heads, cache_len = 64, 2, 8
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(1, heads * hd, generator=g).half().cuda() for _ in range(3))
    kc, vc = (torch.randn(1, heads, cache_len, hd, generator=g).bfloat16().cuda() for _ in range(2))
    cos, sin = torch.ones(1, hd, dtype=torch.float16, device="cuda"), torch.zeros(1, hd, dtype=torch.float16, device="cuda")
    pos = torch.tensor([3], dtype=torch.int64, device="cuda")
    out = torch.full((1, heads * hd), 7.0, dtype=torch.float16, device="cuda")
    before = out.clone()
    for k_cache, v_cache in ((kc, vc), (kc.half(), vc)):
        with pytest.raises(ValueError):
            ops.attn_decode_batched(q, k_cache, v_cache, pos, out, hd ** -0.5)
        with pytest.raises(ValueError):
            ops.attn_decode_gqa_batched(q, k_cache, v_cache, pos, out, hd ** -0.5)
        with pytest.raises(ValueError):
            ops.rope_attn_decode_batched(q, k, v, cos, sin, pos, k_cache, v_cache, out, hd ** -0.5)
    torch.cuda.synchronize()
    assert torch.equal(out, before), "out was written by a refused call"
