"""CPU half of the quantised KV cache's tests (csrc/kv_cache.hip, hqq_amd.ops.kv_*, hqq_amd.utils.kv_cache): the numpy restatement of the row format in
tests/_kvq_cases.py against the oracle's Quantizer.quantize(optimize=False) / dequantize bit for bit, the 4-bit byte rule, the round-trip error bound, the
decoders' keyword validation and ops.kv_covers' rule table.  No GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _kvq_cases as C   # noqa: E402

CODES = {"f16": C.F16, "bf16": C.BF16}
GRID = [(hd, gs, nbits, dt) for hd, gs in C.SHAPES for nbits in (8, 4) for dt in ("f16", "bf16")]
IDS = [f"hd{hd}-gs{gs}-q{nbits}-{dt}" for hd, gs, nbits, dt in GRID]


@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_restatement_equals_the_oracle_bit_for_bit(oracle, hd, gs, nbits, dt):
    """quantise and dequantise of every special row: levels, scale and zero (cast to T) and the rebuilt row equal the oracle's on the [hd / gs, gs] view"""
    code = CODES[dt]
    x = C.special_rows(hd, gs, nbits, code)
    lv, sc, ze = C.quantize_rows(x, code, nbits, gs)
    G = hd // gs
    w32 = C.from_cd(x, code)
    seen_clamp = seen_unit = False
    for r in range(x.shape[0]):
        ref = oracle.quantize(w32[r].reshape(G, gs), nbits=nbits, group_size=gs, round_zero=False, optimize=False)
        assert np.array_equal(ref["Wq"].reshape(-1), lv[r]), r
        ref_sc, ref_ze = oracle.to_cd(ref["scale"].reshape(-1), code), oracle.to_cd(ref["zero"].reshape(-1), code)
        assert np.array_equal(np.asarray(ref_sc).view(np.uint16), np.asarray(sc[r]).view(np.uint16)), r
        assert np.array_equal(np.asarray(ref_ze).view(np.uint16), np.asarray(ze[r]).view(np.uint16)), r
        seen_clamp |= bool((ref["scale"] == np.float32(1.0) / np.float32(2e4)).any())
        seen_unit |= bool((ref["scale"] == np.float32(1.0)).any())
        packed = oracle.pack(nbits, lv[r].reshape(G, gs))
        assert np.array_equal(packed.reshape(-1), C.pack_rows(lv[r:r + 1], nbits)[0]), r   # BitPack.pack_4bit_u8 / pack_8bit_u8 on the level matrix: the stored bytes
        want = oracle.dequantize(nbits, packed, np.asarray(sc[r]).reshape(G, 1), np.asarray(ze[r]).reshape(G, 1), 1, hd, gs, code)
        got = C.dequantize_rows(lv[r:r + 1], sc[r:r + 1], ze[r:r + 1], code, gs)
        assert np.array_equal(np.asarray(want).view(np.uint16).reshape(-1), np.asarray(got).view(np.uint16).reshape(-1)), r
    assert seen_clamp and seen_unit   # the rows reach the 2e4 clamp, and scale 1 (a constant group and a range below 1e-4)


@pytest.mark.parametrize("hd", [64, 128, 256])
def test_the_four_bit_byte_rule(hd):
    """byte i of a row is level[i] << 4 | level[i + hd / 2]; 8 bits: byte i is level i; unpack inverts both"""
    lv = (np.arange(3 * hd).reshape(3, hd) * 7 % 16).astype(np.uint8)
    p = C.pack_rows(lv, 4)
    assert p.shape == (3, hd // 2)
    for i in (0, 1, hd // 2 - 1):
        assert np.array_equal(p[:, i], (lv[:, i] << 4) | lv[:, i + hd // 2])
    assert np.array_equal(C.unpack_rows(p, 4), lv)
    lv8 = (np.arange(3 * hd).reshape(3, hd) * 37 % 256).astype(np.uint8)
    assert np.array_equal(C.pack_rows(lv8, 8), lv8) and np.array_equal(C.unpack_rows(lv8, 8), lv8)


@pytest.mark.parametrize("hd,gs,nbits,dt", GRID, ids=IDS)
def test_round_trip_error_stays_within_the_derived_bound(hd, gs, nbits, dt):
    """randn rows, rows scaled by 8 and rows offset by +-3 (a zero far from the levels): no scale is clamped and nothing leaves T's normal range, which is where
    _kvq_cases.roundtrip_bound's derivation applies"""
    code = CODES[dt]
    rng = np.random.default_rng(hd + gs + nbits)
    x = np.concatenate([rng.standard_normal((8, hd)), 8.0 * rng.standard_normal((8, hd)), 3.0 + rng.standard_normal((4, hd)), -3.0 + 0.5 * rng.standard_normal((4, hd))])
    x_cd = C.to_cd(x.astype(np.float32), code)
    x32 = C.from_cd(x_cd, code)
    rng_g = x32.reshape(-1, hd // gs, gs)
    assert ((rng_g.max(2) - rng_g.min(2)) > max(1e-4, (2 ** nbits - 1) / 2e4)).all()
    lv, sc, ze = C.quantize_rows(x_cd, code, nbits, gs)
    back = C.from_cd(C.dequantize_rows(lv, sc, ze, code, gs), code)
    assert np.isfinite(back).all()
    err, bound = np.abs(back.astype(np.float64) - x32.astype(np.float64)), C.roundtrip_bound(x32, gs, nbits, code)
    assert (err <= bound).all(), float((err / bound).max())
    assert (err > 0.25 * bound).any()   # the bound is not vacuous: some element uses a quarter of it


def test_keyword_validation_of_the_decoders():
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator
    from hqq_amd.utils.kv_cache import check_kv_group_size, kv_cache_bits
    assert kv_cache_bits(None) is None and kv_cache_bits("q8") == 8 and kv_cache_bits("q4") == 4
    for bad in ("q2", "q3", "Q8", "int8", 8, 4, True, ""):
        with pytest.raises(ValueError, match="kv_cache"):
            kv_cache_bits(bad)
        with pytest.raises(ValueError, match="kv_cache"):
            GraphedGreedyDecoder(None, kv_cache=bad)   # (refused before the model is looked at)
        with pytest.raises(ValueError, match="kv_cache"):
            HFGenerator(None, None, kv_cache=bad)
    check_kv_group_size(None, None), check_kv_group_size("q8", 32), check_kv_group_size("q4", 64), check_kv_group_size("q4", None)
    for bad in (16, 48, 128, True, "64"):
        with pytest.raises(ValueError, match="kv_group_size"):
            GraphedGreedyDecoder(None, kv_cache="q8", kv_group_size=bad)
        with pytest.raises(ValueError, match="kv_group_size"):
            HFGenerator(None, None, kv_cache="q4", kv_group_size=bad)
    with pytest.raises(ValueError, match="kv_group_size"):
        GraphedGreedyDecoder(None, kv_group_size=32)   # a group size without a quantised cache


def test_quantized_static_cache_refuses_what_it_does_not_hold():
    from transformers import LlamaConfig, MistralConfig
    from hqq_amd.utils.kv_cache import QuantizedStaticCache
    cfg = LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2, vocab_size=64)
    c = QuantizedStaticCache(cfg, 64, 4)
    assert len(c.layers) == 3 and c.nbytes == 0 and not c.is_initialized and c.is_compileable
    for kw in (dict(nbits=2), dict(nbits=3), dict(nbits=8, group_size=16), dict(nbits=8, group_size=128)):
        with pytest.raises(ValueError):
            QuantizedStaticCache(cfg, 64, **kw)
    for L in (0, 30001):
        with pytest.raises(ValueError):
            QuantizedStaticCache(cfg, L, 8)
    with pytest.raises(ValueError, match="full-attention"):
        QuantizedStaticCache(MistralConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, vocab_size=64, sliding_window=16), 64, 8)


def test_kv_covers_rule_table():
    from hqq_amd import ops
    f16, bf16 = torch.float16, torch.bfloat16
    for dt in (f16, bf16):
        for hd in (64, 128, 256):
            for gs in (32, 64):
                assert ops.kv_covers(dt, 8, hd, gs, 96)                       # 8 bits: every gs that divides head_dim (64 with 64 included)
                assert ops.kv_covers(dt, 4, hd, gs, 96) == (2 * gs <= hd)     # 4 bits: the two halves of a row must not share a group
            assert ops.kv_covers(dt, 8, hd, ops.kv_group_size(hd)) and ops.kv_covers(dt, 4, hd, ops.kv_group_size(hd))
    assert ops.kv_group_size(64) == 32 and ops.kv_group_size(128) == 64 and ops.kv_group_size(256) == 64
    for nbits in (1, 2, 3, 5, 16, True, 4.0):
        assert not ops.kv_covers(f16, nbits, 128, 64)
    for hd in (32, 96, 80, 512):
        assert not ops.kv_covers(f16, 8, hd, 32)
    for gs in (8, 16, 128, None):
        assert not ops.kv_covers(f16, 8, 128, gs)
    assert not ops.kv_covers(torch.float32, 8, 128, 64)
    assert ops.kv_covers(f16, 8, 128, 64, 1) and ops.kv_covers(f16, 8, 128, 64, 30000)
    assert not ops.kv_covers(f16, 8, 128, 64, 0) and not ops.kv_covers(f16, 8, 128, 64, 30001)
