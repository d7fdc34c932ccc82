"""CPU tests of hqq_amd.core.peft.LoRABank (several adapters stacked for one adapted model), of the routed adapter kernels' C ABI as far as it needs no GPU,
and of the `adapter` / `adapters` keyword check of the decoder."""
import ctypes
import os
import re

import pytest

torch = pytest.importorskip("torch")
from torch import nn   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32c, F16c = 0, 1
CFG = {"r": 4, "lora_alpha": 8, "dropout": 0.0}


class Attn(nn.Module):
    def __init__(self, bias=False):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = nn.Linear(64, 32, bias=bias), nn.Linear(64, 32, bias=False), nn.Linear(64, 48, bias=False)


class Block(nn.Module):
    def __init__(self, bias=False):
        super().__init__()
        self.self_attn = Attn(bias)


class Stub(nn.Module):
    def __init__(self, bias=False):
        super().__init__()
        self.layers = nn.ModuleList([Block(bias), Block(bias)])


def _adapted(seed, r_v=6, bias=False):
    """a stub with wrappers on q_proj (rank 4) and v_proj (rank r_v) of both blocks, k_proj left alone; lora_B random (LoRA's own initialiser zeroes it)"""
    from hqq_amd.core.peft import PeftUtils, is_hqq_lora_layer
    torch.manual_seed(seed)
    m = Stub(bias)
    PeftUtils.add_lora(m, {"self_attn.q_proj": dict(CFG), "self_attn.k_proj": None, "self_attn.v_proj": dict(CFG, r=r_v, lora_alpha=3)})
    for w in m.modules():
        if is_hqq_lora_layer(w):
            w.lora_B.data = torch.randn_like(w.lora_B) * 0.1
    return m


def _wrappers(model):
    from hqq_amd.core.peft import is_hqq_lora_layer
    return {n: w for n, w in model.named_modules() if is_hqq_lora_layer(w)}


@pytest.fixture()
def three_files(tmp_path):
    """three adapters for the same architecture, saved by PeftUtils.save_lora_weights: (the file names, the models that hold them)"""
    from hqq_amd.core.peft import PeftUtils
    models = [_adapted(10 + i) for i in range(3)]
    files = []
    for i, m in enumerate(models):
        files.append(str(tmp_path / f"adapter{i}.pt"))
        PeftUtils.save_lora_weights(m, files[-1])
    return files, models


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a.view(torch.int16),
                                                                     b.view(torch.int32) if b.dtype == torch.float32 else b.view(torch.int16))


def test_a_bank_stacked_from_files_holds_exactly_their_bits(three_files, tmp_path):
    from hqq_amd.core.peft import LoRABank
    files, models = three_files
    host = _adapted(99)
    bank = LoRABank.from_files(host, files)
    names = sorted(_wrappers(host))
    assert bank.n == 3 and sorted(bank.names) == names and len(names) == 4
    total = 0
    for name in names:
        A, B, s = bank.layer(name)
        w = _wrappers(host)[name]
        assert tuple(A.shape) == (3, w.in_features, w.r) and tuple(B.shape) == (3, w.r, w.out_features) and tuple(s.shape) == (3,)
        assert A.dtype == B.dtype == w.lora_A.dtype and s.dtype == torch.float32 and A.device == w.lora_A.device
        assert A.is_contiguous() and B.is_contiguous()
        total += A.numel() * 4 + B.numel() * 4 + 12
        for i, m in enumerate(models):
            src = _wrappers(m)[name]
            assert _same_bits(A[i], src.lora_A.data) and _same_bits(B[i], src.lora_B.data)
            assert float(s[i]) == float(torch.tensor(float(src.scaling), dtype=torch.float32))
    assert bank.nbytes == total
    # the bare v0.1 dictionary, as a file and as a dictionary; and from_params on v0.2 dictionaries
    v01 = [str(tmp_path / f"old{i}.pt") for i in range(3)]
    for f_old, f in zip(v01, files):
        torch.save(torch.load(f, map_location="cpu", weights_only=True)["parameters"], f_old)
    for other in (LoRABank.from_files(host, v01), LoRABank.from_params(host, [torch.load(f, map_location="cpu", weights_only=True) for f in files]),
                  LoRABank.from_params(host, [torch.load(f, map_location="cpu", weights_only=True) for f in v01])):
        for name in names:
            assert all(_same_bits(p, q) for p, q in zip(other.layer(name), bank.layer(name)))
    # another dtype for the stack
    half = LoRABank.from_files(host, files, dtype=torch.float16)
    A, B, s = half.layer(names[0])
    assert A.dtype == B.dtype == torch.float16 and s.dtype == torch.float32 and _same_bits(A[1], _wrappers(models[1])[names[0]].lora_A.data.half())


def test_every_refusal_names_layer_and_adapter(three_files):
    from hqq_amd.core.peft import LoRABank
    files, models = three_files
    host = _adapted(99)
    good = [torch.load(f, map_location="cpu", weights_only=True)["parameters"] for f in files]
    name = "layers.1.self_attn.v_proj"

    def broken(edit):
        params = [{k: dict(v) for k, v in p.items()} for p in good]
        edit(params[2])
        return params

    def drop(p):
        del p[name]

    def other_rank(p):
        p[name]["lora_A"], p[name]["lora_B"] = torch.zeros(64, 5), torch.zeros(5, 48)

    def with_bias(p):
        p[name]["bias"] = torch.zeros(48)

    def mixed(p):
        p[name]["lora_B"] = p[name]["lora_B"].half()

    for edit, word in ((drop, "no entry"), (other_rank, "rank"), (with_bias, "bias"), (mixed, "mixed dtypes")):
        with pytest.raises(ValueError, match=word) as e:
            LoRABank.from_params(host, broken(edit))
        assert name in str(e.value) and "adapter 2" in str(e.value), str(e.value)
    # a file saved from wrappers that carry a bias
    biased = _adapted(5, bias=True)
    with pytest.raises(ValueError, match="bias"):
        LoRABank.from_params(host, [{n: w.state_dict() for n, w in _wrappers(biased).items()}])
    with pytest.raises(ValueError, match="wrappers"):
        LoRABank.from_params(Stub(), good)
    with pytest.raises(ValueError, match="at least one"):
        LoRABank.from_params(host, [])
    bank = LoRABank.from_params(host, good)
    for i in (-1, 3):
        with pytest.raises(ValueError, match="index"):
            bank.set(i, good[0])
    for i in (-2, 3):
        with pytest.raises(ValueError, match="index"):
            bank.activate(host, i)
    with pytest.raises(ValueError, match="not the ones"):
        bank.activate(Stub(), 0)
    # a refused set() leaves the bank as it was
    before = [t.clone() for n in bank.names for t in bank.layer(n)]
    with pytest.raises(ValueError):
        bank.set(1, broken(with_bias)[2])
    assert all(_same_bits(p, q) for p, q in zip(before, [t for n in bank.names for t in bank.layer(n)]))


def test_activate_round_trips_the_wrappers_and_keeps_their_addresses(three_files):
    from hqq_amd.core.peft import LoRABank
    files, models = three_files
    host = _adapted(99)
    bank = LoRABank.from_files(host, files)
    ws = _wrappers(host)
    ptrs = {n: (w.lora_A.data_ptr(), w.lora_B.data_ptr()) for n, w in ws.items()}
    x = torch.randn(3, 64)
    for i in (2, 0, 1, 2):
        bank.activate(host, i)
        for n, w in ws.items():
            src = _wrappers(models[i])[n]
            assert _same_bits(w.lora_A.data, src.lora_A.data) and _same_bits(w.lora_B.data, src.lora_B.data)
            assert isinstance(w.scaling, float) and w.scaling == float(torch.tensor(float(src.scaling), dtype=torch.float32))
            assert (w.lora_A.data_ptr(), w.lora_B.data_ptr()) == ptrs[n]
    # -1: lora_B zeroed, lora_A and scaling as they were — the base model
    A_before = {n: w.lora_A.data.clone() for n, w in ws.items()}
    s_before = {n: w.scaling for n, w in ws.items()}
    bank.activate(host, -1)
    for n, w in ws.items():
        assert not w.lora_B.data.any() and _same_bits(w.lora_A.data, A_before[n]) and w.scaling == s_before[n]
        assert (w.lora_A.data_ptr(), w.lora_B.data_ptr()) == ptrs[n]
        assert torch.equal(w(x), w.linear_layer(x))
    bank.activate(host, 1)   # and back
    assert all(_same_bits(w.lora_B.data, _wrappers(models[1])[n].lora_B.data) for n, w in ws.items())


def test_set_copies_in_place(three_files):
    from hqq_amd.core.peft import LoRABank
    files, models = three_files
    host = _adapted(99)
    bank = LoRABank.from_files(host, files)
    ptrs = bank.pointers()
    assert ptrs[0] == 3 and len(ptrs) == 1 + 3 * len(bank.names)
    bank.set(2, files[0])
    bank.set(1, torch.load(files[2], map_location="cpu", weights_only=True))
    assert bank.pointers() == ptrs
    for n in bank.names:
        A, B, s = bank.layer(n)
        assert _same_bits(A[2], A[0]) and _same_bits(B[2], B[0]) and float(s[2]) == float(s[0])
        assert _same_bits(A[1], _wrappers(models[2])[n].lora_A.data) and _same_bits(B[1], _wrappers(models[2])[n].lora_B.data)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------------------------
def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


def test_the_three_symbols_are_bound_and_the_abi_version_stays():
    from hqq_amd import _C
    lib = _C.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hqq_hip.h")).read(), flags=re.S)
    for name, nargs in (("hqq_hip_lora_routed_covers", 8), ("hqq_hip_lora_shrink_routed", 13), ("hqq_hip_lora_expand_routed", 15)):
        m = re.search(rf"\b{name}\s*\(([^)]*)\)", hdr)
        assert m and len(m.group(1).split(",")) == nargs == len(_C.SYMBOLS[name][1]), name
        assert hasattr(lib, name)
    assert lib.hqq_hip_abi_version() == _C.ABI_VERSION == 9
    assert "added without raising HQQ_HIP_ABI_VERSION" in open(os.path.join(ROOT, "include", "hqq_hip.h")).read().split("int hqq_hip_lora_routed_covers(")[0][-400:]


def test_routed_coverage_is_host_arithmetic():
    from hqq_amd import _C, ops
    lib = _C.lib()
    cov = lib.hqq_hip_lora_routed_covers
    assert cov(3, _i64(4096, 1024, 1024), _i64(16, 64, 256), 256, 16, 4096, F16c, F32c) == 1
    assert cov(1, _i64(64), _i64(8), 1, 1, 64, F16c, F16c) == 1
    for na in (0, -1, 257):
        assert cov(1, _i64(64), _i64(8), na, 1, 64, F16c, F32c) == 0 and b"adapters" in lib.hqq_hip_last_error()
    assert cov(1, _i64(64), _i64(8), 3, 17, 64, F16c, F32c) == 0 and b"17 rows" in lib.hqq_hip_last_error()      # what the one-adapter pair refuses
    assert cov(1, _i64(64), _i64(257), 3, 1, 64, F16c, F32c) == 0 and cov(1, _i64(64), _i64(8), 3, 1, 64, F32c, F32c) == 0
    assert ops.LORA_MAX_ADAPTERS == 256 and ops.lora_routed_covers(torch.float16, torch.float32, 256, 16, [4096], 4096, [16])
    assert not ops.lora_routed_covers(torch.float16, torch.float32, 257, 16, [4096], 4096, [16])
    assert not ops.lora_routed_covers(torch.float32, torch.float32, 3, 1, [4096], 4096, [16])
    # refusals with placeholder pointers: no GPU in this process, so a call that got as far as a launch would fail differently
    p16, VP1 = ctypes.c_void_p(16), (ctypes.c_void_p * 1)(16)
    need = lib.hqq_hip_lora_decode_workspace_bytes(1, _i64(8), 2, 520)
    assert lib.hqq_hip_lora_shrink_routed(1, p16, VP1, _i64(8), 0, p16, 2, 520, F16c, F32c, p16, need, None) == -4
    assert lib.hqq_hip_lora_shrink_routed(1, p16, VP1, _i64(8), 3, p16, 2, 520, F16c, F32c, p16, need - 1, None) == -5
    assert lib.hqq_hip_lora_shrink_routed(1, p16, VP1, _i64(8), 3, None, 2, 520, F16c, F32c, p16, need, None) == -2
    assert lib.hqq_hip_lora_expand_routed(1, p16, need, VP1, VP1, VP1, _i64(64), _i64(8), 257, p16, 2, 520, F16c, F32c, None) == -4
    assert lib.hqq_hip_lora_expand_routed(1, p16, need - 1, VP1, VP1, VP1, _i64(64), _i64(8), 3, p16, 2, 520, F16c, F32c, None) == -5
    assert lib.hqq_hip_lora_expand_routed(1, p16, need, VP1, (ctypes.c_void_p * 1)(None), VP1, _i64(64), _i64(8), 3, p16, 2, 520, F16c, F32c, None) == -2


def test_the_routed_wrappers_refuse_cpu_tensors():
    from hqq_amd import ops
    x, A, B = torch.zeros(2, 64, dtype=torch.float16), torch.zeros(3, 64, 8), torch.zeros(3, 8, 64)
    slots, ws, y = torch.zeros(2, dtype=torch.int64), torch.zeros(64, dtype=torch.uint8), torch.zeros(2, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_shrink_routed(x, [A], slots, ws)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.lora_expand_routed(ws, [B], [torch.ones(3)], slots, [y], 64)
    with pytest.raises(ValueError, match=r"A \[n, K, r\]"):
        ops.lora_apply_routed(x, [(A[0], B[0], torch.ones(3))], slots, [y])
    with pytest.raises(TypeError, match="share a dtype"):
        ops.lora_apply_routed(x, [(A, B.half(), torch.ones(3))], slots, [y])


# ---- the decoder's keywords --------------------------------------------------------------------------------------------------------------------------
def test_adapter_keywords_need_a_bank_and_an_index_into_it(three_files):
    from hqq_amd.core.peft import LoRABank
    from hqq_amd.utils.generation import check_adapters
    files, _ = three_files
    bank = LoRABank.from_files(_adapted(99), files)
    assert check_adapters(None, None, 4) == [] and check_adapters(bank, None, 2) == [-1, -1]
    assert check_adapters(bank, [1, -1, 0, 2], 4) == [1, -1, 0, 2]
    for bad in ([0], 0, [-1, 2]):
        with pytest.raises(ValueError, match="without one"):
            check_adapters(None, bad, 2)
    for bad in ([3, 0], [0, -2], [0, 1.0], [0, True], [0, "1"]):
        with pytest.raises(ValueError, match="not an index into the bank"):
            check_adapters(bank, bad, 2)
    with pytest.raises(ValueError, match="3 adapters for 2 prompts"):
        check_adapters(bank, [0, 1, 2], 2)


def test_the_step_and_the_decoders_take_the_keywords():
    """(their behaviour is the GPU suite's; here: the keywords exist where the interface promises them)"""
    import inspect
    from hqq_amd.utils.generation import GraphedGreedyDecoder, HFGenerator
    from hqq_amd.utils.llama_fused import FusedLlamaBatchStep, FusedLlamaStep
    for fn, kw in ((FusedLlamaStep.__init__, "lora_bank"), (FusedLlamaBatchStep.__init__, "lora_bank"), (GraphedGreedyDecoder.__init__, "lora_bank"),
                   (HFGenerator.__init__, "lora_bank"), (GraphedGreedyDecoder.generate, "adapter"), (GraphedGreedyDecoder.generate_batch, "adapters"),
                   (HFGenerator.generate, "adapter"), (HFGenerator.generate_batch, "adapters")):
        p = inspect.signature(fn).parameters
        assert kw in p and p[kw].default is None, (fn.__qualname__, kw)
