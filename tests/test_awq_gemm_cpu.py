"""AWQ GEMM-packing bridge, host side: packing.py's torch ops against what the reference's WQLinear_GEMM.from_linear and
WQLinear_QUICK.from_linear made of the same layers (tests/golden/exact_*.npz: ref_gemm_* and ref_q*), the WQLinear_GEMM module on CPU
tensors, and the shape rules of the two C entry points.  No GPU needed."""
import copy
import io
import os

import numpy as np
import pytest
import torch

from conftest import exact_layer, golden_files, load_golden
from quick_amd import WQLinear_GEMM, WQLinear_QUICK, _lib, fuse_qkv_gemm, packing

EXACT = golden_files("exact_")
ids = lambda p: os.path.basename(p)[:-4]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(a):
    """Bit pattern of an array, whatever its dtype."""
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want):
    got, want = tuple(got), tuple(want)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        a = a.numpy() if isinstance(a, torch.Tensor) else a
        b = b.numpy() if isinstance(b, torch.Tensor) else b
        assert a.shape == b.shape and a.dtype == b.dtype, (i, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bits(a), _bits(b)), i


def _gemm(g):
    return _t(g["ref_gemm_qweight"]), _t(g["ref_gemm_qzeros"]), _t(g["ref_gemm_scales"])


def _quick(g):
    return _t(g["ref_qweight"]), _t(g["ref_qscales"]), _t(g["ref_qzeros"])


def _logical(g):
    """(iw [K, N] uint8, s [K/G, N] fp16, z [K/G, N] uint8) of a fixture."""
    return (_t(g["intweight_nk"].T), _t(g["scales_nk"].T), _t(g["zeros_nk"].T.astype(np.uint8)))


def _gemm_sd(g):
    qw, qz, sc = _gemm(g)
    return {"qweight": qw, "qzeros": qz, "scales": sc}


def _module(g, bias=False):
    return WQLinear_GEMM(4, int(g["G"]), int(g["K"]), int(g["N"]), bias, "cpu")


def test_there_are_six_exact_fixtures():
    assert len(EXACT) == 6 and sum("k64" in p for p in EXACT) == 1


@pytest.mark.parametrize("path", EXACT, ids=ids)
def test_unpack_and_pack_awq_gemm_reproduce_the_reference_tensors(path):
    g = load_golden(path)
    iw, s, z = packing.unpack_awq_gemm(*_gemm(g))
    assert np.array_equal(iw.numpy(), g["intweight_nk"].T)
    assert s.dtype == torch.float16 and np.array_equal(s.numpy().view(np.uint16), np.ascontiguousarray(g["scales_nk"].T).view(np.uint16))
    assert np.array_equal(z.numpy(), g["zeros_nk"].T)
    _same(packing.pack_awq_gemm(iw, s, z), _gemm(g))
    _same(packing.pack_awq_gemm(*_logical(g)), _gemm(g))


@pytest.mark.parametrize("path", EXACT, ids=ids)
def test_awq_gemm_to_cuda_order_is_the_reference_quick_checkpoint(path):
    g = load_golden(path)
    _same(packing.awq_gemm_to_cuda_order(*_gemm(g)), _quick(g))


@pytest.mark.parametrize("path", EXACT, ids=ids)
def test_awq_gemm_to_mi355x_and_back(path):
    g = load_golden(path)
    K, G = int(g["K"]), int(g["G"])
    got = packing.awq_gemm_to_mi355x(*_gemm(g))
    iw, s, z = _logical(g)
    if K % 128 == 0:
        _same(got, packing.pack_mi355x(iw, s, z))
        _same(got, packing.cuda_to_mi355x(*_quick(g)))
        _same(packing.mi355x_to_awq_gemm(*got), _gemm(g))
    else:   # K = 64, G = 64: padded to 128 rows / two groups with weight 0, scale 0, zero point 0
        assert (K, G) == (64, 64) and packing.padded_in_features(K, G) == 128
        pad = lambda t, rows: torch.cat([t, torch.zeros((rows - t.shape[0], t.shape[1]), dtype=t.dtype)])
        _same(got, packing.pack_mi355x(pad(iw, 128), pad(s, 2), pad(z, 2)))


def test_wqlinear_gemm_buffers_have_reference_names_shapes_and_dtypes():
    m = WQLinear_GEMM(4, 64, 256, 512, True, "cpu")
    sd = m.state_dict()
    assert list(sd) == ["qweight", "qzeros", "scales", "bias"]
    assert sd["qweight"].shape == (256, 64) and sd["qweight"].dtype == torch.int32
    assert sd["qzeros"].shape == (4, 64) and sd["qzeros"].dtype == torch.int32
    assert sd["scales"].shape == (4, 512) and sd["scales"].dtype == torch.float16
    assert sd["bias"].shape == (512,) and sd["bias"].dtype == torch.float16
    assert m.extra_repr() == "in_features=256, out_features=512, bias=True, w_bit=4, group_size=64"
    m = WQLinear_GEMM(4, -1, 256, 512, False, "cpu")
    assert m.group_size == 256 and m.bias is None and list(m.state_dict()) == ["qweight", "qzeros", "scales"]
    assert m.qzeros.shape == (1, 64) and m.scales.shape == (1, 512)
    with pytest.raises(NotImplementedError):
        WQLinear_GEMM(8, 128, 256, 256, False, "cpu")
    lin = torch.nn.Linear(256, 512, bias=True)
    m = WQLinear_GEMM.from_linear(lin, 4, 64, init_only=True)
    assert m.qweight.shape == (256, 64) and m.bias.shape == (512,) and not m.is_prepared


@pytest.mark.parametrize("path", EXACT, ids=ids)
def test_wqlinear_gemm_from_linear_packs_like_the_reference(path):
    g = load_golden(path)
    lin = torch.nn.Linear(int(g["K"]), int(g["N"]), bias=False).half()
    lin.weight.data = _t(g["weight"]).clone()
    m = WQLinear_GEMM.from_linear(lin, 4, int(g["G"]), False, _t(g["scales_nk"].T), _t(g["zeros_nk"].T))
    sd = m.state_dict()
    _same((sd["qweight"], sd["qzeros"], sd["scales"]), _gemm(g))


@pytest.mark.parametrize("path", [p for p in EXACT if "k64" not in p][:2], ids=ids)
def test_wqlinear_gemm_state_dict_speaks_the_gemm_packing(path):
    g = load_golden(path)
    K, N, G = int(g["K"]), int(g["N"]), int(g["G"])
    m = _module(g)
    m.load_state_dict(_gemm_sd(g))
    assert not m.is_prepared
    assert m.prepare() is m and m.is_prepared
    assert m.qweight.shape == (K // 4, N // 2) and m.scales.shape == (K // G, 2 * N) and m.qzeros.shape == (K // G, N // 4)
    _same((m.qweight, m.scales, m.qzeros), packing.cuda_to_mi355x(*_quick(g)))
    sd = m.state_dict()
    assert list(sd) == ["qweight", "qzeros", "scales"]
    _same((sd["qweight"], sd["qzeros"], sd["scales"]), _gemm(g))
    assert m.is_prepared                                    # saving does not change what the module holds
    # a second load into the prepared module: GEMM shapes again, unprepared, same bits
    m.load_state_dict({k: v.clone() for k, v in sd.items()})
    assert not m.is_prepared and m.qweight.shape == (K, N // 8) and m.scales.shape == (K // G, N)
    _same((m.qweight, m.qzeros, m.scales), _gemm(g))
    # copies and pickles of a prepared module stay prepared and save the same bits
    m.prepare()
    buf = io.BytesIO()
    torch.save(m, buf)
    for clone in (copy.deepcopy(m), torch.load(io.BytesIO(buf.getvalue()), weights_only=False)):
        assert clone.qweight.data_ptr() != m.qweight.data_ptr()
        assert clone.is_prepared and torch.equal(clone.qweight, m.qweight)
        sd = clone.state_dict()
        _same((sd["qweight"], sd["qzeros"], sd["scales"]), _gemm(g))
        clone.load_state_dict(_gemm_sd(g))                  # ... and a load right after the copy is noticed
        assert not clone.is_prepared and clone.qweight.shape == (K, N // 8)
    assert m.to(torch.device("cpu")).is_prepared             # moving keeps the fact
    m.qweight = _gemm(g)[0].clone()                         # attribute assignment from outside resets it
    assert not m.is_prepared


def test_wqlinear_gemm_k64_keeps_its_buffers_and_pads_a_copy():
    g = load_golden([p for p in EXACT if "k64" in p][0])
    m = _module(g)
    m.load_state_dict(_gemm_sd(g))
    assert m.prepare() is m and not m.is_prepared
    packed = m._padded_mi355x()
    assert packed[0].shape == (32, 64) and packed[1].shape == (2, 256) and packed[2].shape == (2, 32)
    assert m._padded_mi355x() is packed                      # made once ...
    _same(packed, packing.awq_gemm_to_mi355x(*_gemm(g)))
    sd = m.state_dict()
    _same((sd["qweight"], sd["qzeros"], sd["scales"]), _gemm(g))
    m.load_state_dict(_gemm_sd(g))                          # ... and dropped when the buffers are rewritten
    assert m._padded.packed is None
    clone = copy.deepcopy(m)
    assert clone._padded.packed is None and torch.equal(clone.qweight, m.qweight)


@pytest.mark.parametrize("path", [p for p in EXACT if "k128n128" in p or "k64" in p], ids=ids)
def test_wqlinear_gemm_forward_on_cpu_fails_loudly(path):
    g = load_golden(path)
    m = _module(g)
    m.load_state_dict(_gemm_sd(g))
    with pytest.raises(RuntimeError, match="GPU"):
        m(_t(g["x"]))


@pytest.mark.parametrize("path", EXACT, ids=ids)
def test_from_awq_gemm_gives_the_reference_quick_checkpoint(path):
    g = load_golden(path)
    src = _module(g, bias=True)
    src.load_state_dict(dict(_gemm_sd(g), bias=torch.arange(int(g["N"]), dtype=torch.float16)))
    for prepared in (False, True):
        if prepared:
            src.prepare()
        q = WQLinear_QUICK.from_awq_gemm(src)
        assert isinstance(q, WQLinear_QUICK) and q.is_prepared == (int(g["K"]) % 128 == 0)
        ptrs = {t.data_ptr() for t in (src.qweight, src.qzeros, src.scales, src.bias)}
        assert not ptrs & {t.data_ptr() for t in (q.qweight, q.qzeros, q.scales, q.bias)}
        sd = q.state_dict()
        _same((sd["qweight"], sd["scales"], sd["qzeros"]), _quick(g))
        assert torch.equal(sd["bias"], src.bias)

    class Foreign(torch.nn.Module):      # any module with the reference's buffers in the GEMM packing
        def __init__(self):
            super().__init__()
            self.in_features, self.out_features, self.w_bit, self.group_size = int(g["K"]), int(g["N"]), 4, int(g["G"])
            for name, t in _gemm_sd(g).items():
                self.register_buffer(name, t)
            self.bias = None

    sd = WQLinear_QUICK.from_awq_gemm(Foreign()).state_dict()
    assert "bias" not in sd
    _same((sd["qweight"], sd["scales"], sd["qzeros"]), _quick(g))


def test_fuse_qkv_gemm_concatenates_unequal_widths():
    K, G = 256, 128
    mods, logical = [], []
    for i, N in enumerate((256, 128, 128)):
        iw, s, z = [_t(a) for a in exact_layer(K, N, G, 50 + i)]
        m = WQLinear_GEMM(4, G, K, N, True, "cpu")
        qw, qz, sc = packing.pack_awq_gemm(iw, s, z)
        m.load_state_dict({"qweight": qw, "qzeros": qz, "scales": sc, "bias": torch.full((N,), float(i), dtype=torch.float16)})
        mods.append(m)
        logical.append((iw, s, z))
    mods[1].prepare()                                       # whatever the three modules currently hold
    fused = fuse_qkv_gemm(None, *mods)
    assert isinstance(fused, WQLinear_GEMM) and fused.out_features == 512 and not fused.is_prepared
    want = packing.pack_awq_gemm(*[torch.cat([l[i] for l in logical], dim=1) for i in range(3)])
    sd = fused.state_dict()
    _same((sd["qweight"], sd["qzeros"], sd["scales"]), want)
    assert torch.equal(sd["bias"], torch.cat([torch.full((n,), float(i), dtype=torch.float16) for i, n in enumerate((256, 128, 128))]))
    fused.prepare()
    iw2, _, _ = packing.unpack_mi355x(fused.qweight, fused.scales, fused.qzeros)
    assert torch.equal(iw2, torch.cat([l[0] for l in logical], dim=1))


@pytest.mark.parametrize("K,N,G,forward,reverse", [(256, 100, 128, 1, 1), (256, 128, 48, 1, 1), (200, 128, 100, 1, 1),
                                                   (256, 264, 128, 4, 4), (192, 128, 64, None, 4)])
def test_c_abi_answers_the_shape_rules_before_any_gpu_work(K, N, G, forward, reverse):
    """Null pointers, no GPU: (192, 128, 64) is accepted in the forward direction, which needs real pointers (tests/test_awq_gemm_gpu.py)."""
    lib = _lib.load()
    for fn, want in ((lib.quick_repack_awq_gemm_to_mi355x, forward), (lib.quick_repack_mi355x_to_awq_gemm, reverse)):
        if want is None:
            continue
        assert fn(None, None, None, None, None, None, K, N, G, None) == want
        assert _lib.last_error() and f"K={K} N={N} G={G}" in _lib.last_error()
