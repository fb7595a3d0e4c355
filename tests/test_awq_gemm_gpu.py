"""AWQ GEMM-packing bridge on the GPU: the HIP repack kernels against packing.py's torch ops bit for bit, the BASELINE-size pin
against the hashes the reference's packer left, and WQLinear_GEMM's forward against the reference outputs of the exact_* fixtures.
Shapes: the smallest that reach every branch of the staging kernel -- one 128-channel block, N = 768 and 1408 (a 128-channel tail
behind 256-channel blocks), one to eight k tiles, G in {32, 64, 128}, K = 64 and 192 padded to 128 and 256."""
import hashlib
import os

import numpy as np
import pytest
import torch

from conftest import exact_layer, golden_files, load_golden, rel_err
from quick_amd import WQLinear_GEMM, WQLinear_QUICK, kernels, packing

pytestmark = pytest.mark.gpu

TOL = 2e-3      # tests/test_gemm_gpu.py's: the same kernels against the same ref_y
EXACT = golden_files("exact_")
ids = lambda p: os.path.basename(p)[:-4] if isinstance(p, str) else None


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _bits(t):
    return np.ascontiguousarray(t.cpu().numpy()).view(np.uint8)


def _same(got, want):
    got, want = tuple(got), tuple(want)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (i, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bits(a), _bits(b)), i


def _gemm(g):
    return _t(g["ref_gemm_qweight"]), _t(g["ref_gemm_qzeros"]), _t(g["ref_gemm_scales"])


def _quick(g):
    return _t(g["ref_qweight"]), _t(g["ref_qscales"]), _t(g["ref_qzeros"])


def _gemm_sd(g):
    qw, qz, sc = _gemm(g)
    return {"qweight": qw, "qzeros": qz, "scales": sc}


def _seeded(K, N, G, seed):
    return packing.pack_awq_gemm(*[_t(a) for a in exact_layer(K, N, G, seed)])


# GEMM-packing layers on the CPU, built once: the six fixtures, eleven 128-channel blocks x eight k tiles, and K = 192 padded to 256
_CASES = {}


def _case(name):
    if name not in _CASES:
        if name == "seeded_k1024n1408g128":
            _CASES[name] = _seeded(1024, 1408, 128, 77)
        elif name == "seeded_k192n128g64":
            _CASES[name] = _seeded(192, 128, 64, 78)
        else:
            _CASES[name] = _gemm(load_golden([p for p in EXACT if ids(p) == name][0]))
    return _CASES[name]


CASE_NAMES = [ids(p) for p in EXACT] + ["seeded_k1024n1408g128", "seeded_k192n128g64"]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_repack_kernels_equal_the_torch_ops_both_ways(device, name):
    gemm = _case(name)
    K, G = gemm[0].shape[0], gemm[0].shape[0] // gemm[2].shape[0]
    want = packing.awq_gemm_to_mi355x(*gemm)
    got = kernels.repack_awq_gemm_to_mi355x(*[t.to(device) for t in gemm])
    assert got[0].shape[0] * 4 == packing.padded_in_features(K, G)
    _same(got, want)
    if K % 128 == 0:
        _same(kernels.repack_mi355x_to_awq_gemm(*got), gemm)
    else:
        with pytest.raises(NotImplementedError, match="multiple of 128"):     # a padded copy is never turned back
            kernels.repack_mi355x_to_awq_gemm(*got, in_features=K)


def test_baseline_size_pin_through_both_bridges(device):
    g = load_golden(golden_files("pin_")[0])
    K, N, G = int(g["K"]), int(g["N"]), int(g["G"])
    gemm = _seeded(K, N, G, int(g["seed"]))
    mi = kernels.repack_awq_gemm_to_mi355x(*[t.to(device) for t in gemm])
    quick = kernels.repack_mi355x_to_cuda(*mi)
    sha = lambda t: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()
    assert tuple(sha(t) for t in quick) == (str(g["sha_qweight"]), str(g["sha_qscales"]), str(g["sha_qzeros"]))


@pytest.mark.parametrize("path", EXACT, ids=ids)
def test_wqlinear_gemm_forward_matches_the_reference(device, path):
    g = load_golden(path)
    K, N, G = int(g["K"]), int(g["N"]), int(g["G"])
    m = WQLinear_GEMM(4, G, K, N, False, "cpu")
    m.load_state_dict(_gemm_sd(g))
    m = m.to(device)
    y = m(_t(g["x"]).to(device))
    assert y.dtype == torch.float16 and tuple(y.shape) == g["ref_y"].shape
    err = rel_err(y.float().cpu().numpy(), g["ref_y"])
    print(f"{ids(path)}: rel_err {err:.3e}")
    assert err <= TOL
    if K % 128 == 0:
        # the same buffers as the QUICK route: a WQLinear_QUICK loaded from the reference's QUICK checkpoint of the layer and prepared
        assert m.is_prepared
        q = WQLinear_QUICK(4, G, K, N, False, "cpu")
        q.load_state_dict(dict(zip(("qweight", "scales", "qzeros"), _quick(g))))
        q = q.to(device).prepare()
        _same((m.qweight, m.scales, m.qzeros), (q.qweight, q.scales, q.qzeros))
    else:
        # through the padded copy: the buffers keep the GEMM packing
        assert not m.is_prepared and m._padded.packed is not None and m._padded.packed[0].shape[0] * 4 == 128
    sd = m.state_dict()
    _same((sd["qweight"], sd["qzeros"], sd["scales"]), _gemm(g))
    # ... and the QUICK checkpoint of the layer from the module as it stands (prepared, or GEMM packing with K = 64)
    sdq = WQLinear_QUICK.from_awq_gemm(m).state_dict()
    _same((sdq["qweight"], sdq["scales"], sdq["qzeros"]), _quick(g))


def test_from_awq_gemm_of_an_unprepared_gpu_module(device):
    g = load_golden([p for p in EXACT if "k256n512" in p][0])
    m = WQLinear_GEMM(4, int(g["G"]), int(g["K"]), int(g["N"]), False, "cpu")
    m.load_state_dict(_gemm_sd(g))
    m = m.to(device)
    q = WQLinear_QUICK.from_awq_gemm(m)                       # one repack launch
    assert q.is_prepared and not m.is_prepared and q.qweight.is_cuda
    sdq = q.state_dict()
    _same((sdq["qweight"], sdq["scales"], sdq["qzeros"]), _quick(g))
    y = q(_t(g["x"]).to(device))
    assert rel_err(y.float().cpu().numpy(), g["ref_y"]) <= TOL


def test_wqlinear_gemm_bias_fp32_input_and_leading_dimensions(device):
    g = load_golden([p for p in EXACT if "k256n512" in p][0])
    K, N, G = int(g["K"]), int(g["N"]), int(g["G"])
    assert g["x"].shape[0] >= 16
    bias = (torch.arange(N, dtype=torch.float32) / N - 0.5).half()
    m = WQLinear_GEMM(4, G, K, N, True, "cpu")
    m.load_state_dict(dict(_gemm_sd(g), bias=bias))
    m = m.to(device)
    x = _t(g["x"][:16]).float().reshape(2, 8, K).to(device)
    y = m(x)
    assert y.dtype == torch.float32 and tuple(y.shape) == (2, 8, N)
    want = g["ref_y"][:16].astype(np.float64) + bias.double().numpy()[None, :]
    err = rel_err(y.reshape(16, N).cpu().numpy(), want)
    print(f"bias / fp32: rel_err {err:.3e}")
    assert err <= TOL
