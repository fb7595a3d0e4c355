"""WQLinear_QUICK host logic and the C-ABI surface, no GPU needed."""
import ctypes
import json
import os
import sys
import re

import numpy as np
import pytest
import torch

import oracle
from conftest import ROOT, golden_files, load_golden
from quick_amd import WQLinear_QUICK, _lib, fuse_qkv_quick, packing
from quick_amd.build import LIB


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _linear(w):
    lin = torch.nn.Linear(w.shape[1], w.shape[0], bias=False)
    lin.weight.data = w.clone()
    return lin.half()


def _from_golden(g, **kw):
    return WQLinear_QUICK.from_linear(_linear(_t(g["weight"])), 4, int(g["G"]), False, _t(g["scales_nk"]), _t(g["zeros_nk"]), **kw)


def test_buffers_have_reference_shapes_and_names():
    m = WQLinear_QUICK(4, 128, 4096, 11008, True, "cpu")
    sd = m.state_dict()
    assert list(sd) == ["qweight", "qzeros", "scales", "bias"]
    assert sd["qweight"].shape == (1024, 5504) and sd["qweight"].dtype == torch.int32
    assert sd["qzeros"].shape == (32, 2752) and sd["qzeros"].dtype == torch.int32
    assert sd["scales"].shape == (32, 22016) and sd["scales"].dtype == torch.float16
    assert sd["bias"].shape == (11008,) and sd["bias"].dtype == torch.float16
    assert (m.k_split_1, m.k_split_2) == (2, 8)
    with pytest.raises(NotImplementedError):
        WQLinear_QUICK(8, 128, 256, 256, False, "cpu")
    assert WQLinear_QUICK(4, -1, 256, 128, False, "cpu").group_size == 256
    assert "w_bit=4" in m.extra_repr()


@pytest.mark.parametrize("path", [p for p in golden_files("exact_") if "k64" not in p] + golden_files("quant_"),
                         ids=lambda p: os.path.basename(p)[:-4])
def test_from_linear_state_dict_is_reference_format(path):
    g = load_golden(path)
    m = _from_golden(g)
    assert m.is_prepared                                    # in memory: MI355X order
    want = oracle.pack_mi355x(*oracle.unpack_cuda_order(g["ref_qweight"], g["ref_qscales"], g["ref_qzeros"]))
    for name, w in zip(("qweight", "scales", "qzeros"), want):
        assert np.array_equal(getattr(m, name).numpy().view(np.uint8), w.view(np.uint8))
    sd = m.state_dict()                                     # on disk: the reference's order, bit for bit
    assert np.array_equal(sd["qweight"].numpy(), g["ref_qweight"])
    assert np.array_equal(sd["scales"].numpy().view(np.uint16), g["ref_qscales"].view(np.uint16))
    assert np.array_equal(sd["qzeros"].numpy(), g["ref_qzeros"])

    # a fresh module loading that checkpoint is in reference order until prepared
    m2 = WQLinear_QUICK.from_linear(_linear(_t(g["weight"])), 4, int(g["G"]), init_only=True)
    assert not m2.is_prepared
    m2.load_state_dict(sd)
    assert not m2.is_prepared
    m2.prepare()
    assert m2.is_prepared
    for name in ("qweight", "scales", "qzeros"):
        assert torch.equal(getattr(m2, name), getattr(m, name))
    # load_state_dict copies in place: the module must notice it holds reference order again
    m2.load_state_dict(sd)
    assert not m2.is_prepared
    # moving / casting keeps the layout flag
    m3 = _from_golden(g).to("cpu")
    assert m3.is_prepared
    # attribute assignment (what fuse_qkv_quick and accelerate do) resets it
    m3.qweight = sd["qweight"].clone()
    assert not m3.is_prepared


def test_from_linear_k64_stays_in_checkpoint_format():
    g = load_golden([p for p in golden_files("exact_") if "k64" in p][0])
    m = _from_golden(g)
    assert not m.is_prepared
    assert np.array_equal(m.qweight.numpy(), g["ref_qweight"])
    assert m.prepare() is m and not m.is_prepared     # K = 64 is not tileable in the MI355X order: forward() runs on a padded copy
    assert np.array_equal(m.qweight.numpy(), g["ref_qweight"])


def test_fuse_qkv_unequal_widths_cpu():
    rng = np.random.default_rng(11)
    K, G = 256, 128
    mods, logical = [], []
    for N in (256, 128, 128):
        iw = rng.integers(0, 16, (K, N), dtype=np.uint8)
        z = rng.integers(0, 16, (K // G, N), dtype=np.uint8)
        s = rng.uniform(0.005, 0.025, (K // G, N)).astype(np.float16)
        m = WQLinear_QUICK(4, G, K, N, False, "cpu")
        m._set_packed(*[_t(a) for a in oracle.pack_mi355x(iw, s, z)], prepared=True)
        mods.append(m)
        logical.append((iw, s, z))
    fused = fuse_qkv_quick(None, *mods)
    assert fused.out_features == 512 and not fused.is_prepared
    full = oracle.pack_cuda_order(*[np.concatenate([l[i] for l in logical], axis=1) for i in range(3)])
    for name, w in zip(("qweight", "scales", "qzeros"), full):
        assert np.array_equal(getattr(fused, name).numpy().view(np.uint8), w.view(np.uint8))
    fused.prepare()
    iw2, s2, z2 = oracle.unpack_mi355x(fused.qweight.numpy(), fused.scales.numpy(), fused.qzeros.numpy())
    assert np.array_equal(iw2, np.concatenate([l[0] for l in logical], axis=1))


def test_forward_on_cpu_fails_loudly():
    g = load_golden(golden_files("exact_k128n128")[0])
    m = _from_golden(g)
    with pytest.raises(RuntimeError, match="GPU"):
        m(_t(g["x"]))


def test_c_abi_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build the library first: python -m quick_amd.build"
    header = open(os.path.join(ROOT, "include", "quick_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    header = re.sub(r"#ifdef QUICK_AMD_TOOLS.*?#endif", "", header, flags=re.S)      # (measurement aids of the tools library only)
    declared = set(re.findall(r"\b(quick_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    lib = ctypes.CDLL(LIB)
    for name in declared:
        assert hasattr(lib, name), name
    assert _lib.load().quick_amd_abi_version() == 1
    # argument validation runs before any GPU work
    rc = _lib.load().quick_w4a16_gemm_f16(None, None, None, None, None, None, 0, 1, 256, 100, 128, 8, None)
    assert rc == 1 and "cta_N" in _lib.last_error()
    rc = _lib.load().quick_w4a16_gemm_f16(None, None, None, None, None, None, 0, 1, 256, 128, 48, 8, None)
    assert rc == 1 and "multiple of 32" in _lib.last_error()
    rc = _lib.load().quick_w4a16_gemm_f16(None, None, None, None, None, None, 0, 1, 192, 128, 64, 8, None)
    assert rc == 4
    assert _lib.load().quick_w4a16_workspace_bytes(1, 4096, 4096, 128, 8) == 0
    # N = 1024 at M = 1: 64 channel tiles x 4 K slices, one 1 KiB fp32 slab each, behind 64 KiB of arrival counters and the
    # 16 MiB exchange zone (include/quick_amd.h, "workspace")
    assert _lib.load().quick_w4a16_workspace_bytes_ex(1, 4096, 1024, 128, 1, 0) == 65536 + (16 << 20) + 64 * 4 * 256 * 4   # (the r01 skinny kernel; AUTO: a lean launch, no workspace)
    assert _lib.load().quick_w4a16_workspace_bytes(1, 4096, 1024, 128, 8) == 0
    # exchange-K launch with two slices per tile: counters + zone, no slabs
    assert _lib.load().quick_w4a16_workspace_bytes_ex(512, 4096, 4096, 128, 4, 0) == 65536 + (16 << 20)


def test_span_and_profile_refuse_bad_arguments_before_any_gpu_work():
    """quick_w4a16_gemm_span / _profile: no launches, more span launches than the stamp buffer is sized for (256), no weight set and no
    result array are QUICK_ERR_INVALID_ARGUMENT, answered before anything touches the GPU (this test runs without one)."""
    lib = _lib.load()
    out = (ctypes.c_float * 4)()
    def call(fn, n_sets, iters, res):
        return fn(None, None, None, None, n_sets, None, None, 0, 1, 256, 256, 128, 0, 0, iters, res, None)
    for fn, text in ((lib.quick_w4a16_gemm_span, "bad span arguments"), (lib.quick_w4a16_gemm_profile, "bad profile arguments")):
        for n_sets, iters, res in ((1, 0, out), (0, 2, out), (1, 2, None)):
            assert call(fn, n_sets, iters, res) == 1 and text in _lib.last_error(), (text, n_sets, iters, _lib.last_error())
    assert call(lib.quick_w4a16_gemm_span, 1, 257, out) == 1 and "1..256" in _lib.last_error()


def test_product_library_has_no_timing_experiments():
    """Kernel-id bits 16-20 select ablation builds (wrong results on purpose) and phase stamps: a QUICK_AMD_TOOLS build only.
    The product library rejects them before any GPU work and exports no such kernels."""
    lib = _lib.load()
    for kid in (2 | (1 << 16), 3 | (16 << 16), 4 | (4 << 16), 1 << 16, 4 | (1 << 12), 4 | (1 << 13)):   # (the last two: the loader-wave / sixteen-wave exchange-K flavours)
        rc = lib.quick_w4a16_gemm_f16_ex(None, None, None, None, None, None, None, 0, 512, 4096, 4096, 128, kid, 0, None)
        assert rc == 1 and "QUICK_AMD_TOOLS" in _lib.last_error(), (kid, rc, _lib.last_error())
    import subprocess
    nm = "/opt/rocm/lib/llvm/bin/llvm-nm"
    if os.path.exists(nm):
        syms = subprocess.run([nm, "-C", LIB], capture_output=True, text=True).stdout
        # ABL is the last-but-one template argument of the ring kernel and the last of the wide / tiled / xk kernels: every shipped build has 0
        # (ring: 32 = span stamps, a measurement aid that changes no result)
        bad = [l for l in syms.splitlines() if re.search(r"w4a16_wide_kernel<\d+, \d+, \d+, [1-9]\d*>", l) or
               re.search(r"w4a16_xk_kernel<\d+, \d+, \d+, \d+, \d+, [1-9]\d*>", l) or "w4a16_xl_kernel" in l or
               re.search(r"w4a16_ring_kernel<\d+, \d+, \d+, \d+, (?!0,|32,)\d+, \d+>", l) or
               re.search(r"w4a16_tiled_kernel<\d+, \d+, \d+, \d+, [1-9]\d*, \d+>", l) or
               re.search(r"w4a16_xw_kernel<\d+, \d+, \d+, (?!0>|32>)\d+>", l) or "quick_prefetch" in l]     # (r04: four-wave kernels: 0 and the span stamps only)
        assert not bad, bad[:5]


def test_exchange_cus_override_keeps_k_slices_on_one_cu():
    """QUICK_AMD_EXCHANGE_CUS tells the planner how many CUs the K slices of an exchange-K launch may count on being co-resident
    (a CU mask the device attribute does not show); 0 = never split K across CUs that way.  Read once per process: subprocesses."""
    import subprocess
    import sys
    code = ("from quick_amd import kernels; print(kernels.plan_describe(65, 4096, 4096, 128)); "
            "print(kernels.plan_describe(512, 4096, 4096, 128, kernel_id=4 | (4 << 4) | (2 << 8)))")
    def run(env):
        e = dict(os.environ, QUICK_AMD_XM="0", **env)     # (the exchange families' pick: r06's mid-token kernels own this shape by default)
        return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=e).stdout.strip().splitlines()[-2:]
    auto, forced = run({})
    assert "slices=4" in auto and "slices=2" in forced
    for cus in ("0", "60"):           # 32 tiles of 128 x 128 (65 tokens) / 128 tiles (512 tokens): two slices each do not fit 60 CUs
        auto, forced = run({"QUICK_AMD_EXCHANGE_CUS": cus})
        assert "slices=4" not in auto and "slices=2" not in auto and "slices=1" in forced, (cus, auto, forced)
    auto, forced = run({"QUICK_AMD_EXCHANGE_CUS": "100"})      # 32 tiles x 2 slices fit, x 4 do not; 128 tiles x 2 do not
    assert auto.startswith("xw") and "slices=2" in auto and "slices=1" in forced
    auto, forced = run({"QUICK_AMD_EXCHANGE_CUS": "128"})      # [r06: the four-wave rules honour the override as the exchange-K ones always did]
    assert auto.startswith("xw") and "slices=4" in auto and "slices=1" in forced


def test_plan_describe_pins_the_shape_heuristics():
    """quick_w4a16_plan_describe is host-only; the expectations are the r01 measurements quoted in make_plan()."""
    from quick_amd import kernels

    def plan(M, K, N, G=128, **kw):
        return kernels.plan_describe(M, K, N, G, **kw)

    # decode shapes: one token -> deferred-zero table kernel, persistent over the channel blocks when there are many
    assert plan(1, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table grid=256x1x1")   # (r01-r04 skinny rules: family forced; AUTO runs the lean kernels at 1..4 tokens since r05, below)
    assert "grid=464x1x1" in plan(1, 4096, 22016, kernel_id=kernels.KERNEL_SKINNY)          # 1376 blocks in 3 rounds of <= 464
    assert "dequant=exact" in plan(8, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY)            # one block per workgroup: the table does not pay
    assert plan(64, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=4") and "deferred-zero-fragment" in plan(64, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY)   # (r01-r05's pick; AUTO: the r06 mid-token kernels, below)
    assert plan(64, 14336, 4096).startswith("xk tokens=64") and "slices=8" in plan(64, 14336, 4096)   # r03: 32 exchange-K tiles x 8 K slices = one round (x 4 at 65 x 4096 x 4096 there until r06: the mid-token kernels, and from 65 tokens the 128 x 128 four-wave tile)
    assert plan(32, 4096, 8192, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=4")   # 256 workgroups of 64 channels x 16 tokens: one round, 32 stages each
    assert plan(32, 4096, 28672).startswith("tiled")         # (r01: where the skinny workgroups would be two rounds, the tiled kernel, no K split needed)
    # K split until the 256 CUs are covered; the workspace is what workspace_bytes_ex says
    p = plan(128, 4096, 4096, kernel_id=kernels.KERNEL_TILED)
    assert "tokens=32 channels=128" in p and "ksplit=2" in p
    assert p.endswith(f"workspace={_lib.load().quick_w4a16_workspace_bytes_ex(128, 4096, 4096, 128, kernels.KERNEL_TILED, 0)}")
    p = plan(128, 11008, 4096)
    # (what workspace_bytes_ex asks for also covers the launch a SiLU * mul epilogue falls back to where the exchange-K plan cannot carry it)
    assert "slices=4" in p and int(p.rsplit("workspace=", 1)[1]) == 65536 + (16 << 20) <= _lib.load().quick_w4a16_workspace_bytes_ex(128, 11008, 4096, 128, 0, 0)
    # r06's mid-token kernels up to 56 tokens; 57..64 on this long-K layer that leaves 38 % of the CUs idle: the 64 x 128 four-wave tile with two exchange slices (3.5-6 % ahead on three boxes; r02-r04: wide tiles, three K slices)
    assert plan(56, 8192, 10240).startswith("xm tokens=64 channels=64 waves=8 grid=160x1") and plan(64, 8192, 10240).startswith("xw tokens=64 channels=128 waves=4 ring=8 queue=8 grid=160 slices=2")
    assert "grid=80x3 ksplit=3" in plan(64, 8192, 10240, kernel_id=kernels.KERNEL_TILED)
    # r01's tiled kernel (kernel_id TILED; the planner's own choice for G < 128): 256-channel tiles by how they quantise onto 256 CUs
    T = kernels.KERNEL_TILED
    assert "channels=128" in plan(512, 4096, 4096, kernel_id=T)           # 128 wide tiles would need a K split
    assert "channels=256" in plan(576, 4096, 4096, kernel_id=T)           # 144 wide tiles in one round beat 288 narrow ones
    assert "tokens=64 channels=256" in plan(1024, 4096, 4096, kernel_id=T)
    assert "tokens=128 channels=256 waves=4" in plan(2048, 4096, 4096, kernel_id=T)   # 256 four-wave tiles: one round
    assert "tokens=64" in plan(2560, 4096, 4096, kernel_id=T)                         # 320 of them would be two rounds
    assert "channels=128" in plan(192, 4096, 22016, kernel_id=T)          # 258 wide tiles = a second, nearly empty round
    assert "channels=256" in plan(128, 4096, 22016, kernel_id=T)
    assert "channels=256" in plan(8192, 4096, 22016, kernel_id=T)
    assert plan(512, 4096, 4096, G=64).startswith("tiled")                # small groups: the wide kernels need G % 128 == 0
    # r02: the wide kernels (32x32x16 MFMA, LDS-DMA) from 256 tokens, and from 64 once 64 x 128 tiles cover the chip
    assert plan(512, 4096, 4096, kernel_id=kernels.KERNEL_WIDE | (2 << 4) | (1 << 8) | (1 << 15) | (4 << 22)).startswith(
        "wide tokens=64 channels=128 waves=8 ring=4 grid=256x1")                                       # r02's pick there: the LDS-DMA ring, eight waves
    # r03: the exchange-K tiles (weights in an AGPR queue, five x slots, K slices on different CUs) wherever their workgroups fit one round
    X = kernels.KERNEL_XK
    assert plan(512, 4096, 4096, kernel_id=X).startswith("xk tokens=128") and plan(512, 4096, 4096, kernel_id=X | (2 << 4)).startswith(
        "xk tokens=64 channels=128 waves=8 ring=5 queue=4 grid=256 slices=1")                            # r03's bench line: one 64 x 128 tile per CU
    assert plan(64, 4096, 22016, kernel_id=X).startswith("xk tokens=64") and "slices=2" in plan(64, 4096, 12288, kernel_id=X)   # 172 / 96 tiles of 64 x 128 (r03's picks there; AUTO up to 64 tokens: r06's mid-token kernels, below)
    assert plan(128, 11008, 4096).startswith("xw tokens=128 channels=128") and "grid=128 slices=4" in plan(128, 11008, 4096)   # r05 audit: one row of 128 x 128 tiles x four slices (r03-r04: xk 64-token tiles; K = 4096: r06's mid-token kernels, below)
    assert plan(64, 13824, 5120).startswith("xk tokens=64 channels=128") and plan(80, 13824, 5120).startswith("xw tokens=128 channels=128") and plan(48, 5120, 5120).startswith("skinny ntw=4")        # 33..64 tokens where the mid-token kernels are not ahead: the r03-r05 picks
    # [r06] the mid-token kernels (w4a16_xm.hpp), where the audit has them ahead (profiles/r06_xm_audit.txt): 17..32 tokens -- the fewest channel pairs
    # per workgroup that cover the layer in one round; 33..64 tokens -- two 32-token tiles on layers of <= 8192 channels; K <= 8192
    assert plan(64, 4096, 4096).startswith("xm tokens=32 channels=32 waves=8 grid=128x2") and plan(33, 4096, 4096).startswith("xm tokens=32 channels=32 waves=8 grid=128x2")
    assert plan(17, 4096, 4096).startswith("xm tokens=32 channels=32 waves=8 grid=128x1") and plan(16, 4096, 4096).startswith("lean")
    assert plan(32, 4096, 12288).startswith("xm tokens=32 channels=64 waves=8 grid=192x1") and plan(24, 4096, 22016).startswith("xm tokens=32 channels=96 waves=8 grid=230x1")
    assert plan(64, 4096, 6144).startswith("xm tokens=32 channels=64 waves=8 grid=96x2") and plan(64, 8192, 8192).startswith("xm tokens=32 channels=64 waves=8 grid=128x2")
    assert plan(48, 4096, 22016).startswith("xm tokens=64 channels=96 waves=8 grid=230x1") and plan(64, 4096, 22016).startswith("xm tokens=64 channels=96 waves=8 grid=230x1")
    assert plan(64, 4096, 12288).startswith("xm tokens=64 channels=64 waves=8 grid=192x1") and plan(33, 5120, 15360).startswith("xm tokens=64 channels=64 waves=8 grid=240x1")
    # longer K: two 32-token tiles x one pair on the <= 4096-wide layers from 33 tokens up to K = 11008 (there: up to 48 tokens); the fragment kernels up to 32 tokens
    assert plan(48, 11008, 4096).startswith("xm tokens=32 channels=32 waves=8 grid=128x2") and plan(33, 11008, 4096).startswith("xm") and not plan(32, 11008, 4096).startswith("xm")
    assert not plan(56, 11008, 4096).startswith("xm") and not plan(64, 11008, 4096).startswith("xm")   # (the exchange launch is level or ahead there on two boxes of three)
    assert not plan(40, 14336, 4096).startswith("xm") and not plan(64, 14336, 4096).startswith("xm") and not plan(64, 13824, 5120).startswith("xm")
    # layers one round does not cover with three pairs per workgroup, and layers that leave > 30 % of the CUs idle below 56 tokens: the r03-r05 picks
    assert not plan(64, 4096, 28672).startswith("xm") and not plan(24, 8192, 57344).startswith("xm") and not plan(64, 28672, 8192).startswith("xm")
    assert not plan(48, 5120, 5120).startswith("xm") and plan(56, 5120, 5120).startswith("xm tokens=32 channels=64 waves=8 grid=80x2")
    # 65..128 tokens (profiles/r06_xm_audit_65_128.txt, three boxes): 32-token tiles x the fewest pairs that make one round on narrow layers with K <= 8192
    # (K = 11008 up to 80 tokens), 64-token tiles x <= 2 pairs up to 95 tokens (K = 4096: up to 128); the 128 x 128 four-wave tile elsewhere
    assert plan(65, 4096, 4096).startswith("xm tokens=32 channels=64 waves=8 grid=64x3") and plan(128, 4096, 4096).startswith("xm tokens=32 channels=64 waves=8 grid=64x4")
    assert plan(80, 11008, 4096).startswith("xm tokens=32 channels=64") and not plan(96, 11008, 4096).startswith("xm") and not plan(65, 14336, 4096).startswith("xm")
    assert plan(96, 5120, 5120).startswith("xm tokens=32 channels=64 waves=8 grid=80x3") and not plan(112, 5120, 5120).startswith("xm")
    assert plan(96, 4096, 6144).startswith("xm tokens=32 channels=96 waves=8 grid=64x3") and not plan(128, 4096, 6144).startswith("xm")
    assert plan(128, 4096, 8192).startswith("xm tokens=64 channels=64 waves=8 grid=128x2") and plan(80, 8192, 8192).startswith("xm tokens=64 channels=64") and plan(128, 8192, 8192).startswith("xm tokens=64 channels=64 waves=8 grid=128x2") and not plan(129, 8192, 8192).startswith("xm")   # (K <= 8192 up to 128 tokens since the end of r06: the four-slice exchange launch there follows the box, 19.6-32.8 us)
    assert plan(95, 4096, 8192).startswith("xm tokens=64 channels=64 waves=8 grid=128x2") and plan(95, 8192, 8192).startswith("xm tokens=64 channels=64")
    # ... and where the mid-token kernels are not taken, 65..95 tokens run the 128 x 128 four-wave tile as 96..128 do (r06 audit: the 64-token exchange tiles r03-r05 ran there were 10-32 % behind)
    assert plan(80, 4096, 12288).startswith("xw tokens=128 channels=128") and "slices=2" in plan(80, 4096, 12288) and plan(65, 4096, 22016).startswith("xw tokens=128 channels=128")
    assert plan(65, 14336, 4096).startswith("xw tokens=128 channels=128") and "slices=4" in plan(65, 14336, 4096) and plan(80, 8192, 10240).startswith("xw tokens=128 channels=128")
    assert not plan(65, 4096, 22016).startswith("xm") and not plan(65, 4096, 28672).startswith("xm") and not plan(129, 4096, 4096).startswith("xm")
    assert not plan(64, 4096, 4096, G=64).startswith("xm") and not plan(64, 4608, 4096, G=384).startswith("xm")               # G a power-of-two multiple of 128
    assert plan(40, 4096, 4096, kernel_id=kernels.KERNEL_XM | (3 << 4) | (2 << 8)).startswith("xm tokens=64 channels=96 waves=8 grid=43x1")   # forced: pairs, 64-token tiles; ragged last block
    # r04: the four-wave kernels with generated loops (w4a16_xw.hpp) from 160 tokens (96 on wide layers), picked by their own launch-time model
    assert plan(512, 4096, 4096).startswith("xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=2")    # the bench line: 128 x 128 tiles, two K slices
    # [r06, three-box audit] 129..256 tokens where four slices of the 128 x 128 tile are exactly one round (N = 4096): that tile, not two slices of 64 x 128 (the fit's pick, 4-10 % behind on every box)
    assert plan(256, 4096, 4096).startswith("xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=4") and "tokens=128 channels=128" in plan(160, 11008, 4096) and "slices=4" in plan(192, 11008, 4096)
    assert plan(160, 5120, 5120).startswith("xw tokens=64 channels=128") and "slices=2" in plan(160, 5120, 5120)      # (320 workgroups with four slices: the 64-token tile stays)
    assert plan(160, 4096, 6144).startswith("xw tokens=128 channels=128") and "slices=2" in plan(160, 4096, 6144)
    assert plan(1024, 4096, 4096).startswith("xw tokens=128 channels=128 waves=4 ring=4 queue=4 grid=256 slices=1")   # 256 tiles of 128 x 128: one round, nothing to exchange
    assert "slices=2" in plan(512, 11008, 4096) and "xw tokens=128 channels=128" in plan(512, 11008, 4096)            # 128 tiles x 2 slices of 43 stages
    assert plan(96, 4096, 22016).startswith("xw tokens=128 channels=128") and plan(96, 11008, 4096).startswith("xw tokens=128 channels=128")   # from 96 tokens on every layer since r05
    assert plan(2048, 3584, 18944).startswith("xw tokens=256 channels=256")                            # several rounds: the 256 x 256 tile, since r04 with the generated loop
    assert plan(2048, 4096, 4096).startswith("xw tokens=128 channels=256") and "xw tokens=256 channels=256 waves=4 ring=2 queue=2 grid=2752 slices=1" in plan(8192, 4096, 22016)
    assert plan(1024, 28672, 8192).startswith("xw tokens=128 channels=256 waves=4 ring=4 queue=4 grid=256 slices=1")   # (r02: 128 tiles of 256 x 256 x 2 K slices; 256 one-slice tiles of 128 x 256 are 10 % ahead)
    os.environ["QUICK_AMD_XW256"] = "0"
    try:
        assert plan(4096, 4096, 4096).startswith("wide tokens=128 channels=256")                       # (the A/B switch; r06: the product library no longer carries r02's hipcc-scheduled 256 x 256 tile -- it spilled -- only tools builds do)
    finally:
        del os.environ["QUICK_AMD_XW256"]
    assert plan(4096, 4096, 4096).startswith("xw tokens=256 channels=256 waves=4 ring=2 queue=2 grid=256 slices=1")
    assert plan(384, 4096, 12288).startswith("xw tokens=128 channels=256 waves=4 ring=4 queue=4 grid=144 slices=1")   # 41.6 us (r03's 128 x 256 wide tile: 51.2)
    assert plan(512, 4096, 4096, kernel_id=kernels.KERNEL_XW).startswith("xw tokens=128 channels=256") and "slices=4" in plan(512, 4096, 4096, kernel_id=kernels.KERNEL_XW)
    assert not plan(512, 4608, 4096, G=384).startswith("xw") and not plan(512, 4608, 4096, G=384, kernel_id=kernels.KERNEL_XW).startswith("xw")  # G / 128 must be a power of two
    W = kernels.KERNEL_WIDE
    assert "tokens=256 channels=128" in plan(4096, 8192, 8192, kernel_id=W | (8 << 4) | (1 << 8))      # explicit tile
    assert "tokens=128 channels=256" in plan(4096, 8192, 8192, kernel_id=W | (8 << 4) | (2 << 8))      # (r06: the hipcc-scheduled 256 x 256 tile left the product library -- 128 x 256 tiles answer)
    assert "waves=8 ring=6" in plan(512, 4096, 4096, kernel_id=W | (2 << 4) | (1 << 8) | (1 << 15))   # eight-wave ring
    assert "ring=0" in plan(512, 4096, 4096, kernel_id=W | (2 << 4) | (1 << 8) | (1 << 12))           # double-buffered instead
    # r02 planner audit (profiles/r02_planner_audit*.jsonl): the rules it added
    assert "waves=16" in plan(1, 11008, 4096, kernel_id=kernels.KERNEL_SKINNY) and "waves=8" in plan(1, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY) and "waves=8" in plan(1, 4096, 22016, kernel_id=kernels.KERNEL_SKINNY)   # long K, one workgroup per CU
    assert "waves=16" in plan(1, 11008, 4096, G=64) and "waves=8" in plan(1, 11008, 4096, G=32)                            # (not with four units per k-tile)
    assert plan(16, 4096, 6144, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=2") and "deferred-zero-fragment" in plan(16, 4096, 6144, kernel_id=kernels.KERNEL_SKINNY)    # 384 blocks: one round of 192
    assert plan(6, 8192, 8192, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=2") and plan(4, 28672, 8192).startswith("skinny ntw=4")
    assert "deferred-zero-table" in plan(12, 4096, 22016, kernel_id=kernels.KERNEL_SKINNY) and plan(16, 4096, 22016, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=4")
    # [r05] 9..16 tokens on the Llama-2-70B layers: the straight-line eight-tile fragment kernel where K / 128 = 8 waves x slices x {2, 4, 7, 8} and the
    # blocks come in multiples of 64 (measured ahead there); 80 blocks (the fused qkv) stay with four tiles
    # [r06, late] ... with SEVEN tiles per workgroup where that makes fuller rounds of one workgroup per CU: 57344 = 448 blocks of 128 (1.75 rounds) = 512 of 112 (two),
    # 28672 = 224 of 128 = 256 of 112 (every CU busy); the forced eight-tile id keeps eight
    assert plan(16, 8192, 57344).startswith("skinny ntw=7") and "grid=512x1x1 ksplit=1" in plan(16, 8192, 57344)
    assert "grid=448x1x1 ksplit=1" in plan(16, 8192, 57344, kernel_id=kernels.KERNEL_SKINNY | (8 << 4)) and plan(16, 8192, 1792, kernel_id=kernels.KERNEL_SKINNY | (7 << 4)).startswith("skinny ntw=7")
    assert plan(16, 28672, 8192).startswith("skinny ntw=8") and "grid=64x1x4 ksplit=4" in plan(16, 28672, 8192)
    assert plan(16, 8192, 8192).startswith("skinny ntw=8") and "ksplit=4" in plan(16, 8192, 8192) and plan(9, 8192, 57344).startswith("skinny ntw=7")
    assert plan(16, 8192, 10240).startswith("skinny ntw=4") and plan(8, 8192, 57344).startswith("skinny ntw=1") and not plan(17, 8192, 57344).startswith("skinny ntw=8")
    assert plan(16, 8192, 28672).startswith("skinny ntw=7") and "grid=256x1x1 ksplit=1" in plan(16, 8192, 28672) and plan(16, 8192, 16384).startswith("skinny ntw=4")   # (one slice from 192 blocks; 128 blocks x 2 slices measured behind)
    # r03 audit: from five tokens no LDS copy of x outside the table flavour; one-tile launches with K = 4096 run sixteen waves
    assert plan(6, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=1 waves=16 x=l2 dequant=exact") and "waves=8 x=lds" in plan(4, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY)
    assert plan(7, 4096, 12288).startswith("skinny ntw=4 waves=8 x=l2") and plan(10, 11008, 4096).startswith("skinny ntw=4 waves=8 x=l2")
    # [r06 audit of the lean rule, profiles/r06_lean_rule_audit.txt] 5 / 6 tokens on 768 channel blocks: lean; a long K only where every workgroup is co-resident
    assert plan(6, 4096, 12288).startswith("lean ntw=1 waves=8") and plan(8, 8192, 4096).startswith("lean ntw=1 waves=8 tiles_per_wave<=8 grid=256x1")
    assert plan(8, 8192, 8192).startswith("skinny ntw=2") and plan(12, 5120, 5120).startswith("skinny ntw=4") and plan(6, 11008, 8192).startswith("skinny ntw=2") and plan(5, 8192, 8192).startswith("lean ntw=2 waves=16")
    # third audit (17..64 tokens, layer shapes the rules were not tuned on): the four-tile skinny kernel by its own geometry
    assert plan(32, 4096, 6144, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=4") and plan(32, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=4")    # one round of workgroups, <= 64 stages each (AUTO at 17..32 tokens: the r06 mid-token kernels)
    assert plan(48, 5120, 5120).startswith("skinny ntw=4") and plan(55, 5120, 5120).startswith("xk tokens=64")    # 320 skinny workgroups would be two rounds; r03: 40 tiles x 4 slices (from 56 tokens: r06's mid-token kernels)
    assert plan(32, 13824, 5120).startswith("tiled") and "slices=8" in plan(48, 14336, 4096)                      # slices of > 64 stages; r03 from 33 tokens: 32 tiles x 8 slices of 14 stages
    assert "tokens=32 channels=128 waves=8 grid=192x1 ksplit=1" in plan(64, 4096, 12288, kernel_id=T)              # twice the tiles, nothing to reduce
    assert plan(48, 8192, 10240).startswith("xm tokens=64 channels=64 waves=8 grid=160x1")   # (r06; r05: four-wave 64 x 128 tiles x two slices; r02-r04: wide tiles, three K slices)
    assert plan(64, 11008, 4096, kernel_id=T).startswith("tiled tokens=32") and "slices=8" in plan(48, 11008, 4096, kernel_id=X)
    assert plan(64, 28672, 8192).startswith("xk tokens=64") and "slices=4" in plan(64, 28672, 8192)               # long K slices fill the chip
    assert "slices=4" in plan(48, 28672, 8192) and "slices=4" in plan(64, 8192, 8192, kernel_id=kernels.KERNEL_XK | (2 << 4)) and "slices=4" in plan(64, 4096, 8192, kernel_id=kernels.KERNEL_XK | (2 << 4))
    assert "deferred-zero-table" in plan(3, 13824, 5120, kernel_id=kernels.KERNEL_SKINNY) and "dequant=exact" in plan(3, 18944, 3584, kernel_id=kernels.KERNEL_SKINNY)              # M = 3: the table from 256 channel blocks
    assert plan(8, 11008, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=4") and plan(6, 11008, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny ntw=1")    # x too large for LDS: share the L2 fragments (r03 audit: among four tiles)
    # [r05] the lean small-M kernels: 1..4 tokens wherever a build exists (G % 128 == 0, k tiles between the waves and 8 / 12 per wave), up to 16
    # tokens on layers of <= 512 channel blocks; two channel tiles per workgroup where that fills the rounds no worse
    L = kernels.KERNEL_LEAN
    assert plan(1, 4096, 4096).startswith("lean ntw=1 waves=8 tiles_per_wave<=4 grid=256x1") and "workspace=0" in plan(1, 4096, 4096)
    assert plan(1, 4096, 12288).startswith("lean ntw=1 waves=8") and plan(1, 4096, 22016).startswith("lean ntw=2 waves=8 tiles_per_wave<=4 grid=688x1")
    assert plan(1, 11008, 4096).startswith("lean ntw=1 waves=16 tiles_per_wave<=8") and plan(1, 8192, 8192).startswith("lean ntw=2 waves=16 tiles_per_wave<=4 grid=256x1")
    assert plan(1, 8192, 10240).startswith("lean ntw=1 waves=8 tiles_per_wave<=8") and plan(4, 4096, 22016).startswith("lean ntw=2")
    assert plan(16, 4096, 4096).startswith("lean") and plan(8, 4096, 8192).startswith("lean") and plan(17, 4096, 4096).startswith("xm")
    assert plan(7, 4096, 12288).startswith("skinny") and plan(5, 4096, 22016).startswith("skinny") and plan(7, 4096, 22016).startswith("skinny")   # 5..7 tokens on wide layers: the r01-r04 kernels (r06: 5 / 6 tokens up to 768 blocks are lean)
    # 8..16 tokens on wide layers: one persistent workgroup per CU (x staged once; a one-block workgroup would fetch more bytes of x than of weights)
    assert plan(8, 4096, 22016).startswith("lean ntw=2 waves=8 tiles_per_wave<=4 grid=256x1") and plan(16, 4096, 22016).startswith("lean ntw=1 waves=8 tiles_per_wave<=4 grid=256x1")
    assert plan(16, 4096, 12288).startswith("lean ntw=1") and "grid=256x1" in plan(16, 4096, 12288) and plan(16, 8192, 57344).startswith("skinny")   # (x of 16 x 8192 does not fit LDS)
    assert plan(1, 28672, 8192).startswith("skinny") and plan(1, 512, 256).startswith("skinny")              # 224 / 4 k tiles: no build
    assert plan(1, 4096, 4096, G=64).startswith("skinny") and plan(2, 4096, 4096, G=256).startswith("lean")
    assert "tiles_per_wave<=0" in plan(1, 28672, 8192, kernel_id=L) and "tiles_per_wave<=0" in plan(1, 4096, 4096, G=64, kernel_id=L)   # forced without a build: UNSUPPORTED at launch
    assert plan(1, 4096, 4096, kernel_id=L | (2 << 4) | (4 << 8)).startswith("lean ntw=2 waves=16 tiles_per_wave<=4 grid=128x1")
    assert kernels.can_fuse_rmsnorm(1, 4096, 12288, 128) and kernels.can_fuse_rmsnorm(16, 4096, 4096, 128)
    # forcing a family / a split through the kernel id and grid_split_k
    assert plan(512, 4096, 4096, kernel_id=kernels.KERNEL_SKINNY).startswith("skinny")
    assert "ksplit=4" in plan(64, 4096, 4096, kernel_id=kernels.KERNEL_TILED, grid_split_k=4)
    with pytest.raises(ValueError, match="cta_N"):
        plan(4, 4096, 4100)


def test_rmsnorm_prologue_is_not_fused_on_very_large_fragment_layers():
    """r05: the fragment flavour of the skinny kernel carries the norm in registers; above K * N = 2^28 (Llama-2-70B's gate_up at 9..16 tokens)
    a separate RMSNorm launch is faster (profiles/r05_decode70_ab.txt), so can_fuse_rmsnorm answers no there and yes below."""
    from quick_amd import kernels
    assert "deferred-zero-fragment" in kernels.plan_describe(16, 8192, 57344, 128) and not kernels.can_fuse_rmsnorm(16, 8192, 57344, 128)
    assert "deferred-zero-fragment" in kernels.plan_describe(16, 8192, 10240, 128) and kernels.can_fuse_rmsnorm(16, 8192, 10240, 128)
    assert kernels.can_fuse_rmsnorm(8, 8192, 57344, 128) and kernels.can_fuse_rmsnorm(1, 8192, 57344, 128)      # table flavour / lean: x in LDS


def test_forced_four_wave_id_checks_the_width_against_its_own_tile():
    """XW | 8 token blocks | bit 12 means 256-channel tiles (bit 12 is ignored at 8 blocks); with N % 256 == 128 the launch
    used to drop the last 128 channels and answer QUICK_OK.  The width is now checked against the tile the id resolves to."""
    from quick_amd import kernels
    XW = kernels.KERNEL_XW if hasattr(kernels, "KERNEL_XW") else 5
    for kid in (XW | (8 << 4) | (1 << 12), XW | (8 << 4), XW):                      # 256-channel tiles
        assert kernels.plan_describe(256, 1024, 384, 128, kernel_id=kid).startswith("tiled"), hex(kid)
        assert kernels.plan_describe(256, 1024, 512, 128, kernel_id=kid).startswith("xw "), hex(kid)
    for kid in (XW | (1 << 12), XW | (2 << 4)):                                      # 128-channel tiles take N = 384
        p = kernels.plan_describe(256, 1024, 384, 128, kernel_id=kid)
        assert p.startswith("xw ") and "channels=128" in p, (hex(kid), p)


@pytest.mark.parametrize("K,N,G", [(96, 128, 32), (320, 256, 64), (192, 128, 96), (480, 128, 32)])
def test_in_features_not_a_multiple_of_128_runs_on_a_zero_padded_copy(K, N, G):
    """The reference takes in_features % 32 == 0 (csrc/gemm_cuda_quick.cu:1479-1484); the MI355X weight order needs 128-k tiles.
    Such a layer (only possible with a group size that is not a multiple of 128) keeps its buffers in the checkpoint order and
    computes on a copy padded along K with weights 0 / zero points 0 / scales 0: the copy dequantises to the layer's weights
    followed by exact zeros."""
    from quick_amd import kernels
    x, iw, s, z = oracle.make_synthetic(3, K, N, G, seed=K + N + G)
    ref = [torch.from_numpy(np.ascontiguousarray(a)) for a in oracle.pack_cuda_order(iw, s, z)]
    Kp = kernels.padded_in_features(K, G)
    assert Kp % 128 == 0 and Kp % G == 0 and Kp >= K and Kp - K < 128 * G // np.gcd(128, G)
    packed = kernels._padded_mi355x(*ref)
    assert packed[0].shape[0] * 4 == Kp
    iwp, sp, zp = oracle.unpack_mi355x(*[t.numpy() for t in packed])
    w = oracle.dequantize(iwp, sp, zp, G)
    assert np.array_equal(w[:K], oracle.dequantize(iw, s, z, G)) and not w[K:].any()
    m = WQLinear_QUICK(4, G, K, N, False, "cpu")
    m.load_state_dict({"qweight": ref[0], "scales": ref[1], "qzeros": ref[2]})
    assert m.prepare() is m and not m.is_prepared                      # stays in the reference's order
    assert all(torch.equal(a, b) for a, b in zip((m.qweight, m.scales, m.qzeros), ref))


def test_quick_kernels_shim_exports_reference_symbol():
    import quick_kernels
    assert callable(quick_kernels.gemm_forward_cuda_quick)
    x = torch.zeros(1, 128, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="Half|float16"):
        quick_kernels.gemm_forward_cuda_quick(x, torch.zeros(32, 64, dtype=torch.int32), torch.zeros(1, 256, dtype=torch.float16),
                                              torch.zeros(1, 32, dtype=torch.int32), 8)


def test_compiled_quick_kernels_extension_builds_and_exports_the_symbol():
    """quick_amd/csrc/quick_kernels_ext.cpp (pybind11 over the C ABI, the shape of the reference's csrc/pybind.cpp:5-8)
    builds with torch.utils.cpp_extension -- no GPU needed -- and rejects CPU tensors like the ctypes shim does."""
    from quick_amd.build_ext import build_quick_kernels_ext
    ext = build_quick_kernels_ext()
    assert callable(ext.gemm_forward_cuda_quick)
    x = torch.zeros(1, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ext.gemm_forward_cuda_quick(x, torch.zeros(32, 64, dtype=torch.int32), torch.zeros(1, 256, dtype=torch.float16),
                                    torch.zeros(1, 32, dtype=torch.int32), 8)
    with pytest.raises(ValueError, match="split_k_iters"):
        ext.gemm_forward_cuda_quick(x, torch.zeros(32, 64, dtype=torch.int32), torch.zeros(1, 256, dtype=torch.float16),
                                    torch.zeros(1, 32, dtype=torch.int32), 0)


# ------------------------------------------------------------------------------------------------
# quantizer hook-up (quick/awq/quantize/quantizer.py:46-72, 141-174)
# ------------------------------------------------------------------------------------------------
def test_pseudo_quantize_and_quantize_linear_reproduce_the_reference_fixture():
    """tests/golden/quant_k256n256g128.npz holds what the reference's pseudo_quantize_tensor + from_linear made of a
    seeded weight (gen_golden.py); the same seed through quick_amd.quantize must give the same bits."""
    import torch
    from conftest import golden_files, load_golden
    from quick_amd import pseudo_quantize_tensor, quantize_linear
    g = load_golden(golden_files("quant_")[0])
    K, N, G = int(g["K"]), int(g["N"]), int(g["G"])
    w = (torch.randn(N, K, generator=torch.Generator().manual_seed(400)) * 0.03).half()
    wq, s, z = pseudo_quantize_tensor(w.clone(), 4, G, get_scale_zp=True)
    assert np.array_equal(wq.numpy().view(np.uint16), g["weight"].view(np.uint16))
    assert np.array_equal(s.numpy().view(np.uint16), g["scales_nk"].view(np.uint16))
    assert np.array_equal(z.numpy().view(np.uint16), g["zeros_nk"].view(np.uint16))
    lin = torch.nn.Linear(K, N, bias=False)
    lin.weight.data = w.float()
    sd = quantize_linear(lin, 4, G).state_dict()          # reference packed order
    assert np.array_equal(sd["qweight"].numpy(), g["ref_qweight"])
    assert np.array_equal(sd["qzeros"].numpy(), g["ref_qzeros"])
    assert np.array_equal(sd["scales"].numpy().view(np.uint16), g["ref_qscales"].view(np.uint16))


def test_quantize_module_linears_replaces_and_skips():
    import torch
    from quick_amd import WQLinear_QUICK, quantize_module_linears
    torch.manual_seed(0)
    m = torch.nn.ModuleDict({"attn": torch.nn.ModuleDict({"q_proj": torch.nn.Linear(256, 128), "o_proj": torch.nn.Linear(128, 256, bias=False)}),
                             "lm_head": torch.nn.Linear(256, 128, bias=False)})
    done = quantize_module_linears(m, 4, 128, modules_to_not_convert=("lm_head",))
    assert sorted(done) == ["attn.o_proj", "attn.q_proj"]
    assert isinstance(m["attn"]["q_proj"], WQLinear_QUICK) and m["attn"]["q_proj"].bias is not None
    assert isinstance(m["lm_head"], torch.nn.Linear)
    with pytest.raises(ValueError):
        quantize_module_linears(torch.nn.ModuleDict({"x": torch.nn.Linear(192, 128)}), 4, 128)


# ------------------------------------------------------------------------------------------------
# layout tracking: inference mode, copies, pickles
# ------------------------------------------------------------------------------------------------
def _reference_checkpoint_module():
    g = load_golden(golden_files("exact_k128n256")[0])
    m = WQLinear_QUICK(4, int(g["G"]), int(g["K"]), int(g["N"]), False, "cpu")
    m.load_state_dict({"qweight": _t(g["ref_qweight"]), "scales": _t(g["ref_qscales"]), "qzeros": _t(g["ref_qzeros"])})
    return g, m


def test_prepare_inside_inference_mode():
    """The reference runs every forward under torch.inference_mode() (quick/awq/modules/fused/model.py:76,
    examples/benchmark.py:45): the lazy prepare() of the first forward then creates inference tensors, which have no
    version counter."""
    g, m = _reference_checkpoint_module()
    assert not m.is_prepared
    with torch.inference_mode():
        m.prepare()
        assert m.is_prepared
        assert m.qweight.is_inference()
    assert m.is_prepared                                                # ... and still outside
    sd = m.state_dict()
    assert np.array_equal(sd["qweight"].numpy(), g["ref_qweight"])
    # a module CREATED under inference mode, loaded there too
    with torch.inference_mode():
        m2 = WQLinear_QUICK(4, int(g["G"]), int(g["K"]), int(g["N"]), False, "cpu")
        m2.load_state_dict({k: v.clone() for k, v in sd.items()})
        assert not m2.is_prepared
        m2.prepare()
        assert m2.is_prepared and torch.equal(m2.qweight, m.qweight)


def test_deepcopy_and_pickle_keep_the_layout():
    import copy
    import io
    g, m = _reference_checkpoint_module()
    m.prepare()
    for clone in (copy.deepcopy(m), torch.load(io.BytesIO(_save_bytes(m)), weights_only=False)):
        assert clone.qweight.data_ptr() != m.qweight.data_ptr()
        assert clone.is_prepared                                        # same MI355X-order bits in new storages
        assert torch.equal(clone.qweight, m.qweight)
        sd = clone.state_dict()                                         # ... so the checkpoint is still the reference's
        assert np.array_equal(sd["qweight"].numpy(), g["ref_qweight"])
        assert np.array_equal(sd["qzeros"].numpy(), g["ref_qzeros"])
        assert np.array_equal(sd["scales"].numpy().view(np.uint16), g["ref_qscales"].view(np.uint16))
        clone.load_state_dict(sd)                                       # an in-place rewrite is still noticed
        assert not clone.is_prepared
    unprepared = copy.deepcopy(_reference_checkpoint_module()[1])
    assert not unprepared.is_prepared


def test_load_state_dict_right_after_a_copy_marks_reference_order():
    """deepcopy / unpickle carry `prepared` without a storage key (they re-key on first use); a load_state_dict that follows
    BEFORE any such use copies reference-order bits into the storages in place, and under inference mode there is no version
    counter to notice it.  The load itself must reset the layout."""
    import copy
    import io
    g, m = _reference_checkpoint_module()
    ckpt = {k: v.clone() for k, v in m.state_dict().items()}            # reference order
    m.prepare()
    for clone in (copy.deepcopy(m), torch.load(io.BytesIO(_save_bytes(m)), weights_only=False)):
        clone.load_state_dict(ckpt)                                     # no is_prepared / forward in between
        assert not clone.is_prepared
        assert torch.equal(clone.qweight, ckpt["qweight"])
        clone.prepare()
        assert clone.is_prepared and torch.equal(clone.qweight, m.qweight)
    with torch.inference_mode():                                        # inference tensors: version 0 for ever
        m3 = WQLinear_QUICK(4, int(g["G"]), int(g["K"]), int(g["N"]), False, "cpu")
        m3.load_state_dict({k: v.clone() for k, v in ckpt.items()})
        m3.prepare()
        assert m3.is_prepared
        m3.load_state_dict({k: v.clone() for k, v in ckpt.items()})     # in place, no version bump
        assert not m3.is_prepared and torch.equal(m3.qweight, ckpt["qweight"])
    # a partial load must not mix the two orders: the tensors that are not in the checkpoint go back to the reference's order
    m4 = copy.deepcopy(m)
    assert m4.is_prepared
    m4.load_state_dict({"scales": ckpt["scales"].clone()}, strict=False)
    assert not m4.is_prepared and torch.equal(m4.qweight, ckpt["qweight"]) and torch.equal(m4.qzeros, ckpt["qzeros"])


def _save_bytes(module):
    import io
    buf = io.BytesIO()
    torch.save(module, buf)
    return buf.getvalue()


def test_gemm_forward_validates_optional_tensors():
    """Everything handed to the library as a raw pointer is checked on the Python side first (no GPU needed: the checks
    come before the device check of the tensors they concern only where the message says so)."""
    from quick_amd import kernels
    x = torch.zeros(2, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        kernels.gemm_forward(x, torch.zeros(32, 64, dtype=torch.int32), torch.zeros(1, 256, dtype=torch.float16),
                             torch.zeros(1, 32, dtype=torch.int32))


def test_no_kernel_of_the_library_traps(tmp_path):
    """r03's exchange-K kernels ended a wave that had polled ~4 s for a partner slice with s_trap -- a dead GPU context when a second
    process or another stream kept the partner off the chip.  Since r04 a waiting wave gives its part up and
    leaves, and the last slice to arrive finishes it (w4a16_xk.hpp, w4a16_xw.hpp): the shipped gfx950 code objects contain no trap."""
    import shutil
    import subprocess
    from quick_amd import _lib
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump here")
    lib = tmp_path / "lib.so"
    shutil.copy(_lib.LIB, lib)
    subprocess.run([objdump, "--offloading", str(lib)], capture_output=True, text=True, check=True)
    objs = [p for p in tmp_path.iterdir() if "gfx950" in p.name]
    assert objs, list(tmp_path.iterdir())
    mfma = 0
    for o in objs:
        text = subprocess.run([objdump, "-d", str(o)], capture_output=True, text=True, check=True).stdout
        assert "s_trap" not in text, o.name
        mfma += text.count("v_mfma_f32_32x32x16_f16")
    assert mfma > 1000     # (the disassembly really is the GEMM kernels)


def test_no_kernel_of_the_library_spills_registers(tmp_path):
    """[r06, VERDICT r05 #6] The kernels' design is register-resident (the counterpart of the reference's compute_gemm, csrc/gemm_cuda_quick.cu:20-455:
    weights HBM -> registers -> matrix core, nothing through memory on the way).  r01-r05 shipped instantiations that spilled to scratch memory
    (sixteen-wave skinny builds with two and four tiles, r01's 32x32x16 tiled flavour, r02's hipcc-scheduled 256 x 256 tile); r06 retired them or
    moved them to tools builds.  Every kernel descriptor of the shipped gfx950 code objects -- the GEMM families the planner can reach AND the
    forced-id ones, the repack and decode kernels -- declares a private segment of 0 bytes, and the disassembly has no scratch_ instruction."""
    import re
    import shutil
    import subprocess
    from quick_amd import _lib
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("no llvm-objdump / llvm-readelf here")
    lib = tmp_path / "lib.so"
    shutil.copy(_lib.LIB, lib)
    subprocess.run([objdump, "--offloading", str(lib)], capture_output=True, text=True, check=True)
    objs = [p for p in tmp_path.iterdir() if "gfx950" in p.name]
    assert objs, list(tmp_path.iterdir())
    kernels_seen, spilling = 0, []
    for o in objs:
        notes = subprocess.run([readelf, "--notes", str(o)], capture_output=True, text=True, check=True).stdout
        for block in notes.split("- .agpr_count")[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            priv = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
            assert name and priv, block[:200]
            kernels_seen += 1
            if int(priv.group(1)) > 0:
                spilling.append((name.group(1), int(priv.group(1))))
        text = subprocess.run([objdump, "-d", str(o)], capture_output=True, text=True, check=True).stdout
        assert not re.search(r"\bscratch_(load|store)", text), o.name
    assert kernels_seen > 300 and not spilling, spilling


def _gfx950_disassemblies(tmp_path):
    """llvm-objdump -d --symbolize-operands of every gfx950 code object in the product library -> list of paths"""
    import shutil
    import subprocess
    from quick_amd import _lib
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("no llvm-objdump here")
    lib = tmp_path / "lib.so"
    shutil.copy(_lib.LIB, lib)
    subprocess.run([objdump, "--offloading", str(lib)], capture_output=True, text=True, check=True, cwd=tmp_path)
    out = []
    for o in sorted(p for p in tmp_path.iterdir() if "gfx950" in p.name):
        dis = tmp_path / (o.name + ".dis")
        dis.write_text(subprocess.run([objdump, "-d", "--symbolize-operands", str(o)], capture_output=True, text=True, check=True).stdout)
        out.append(str(dis))
    assert out
    return out


def _tool(name):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_every_mfma_of_the_library_keeps_its_distance_from_the_vector_alu(tmp_path):
    """[r06, VERDICT r05 #2] gfx950 does not interlock the matrix core against the vector ALU: software pads MFMA -> VALU read (7 / 10 wait
    states for the 4- / 8-pass instructions the kernels use), MFMA -> VALU overwrite of the destination (4 / 8), MFMA SrcC -> VALU overwrite
    (0 / 3), VALU write -> MFMA read (1) -- the table MEASURED by tools/mfma_valu_read_hazard.hip / mfma_valu_write_hazard.hip
    (profiles/r06_mfma_hazards.txt).  hipcc pads what it can see; an instruction inside an asm statement it cannot, which is how r05's
    unconditional-request chunk loop came to compute tiles wrong.  tools/mfma_hazard_lint.py reads the ISA of EVERY kernel of
    the shipped code objects -- hipcc-scheduled and generated loops alike -- and finds no pair closer than the table."""
    lint = _tool("mfma_hazard_lint")
    vm = _tool("vmcnt_lint")
    kernels_seen = mfmas = 0
    for dis in _gfx950_disassemblies(tmp_path):
        for name, items in vm.parse(dis).items():
            if not any(k == "ins" and v.mn == "s_endpgm" for k, v in items):
                continue
            findings, n = lint.check_kernel(name, items)
            assert not findings, findings[:3]
            kernels_seen += 1
            mfmas += n
    assert kernels_seen > 300 and mfmas > 10000


def test_every_load_of_the_library_is_waited_for_before_its_registers_are_touched(tmp_path):
    """[r06, VERDICT r05 #2] The other suspect of the r04 / r05 wrong-results builds: wait counts.  tools/vmcnt_lint.py walks the control-flow graph
    of every kernel with the in-order model behind s_waitcnt vmcnt (verified on the part across load classes: tools/vmcnt_order_probe.hip,
    5.2 M rounds) and demands that no instruction touches a register a load in flight is going to write -- for hipcc's waits and for the counted
    waits of the generated loops (w4a16_xw_loop.inc, w4a16_xm_loop.inc) alike.  Not asserted: the exchange-K family (w4a16_xk_kernel), whose
    hand-counted waits are chosen by the same wave-uniform predicates that guard its requests -- the checker is path-insensitive and reports the
    combinations of a guarded request with the other branch's wait; its results are pinned by the parity suite and 10 M contended
    launches instead."""
    vm = _tool("vmcnt_lint")
    checked = loads = 0
    for dis in _gfx950_disassemblies(tmp_path):
        for name, items in vm.parse(dis).items():
            if "w4a16_xk_kernel" in name or not any(k == "ins" and v.mn == "s_endpgm" for k, v in items):
                continue
            findings, n = vm.check_kernel(name, items)
            assert not findings, findings[:3]
            checked += 1
            loads += n
    assert checked > 300 and loads > 5000


def test_no_vector_alu_instruction_hides_in_an_asm_statement_of_hipcc_scheduled_code():
    """[r06] The source-level half of the above: in the hipcc-scheduled translation units (everything but the generated loops, which are whole
    K loops with their own asserted distances) no asm statement contains a VALU instruction that computes -- and_or() is
    `(a & m) | o` on operands made opaque by EMPTY asm statements, so that v_and_or_b32 is hipcc's own instruction.  Allowed: the exchange-K
    queue's v_accvgpr_read_b32 (covered by the ISA lint), memory / scalar / wait instructions."""
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quick_amd", "csrc")
    offenders = []
    for fn in sorted(os.listdir(root)):
        if fn.endswith("_loop.inc") or not fn.endswith((".hpp", ".hip", ".cpp")):
            continue
        text = open(os.path.join(root, fn)).read()
        for m in re.finditer(r"asm\s*(?:volatile)?\s*\(\s*((?:\"(?:[^\"\\\\]|\\\\.)*\"\s*)+)", text):
            body = "".join(re.findall(r"\"((?:[^\"\\\\]|\\\\.)*)\"", m.group(1)))
            for ins in re.split(r"\\n\\t|\\n|;", body):
                mn = ins.strip().split(" ")[0]
                if mn.startswith("v_") and not mn.startswith(("v_accvgpr_read", "v_readfirstlane", "v_readlane")):
                    offenders.append((fn, ins.strip()[:60]))
    assert not offenders, offenders[:5]


def test_product_sources_have_no_compile_time_switch_but_the_tools_one():
    """A/B experiments live as patches under tools/patches/ (tools/build_variant.sh applies them to a copy), not as switches in the product's
    sources: every preprocessor conditional under quick_amd/csrc/ names QUICK_AMD_TOOLS and nothing else (the sources use #pragma once: no
    include guards), and the build defines no other macro."""
    import re
    from quick_amd import build
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "quick_amd", "csrc")
    seen, offenders = 0, []
    for fn in sorted(os.listdir(root)):
        if not fn.endswith((".hip", ".hpp", ".cpp", ".inc")):
            continue
        for no, line in enumerate(open(os.path.join(root, fn)), 1):
            m = re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b(.*)", line)
            if m is None:
                continue
            seen += 1
            cond = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
            names = set(re.findall(r"[A-Za-z_]\w*", cond)) - {"defined"}
            if names != {"QUICK_AMD_TOOLS"}:
                offenders.append((fn, no, line.strip()[:80]))
    assert seen > 0 and not offenders, offenders[:5]
    flags = list(build.CFLAGS) + [f for extra in build.EXTRA_CFLAGS.values() for f in extra]
    assert [f for f in flags if f.startswith("-D") and f != "-DQUICK_AMD_TOOLS"] == []
    src = open(build.__file__).read()
    assert set(re.findall(r"-D\w*", src)) == {"-DQUICK_AMD_TOOLS"}, "quick_amd/build.py passes a -D other than -DQUICK_AMD_TOOLS"


def test_generated_k_loops_are_what_the_generator_writes(tmp_path):
    """quick_amd/csrc/w4a16_xw_loop.inc is checked in (the build does not run the generator): it must be byte for byte what
    tools/gen_xw_loop.py writes today -- hazard distances, counted waits and register plans are asserted inside the generator."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("gen_xw_loop", os.path.join(root, "tools", "gen_xw_loop.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    gen.OUT = str(tmp_path / "loop.inc")
    gen.main()
    assert open(gen.OUT).read() == open(os.path.join(root, "quick_amd", "csrc", "w4a16_xw_loop.inc")).read()
    names = {c.name for c in gen.CONFIGS}
    assert names == {"82", "42", "41", "21"}


def test_generated_mid_token_loops_are_what_the_generator_writes(tmp_path, monkeypatch):
    """quick_amd/csrc/w4a16_xm_loop.inc (the per-wave K loops of the r06 mid-token kernels) is checked in as well: byte for byte what
    tools/gen_xm_loop.py writes with its default switches.  The generator asserts the hazard distances itself and takes every counted
    vmcnt from a walk over the dynamic instruction stream; here: every wait that protects an x piece or a weight tile is a counted one
    (no vmcnt(0) drain inside a loop copy except where the walk says nothing is behind the piece), and the six tile shapes exist."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for k in ("XM_EXP", "XM_OUT", "XM_D", "XM_TOUCH", "XM_BARRIER", "XM_WFIRST", "XM_W_NT", "XM_JITQ", "XM_SBAR"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.syspath_prepend(os.path.join(root, "tools"))
    spec = importlib.util.spec_from_file_location("gen_xm_loop", os.path.join(root, "tools", "gen_xm_loop.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    body, info = gen.generate()
    assert body == open(os.path.join(root, "quick_amd", "csrc", "w4a16_xm_loop.inc")).read()
    assert {c.name for c in gen.CONFIGS} == {"21", "22", "23", "11", "12", "13"}
    for c in gen.CONFIGS:
        pro, first, loop, counts = gen.resolve(c, 4 * c.D + 3)
        for copy in loop:
            waits = [i.text for i in copy if i.text.startswith("s_waitcnt vmcnt")]
            assert len(waits) == 5 and all(int(w.split("(")[1].rstrip(")")) <= 63 for w in waits)
        assert 16 * c.MB * c.PR <= c.AXF and c.VEND <= 128      # accumulators below the x fragments; the 512-thread workgroup's 128 VGPRs


def _attention_table(B, nh, nkv, L):
    """The dispatch of quick_decode_rope_attention_f16 with the A/B switches unset, restated: (kernel word, heads per workgroup, gsplit, waves)."""
    group, pairs = nh // nkv, B * nkv
    if group == 8 and pairs >= 256:
        return "gqa-mfma", 8, 1, 4
    if group == 8 and pairs >= 128:
        return "gqa-mfma", 4, 2, 4
    if group == 4 and pairs >= 256:
        return "gqa-mfma", 4, 1, 4
    if group == 4 and pairs >= 128:
        return "gqa", 2, 2, 4
    if group == 2 and pairs >= 256:
        return "gqa", 2, 1, 4
    return "flash", 1, 1, (8 if B * nh <= 128 and L > 128 else 4)


def test_attention_describe_pins_the_dispatch():
    """quick_decode_rope_attention_describe is host-only and makes the launcher's own decision.  Pinned: the decoder configs at the batch
    sizes the benchmarks run, the pair boundaries 127 / 128 / 255 / 256, the flash wave boundary at cache_len 128 / 129, and the groups
    that no grouped-query kernel serves (1, 3, 16)."""
    import subprocess
    code = r"""
import json, sys
from quick_amd import kernels
print(json.dumps([kernels.attention_describe(B, nh, nkv, 128, L) for B, nh, nkv, L in json.loads(sys.argv[1])]))
"""
    from quick_amd.decoder import CONFIGS
    cases = []
    for name in ("llama2-7b", "mistral-7b", "llama2-70b", "tiny"):
        c = CONFIGS[name]
        for B in (1, 4, 16, 32, 64):
            for L in (128, 129, 4096):
                cases.append((B, c.heads, c.kv_heads, L))
    for group in (2, 4, 8):                     # pairs = B * nkv at 127 / 128 / 255 / 256
        for B, nkv in ((127, 1), (128, 1), (255, 1), (256, 1), (16, 8), (32, 8), (15, 17), (17, 15), (51, 5), (64, 4)):
            cases.append((B, group * nkv, nkv, 4096))
    for group in (1, 3, 16):                    # flash whatever the pairs
        for B, nkv in ((1, 8), (16, 8), (32, 8), (64, 8), (256, 1), (4, 2)):
            for L in (128, 129):
                cases.append((B, group * nkv, nkv, L))
    cases += [(1, 128, 8, 129), (1, 129, 1, 129), (2, 64, 64, 129), (2, 64, 64, 128), (3, 43, 43, 129), (65535, 1, 1, 4096)]
    env = {k: v for k, v in os.environ.items() if k not in ("QUICK_AMD_ATTN_MFMA", "QUICK_AMD_ATTN_WAVES")}
    r = subprocess.run([sys.executable, "-c", code, json.dumps(cases)], capture_output=True, text=True, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr
    texts = json.loads(r.stdout.strip().splitlines()[-1])
    seen = set()
    for (B, nh, nkv, L), text in zip(cases, texts):
        word, heads, gsplit, waves = _attention_table(B, nh, nkv, L)
        want = f"{word} heads={heads} gsplit={gsplit} waves={waves} set_rows={waves * 16 if word == 'flash' else 64} "
        grid = f"grid={nh if word == 'flash' else nkv * gsplit}x{B}"
        assert text.startswith(want) and text.endswith(grid), (B, nh, nkv, L, text, want, grid)
        seen.add(want)
    assert len(seen) == 7, seen                 # every branch of the table was reached (flash with 4 and with 8 waves)
    # the decoder shapes the issue's table names
    from quick_amd import kernels
    assert kernels.attention_describe(16, 64, 8, 128, 4096).startswith("gqa-mfma heads=4 gsplit=2")     # Llama-2-70B bs 16
    assert kernels.attention_describe(32, 32, 8, 128, 4096).startswith("gqa-mfma heads=4 gsplit=1")     # Mistral-7B bs 32
    assert kernels.attention_describe(1, 32, 32, 128, 4096).startswith("flash heads=1 gsplit=1 waves=8")   # Llama-2-7B bs 1
    assert kernels.attention_describe(64, 32, 32, 128, 4096).startswith("flash heads=1 gsplit=1 waves=4")  # Llama-2-7B bs 64


def test_decode_entry_points_refuse_before_launching():
    """The decode-step C entry points validate their arguments before they launch anything: these calls pass null device pointers (the
    lm_head ones a zero-byte workspace, refused last) and must come back with the documented error code."""
    lib = _lib.load()
    INVALID, WORKSPACE, UNSUPPORTED = 1, 2, 4
    buf = ctypes.create_string_buffer(128)
    # RMSNorm: hidden % 8 != 0
    for H in (4, 12, 4100, 0, -8):
        assert lib.quick_rmsnorm_f16(None, None, None, 2, H, 1e-5, None) == INVALID, H
    assert lib.quick_rmsnorm_f16(None, None, None, 0, 512, 1e-5, None) == INVALID
    # RoPE + KV append / prefill write: odd or too large head_dim, head counts, grid.y
    for D in (127, 63, 130, 256):
        assert lib.quick_rope_kv_append_f16(None, None, None, None, None, None, None, 1, 8, 2, D, 64, None) == INVALID, D
        assert lib.quick_rope_kv_write_f16(None, None, None, None, None, None, None, 1, 4, 8, 2, D, 64, None) == INVALID, D
    for nh, nkv in ((8, 3), (8, 0), (0, 2), (-8, 2)):
        assert lib.quick_rope_kv_append_f16(None, None, None, None, None, None, None, 1, nh, nkv, 128, 64, None) == INVALID, (nh, nkv)
        assert lib.quick_rope_kv_write_f16(None, None, None, None, None, None, None, 1, 4, nh, nkv, 128, 64, None) == INVALID, (nh, nkv)
    assert lib.quick_rope_kv_append_f16(None, None, None, None, None, None, None, 65536, 8, 2, 128, 64, None) == UNSUPPORTED
    assert lib.quick_rope_kv_write_f16(None, None, None, None, None, None, None, 65536, 1, 8, 2, 128, 64, None) == UNSUPPORTED
    assert lib.quick_rope_kv_write_f16(None, None, None, None, None, None, None, 256, 257, 8, 2, 128, 64, None) == UNSUPPORTED   # B * T = 65792
    assert lib.quick_rope_kv_write_f16(None, None, None, None, None, None, None, 1, 65536, 8, 2, 128, 64, None) == UNSUPPORTED
    # fused RoPE + attention (and its describe): head_dim 128 only, batch <= 65535, whole groups
    for args in ((1, 8, 2, 64, 64), (1, 8, 2, 127, 64), (65536, 8, 2, 128, 64), (1, 8, 3, 128, 64), (1, 8, 0, 128, 64), (0, 8, 2, 128, 64),
                 (1, 8, 2, 128, 0)):
        assert lib.quick_decode_rope_attention_f16(None, None, None, None, None, None, None, *args, 0.1, None) == UNSUPPORTED, args
        assert lib.quick_decode_rope_attention_describe(*args, buf, len(buf)) == UNSUPPORTED, args
    assert lib.quick_decode_rope_attention_describe(1, 8, 2, 128, 64, None, 0) == INVALID
    # the two-pass kernel: scores of the whole cache in LDS, cache_len <= 15872
    assert lib.quick_decode_attention_f16(None, None, None, None, None, 1, 8, 2, 128, 15873, 0.1, None) == UNSUPPORTED
    for args in ((1, 8, 2, 64, 64), (65536, 8, 2, 128, 64), (1, 8, 3, 128, 64), (1, 8, 0, 128, 64)):
        assert lib.quick_decode_attention_f16(None, None, None, None, None, *args, 0.1, None) == UNSUPPORTED, args
    # lm_head: batch <= 4, hidden % 512 == 0, batch * hidden <= 36864 -- refused ahead of the (zero-byte) workspace
    fake = ctypes.c_void_p(1 << 40)
    lm = lambda B, V, H, ws=0: lib.quick_lm_head_argmax_f16(fake, None, 1e-5, fake, None, None, fake, fake, ws, B, V, H, None)
    assert lib.quick_lm_head_argmax_f16(None, None, 1e-5, None, None, None, None, None, 0, 1, 1000, 4096, None) == INVALID
    for B, V, H in ((5, 1000, 512), (0, 1000, 512), (1, 1000, 4000), (2, 1000, 256), (1, 1000, 0), (4, 1000, 9728), (1, 1000, 37376),
                    (2, 1000, 18944), (3, 1000, 12800), (1, 0, 512)):
        assert lm(B, V, H) == UNSUPPORTED, (B, V, H)
    for B, H in ((4, 9216), (1, 36864), (2, 18432)):   # at the LDS limit: only the workspace is missing
        assert lm(B, 1000, H) == WORKSPACE, (B, H)
