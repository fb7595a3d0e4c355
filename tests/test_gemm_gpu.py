"""Parity of the HIP W4A16 path (through the C ABI) against the CPU oracle.  Needs an MI355X.

Tolerance: the north star asks for <= 1e-2 relative error against CPU dequantize + matmul; the HIP path
accumulates in fp32 with one final rounding, so the tests hold it to 2e-3 (only summation order differs)
and to bit-exactness wherever the result is order-independent (dequantised weights, one-hot probes,
power-of-two scaling).
"""
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import golden_files, load_golden, rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-3
SKINNY, TILED = 1, 2
SKINNY_EXACT = SKINNY | (1 << 25)     # M <= 16: per-weight fp16((w - z) * s) instead of the deferred-zero path
SKINNY_DZ = SKINNY | (1 << 26)        # M <= 16: deferred-zero path even where the planner would not pick it


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _pack_dev(iw, s, z, device):
    return [_dev(a, device) for a in oracle.pack_mi355x(iw, s, z)]


@pytest.fixture(scope="module")
def qa(device):
    import quick_amd
    from quick_amd import _lib
    _lib.load()          # fail loudly if the HIP extension is not built
    return quick_amd


# ------------------------------------------------------------------------------------------------
# golden fixtures produced by the reference's own Python
# ------------------------------------------------------------------------------------------------
GOLD = [p for p in golden_files("exact_") if "k64" not in p] + golden_files("quant_")


@pytest.mark.parametrize("kernel_id,ksplit", [(0, 0), (SKINNY_DZ, 1), (SKINNY_DZ, 2), (SKINNY_EXACT, 1), (SKINNY_EXACT, 2),
                                              (TILED, 1), (TILED, 2), (3, 1), (3, 2), (3 | (8 << 4) | (2 << 8), 1),
                                              (3 | (4 << 4) | (1 << 8), 2), (4, 0), (4 | (2 << 4), 2), (4 | (4 << 4), 1),
                                              (4 | (4 << 4) | (2 << 8), 0)])
@pytest.mark.parametrize("path", GOLD, ids=lambda p: os.path.basename(p)[:-4])
def test_golden_fixture_forward(qa, device, path, kernel_id, ksplit):
    g = load_golden(path)
    # reference-format checkpoint -> GPU -> HIP repack -> HIP GEMM
    qw, qs, qz = qa.repack_cuda_to_mi355x(_dev(g["ref_qweight"], device), _dev(g["ref_qscales"], device), _dev(g["ref_qzeros"], device))
    y = qa.gemm_forward(_dev(g["x"], device), qw, qs, qz, kernel_id=kernel_id, grid_split_k=ksplit)
    assert y.dtype == torch.float16 and tuple(y.shape) == g["ref_y"].shape
    assert rel_err(y.cpu().numpy(), g["ref_y"]) <= TOL


@pytest.mark.parametrize("path", GOLD, ids=lambda p: os.path.basename(p)[:-4])
def test_golden_dequant_bit_exact_and_repack_roundtrip(qa, device, path):
    g = load_golden(path)
    ref = [_dev(g[k], device) for k in ("ref_qweight", "ref_qscales", "ref_qzeros")]
    mi = qa.repack_cuda_to_mi355x(*ref)
    want = oracle.pack_mi355x(*oracle.unpack_cuda_order(g["ref_qweight"], g["ref_qscales"], g["ref_qzeros"]))
    for a, b in zip(mi, want):
        assert np.array_equal(a.cpu().numpy().view(np.uint8), b.view(np.uint8))
    back = qa.repack_mi355x_to_cuda(*mi)
    for a, b in zip(back, ref):
        assert torch.equal(a, b)
    wdeq = qa.dequantize_mi355x(*mi)
    assert np.array_equal(wdeq.cpu().numpy().view(np.uint16), g["ref_wdeq"].view(np.uint16))


@pytest.mark.parametrize("path", GOLD[:3], ids=lambda p: os.path.basename(p)[:-4])
def test_module_forward_from_reference_checkpoint(qa, device, path):
    g = load_golden(path)
    K, N, G = int(g["K"]), int(g["N"]), int(g["G"])
    m = qa.WQLinear_QUICK(4, G, K, N, True, "cpu")
    sd = {"qweight": torch.from_numpy(g["ref_qweight"]), "scales": torch.from_numpy(g["ref_qscales"]),
          "qzeros": torch.from_numpy(g["ref_qzeros"]), "bias": torch.linspace(-1, 1, N).half()}
    m.load_state_dict(sd)
    m = m.to(device)
    assert not m.is_prepared
    x = _dev(g["x"], device)
    y = m(x.reshape(1, *x.shape))                       # 3-D input, like hidden states
    assert m.is_prepared and tuple(y.shape) == (1, x.shape[0], N)
    want = (g["ref_y"].astype(np.float32) + sd["bias"].numpy().astype(np.float32))
    assert rel_err(y[0].cpu().numpy(), want) <= TOL
    sd2 = m.state_dict()                                # and it still saves the reference's format
    assert np.array_equal(sd2["qweight"].cpu().numpy(), g["ref_qweight"])
    assert np.array_equal(sd2["qzeros"].cpu().numpy(), g["ref_qzeros"])
    assert np.array_equal(sd2["scales"].cpu().numpy().view(np.uint16), g["ref_qscales"].view(np.uint16))


# ------------------------------------------------------------------------------------------------
# seeded synthetic sweeps against the oracle
# ------------------------------------------------------------------------------------------------
SHAPES = [  # (M, K, N, G)
    (1, 128, 128, 128), (1, 512, 256, 128), (2, 512, 256, 32), (7, 1024, 384, 64), (8, 1024, 128, 128),
    (16, 2048, 256, 128), (17, 512, 256, 128), (31, 1024, 384, 128), (33, 512, 128, 64), (64, 1024, 256, 128),
    (65, 512, 256, 128), (100, 640, 384, 32), (128, 1024, 256, 128), (129, 256, 128, 128), (200, 512, 640, 128),
    (300, 384, 256, 128), (3, 1024, 256, 1024), (40, 512, 256, 256), (2048, 256, 256, 128), (4100, 128, 128, 128),
]


TILED_MFMA32 = TILED | (1 << 13)      # r01's experimental 32x32x16 flavour of the tiled kernel: retired in r06 (INVALID_ARGUMENT, test_retired_kernel_ids)
TILED_16WAVES = TILED | (4 << 8)      # 4 x 4 waves per workgroup
TILED_WIDE = TILED | (1 << 29)        # 64 x 256 workgroup tiles (the planner's choice once they cover the 256 CUs: large M)
TILED_BIG = TILED | (1 << 27)         # 128 x 256 tiles run by four waves with 128 accumulators each (large M)
WIDE = 3                              # 32x32x16 MFMA kernel, one wave per SIMD, activations by LDS-DMA (large M)
XK = 4                                # exchange-K kernels: 64- / 128-token tiles whose K slices run on different CUs and swap partial tiles


def wide(mb, pairs):                  # explicit workgroup tile: mb * 32 tokens x pairs * 128 channels
    return WIDE | (mb << 4) | (pairs << 8)


WIDE_8WAVES = 1 << 15                 # ring kernel with eight waves per workgroup (two per SIMD), k16 steps split by parity
WIDE_NORING = 1 << 12                 # 64- / 128-token tiles on the double-buffered kernel instead of the LDS-DMA ring
WIDE_IDS = ([WIDE] + [wide(mb, pairs) for mb in (2, 4, 8) for pairs in (1, 2)] + [wide(mb, pairs) | WIDE_NORING for mb in (2, 4) for pairs in (1, 2)]
            + [wide(2, 1) | (3 << 22), wide(2, 1) | (4 << 22), wide(2, 2) | (3 << 22)]      # shorter rings
            + [wide(2, 1) | WIDE_8WAVES, wide(2, 2) | WIDE_8WAVES, wide(4, 1) | WIDE_8WAVES, wide(2, 1) | WIDE_8WAVES | (3 << 22)])


@pytest.mark.parametrize("kernel_id", [0, SKINNY_DZ, SKINNY_EXACT, TILED, TILED_16WAVES, TILED_WIDE, TILED_BIG] + WIDE_IDS)
@pytest.mark.parametrize("M,K,N,G", SHAPES)
def test_synthetic_sweep(qa, device, M, K, N, G, kernel_id):
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M * 7 + K + N + G)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    y = qa.gemm_forward(_dev(x, device), *_pack_dev(iw, s, z, device), kernel_id=kernel_id)
    assert rel_err(y.cpu().numpy(), want) <= TOL


def test_hipcc_scheduled_kernels_equal_their_forcezero_build(qa, device):
    """[r06, VERDICT r05 #2] Twice (r04's exchange stores, r05's unconditional-request chunk loop) a build computed wrong results that
    `-mllvm -amdgpu-waitcnt-forcezero` cured; both turned out to be instructions hipcc could not see inside asm statements next to the wrong neighbour
     -- found by luck of a stress tool and of the golden fixtures.  This is the systematic form: the product library against
    quick_amd/lib/libquick_amd_forcezero.so (the same sources, hipcc waiting for every counter in front of every instruction it schedules --
    `python -m quick_amd.build --forcezero`, built by __graft_entry__.build()), every hipcc-scheduled family under forced ids and what AUTO picks
    across the token range, NaN-poisoned outputs, bit for bit."""
    import ctypes
    from quick_amd import _lib, kernels as K_
    from quick_amd.build import FORCEZERO_LIB
    fz = _lib.load_other(FORCEZERO_LIB)
    prod = _lib.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.zeros(96 << 20, dtype=torch.uint8, device=device)

    def run(lib, x, packed, M, K, N, G, kid):
        y = torch.full((M, N), float("nan"), dtype=torch.float16, device=device)
        rc = lib.quick_w4a16_gemm_f16_ex(x.data_ptr(), packed[0].data_ptr(), packed[1].data_ptr(), packed[2].data_ptr(), None, y.data_ptr(),
                                         ws.data_ptr(), ws.numel(), M, K, N, G, kid, 0, stream)
        torch.cuda.synchronize()
        return rc, y

    LEAN_, XK_ = 6, 4
    cases = []
    for (K, N, G) in ((1024, 512, 128), (4096, 1024, 128), (2048, 768, 64), (8192, 1024, 128)):
        for M in (1, 3, 8, 16, 17, 33, 64, 100, 256):
            cases.append((M, K, N, G, 0))
        for kid in (SKINNY_EXACT, SKINNY_DZ, SKINNY_EXACT | (2 << 4), SKINNY_EXACT | (4 << 4), SKINNY | (4 << 4), SKINNY | (2 << 4)):
            for M in (5, 16):
                cases.append((M, K, N, G, kid))
        for M in (33, 64):
            cases.append((M, K, N, G, SKINNY | (4 << 4)))
        for kid in (TILED, TILED_16WAVES, TILED_WIDE, TILED_BIG, WIDE, wide(2, 1), wide(4, 2), wide(8, 1), wide(2, 1) | WIDE_8WAVES, XK_, XK_ | (2 << 4), XK_ | (4 << 4)):
            cases.append((200, K, N, G, kid))
        if G == 128:
            cases += [(1, K, N, G, LEAN_), (4, K, N, G, LEAN_), (16, K, N, G, LEAN_)]
    cases += [(16, 8192, 1024, 128, SKINNY | (8 << 4)), (12, 8192, 2048, 128, SKINNY | (8 << 4))]      # the eight-tile straight-line kernel
    ran = 0
    for (M, K, N, G, kid) in cases:
        x_np, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G)
        packed = _pack_dev(iw, s, z, device)
        x = _dev(x_np, device)
        rc1, y1 = run(prod, x, packed, M, K, N, G, kid)
        rc2, y2 = run(fz, x, packed, M, K, N, G, kid)
        assert rc1 == rc2, (M, K, N, G, kid, rc1, rc2)
        if rc1 != 0:
            continue          # (a forced id without a build for this shape: both libraries say so)
        ran += 1
        assert not torch.isnan(y1).any() and torch.equal(y1, y2), (M, K, N, G, kid, K_.plan_describe(M, K, N, G, kid))
    assert ran >= 100, ran
    assert not ws[:65536 + (16 << 20)].any()          # (both libraries hand the arrival counters and the exchange zone back zeroed; the fp32 slabs behind them are scratch)


def test_retired_kernel_ids(qa, device):
    """[r06] Instantiations that spilled registers left the product library (tests/test_module_cpu.py::test_no_kernel_of_the_library_spills_registers):
    r01's 32x32x16 flavour of the tiled kernel answers INVALID_ARGUMENT; a forced 256 x 256 tile of r02's hipcc-scheduled kernel and forced
    sixteen-wave skinny launches with several tiles run their nearest build (128 x 256 tiles / eight waves) -- with the right result."""
    from quick_amd import kernels as K_
    M, K, N, G = 300, 1024, 512, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=77)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    packed = _pack_dev(iw, s, z, device)
    with pytest.raises((RuntimeError, ValueError), match="retired"):
        qa.gemm_forward(_dev(x, device), *packed, kernel_id=TILED_MFMA32)
    assert K_.plan_describe(M, K, N, G, wide(8, 2)).startswith("wide tokens=128 channels=256")
    assert rel_err(qa.gemm_forward(_dev(x, device), *packed, kernel_id=wide(8, 2)).cpu().numpy(), want) <= TOL
    for ntw in (2, 4):
        kid = SKINNY_EXACT | (ntw << 4) | (4 << 8)    # sixteen waves asked for
        assert f"ntw={ntw} waves=8" in K_.plan_describe(16, K, N, G, kid), K_.plan_describe(16, K, N, G, kid)
        assert rel_err(qa.gemm_forward(_dev(x[:16], device), *packed, kernel_id=kid).cpu().numpy(), want[:16]) <= TOL


# ------------------------------------------------------------------------------------------------
# skinny kernel, M <= 16: deferred-zero vs exact arithmetic, persistent vs one-block-per-workgroup launches
# ------------------------------------------------------------------------------------------------
PERSIST_FLIP = 1 << 21                # flips the default (deferred-zero: persistent, exact: not)
ONE_WG_PER_CU = 1 << 22


@pytest.mark.parametrize("variant", [0, PERSIST_FLIP, ONE_WG_PER_CU], ids=["default", "flip", "1wg"])
@pytest.mark.parametrize("base", [SKINNY_DZ, SKINNY_EXACT], ids=["dz", "exact"])
@pytest.mark.parametrize("M,K,N,G", [(1, 1024, 8320, 128), (5, 512, 8320, 64), (16, 512, 8448, 32), (3, 1024, 8320, 256),
                                     (9, 640, 8320, 128), (16, 4096, 4224, 128), (2, 384, 8320, 96)])
def test_skinny_variants_many_channel_blocks(qa, device, M, K, N, G, base, variant):
    # N / 16 > 512 channel blocks: the persistent launches walk >= 2 blocks per workgroup
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    bias = np.linspace(-1, 1, N).astype(np.float16)
    y = qa.gemm_forward(_dev(x, device), *_pack_dev(iw, s, z, device), bias=_dev(bias, device), kernel_id=base | variant)
    assert rel_err(y.cpu().numpy(), want.astype(np.float32) + bias.astype(np.float32)) <= TOL


@pytest.mark.parametrize("M,K,N,G", [(1, 4096, 4096, 128), (8, 4096, 11008, 128), (16, 2048, 512, 64), (4, 1024, 256, 32)])
def test_deferred_zero_matches_exact_kernel(qa, device, M, K, N, G):
    """The deferred-zero path keeps w - z unrounded; the exact path (and the reference) round (w - z) * s to fp16 per
    weight.  Both must sit within TOL of the oracle, and within 1e-3 of each other."""
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=K + 3 * N + M)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    packed = _pack_dev(iw, s, z, device)
    ydz = qa.gemm_forward(_dev(x, device), *packed, kernel_id=SKINNY_DZ).cpu().numpy()
    yex = qa.gemm_forward(_dev(x, device), *packed, kernel_id=SKINNY_EXACT).cpu().numpy()
    assert rel_err(ydz, want) <= TOL and rel_err(yex, want) <= TOL
    assert rel_err(ydz, yex) <= 1e-3


@pytest.mark.parametrize("M,K,N,G", [(16, 4096, 12288, 128), (12, 8192, 8192, 128), (8, 4096, 12288, 64), (9, 4096, 12288, 32),
                                     (24, 11008, 4096, 128)])
def test_fragment_deferred_zero_matches_exact_kernel(qa, device, M, K, N, G):
    """M = 6..32 on large layers: 4 channel tiles per workgroup, x fragments straight from L2, the unit sums from an extra
    MFMA per k-step (no LDS table).  Against the same launch shape with exact per-weight dequantisation (bit 25) and the
    oracle; per-row, so that a token-dependent slip cannot hide behind the matrix maximum."""
    from quick_amd import kernels as K_
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=5 * M + K + N)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    ydz = qa.gemm_forward(_dev(x, device), *packed).cpu().numpy().astype(np.float32)
    yex = qa.gemm_forward(_dev(x, device), *packed, kernel_id=1 << 25).cpu().numpy().astype(np.float32)
    scale = np.abs(want).max()
    assert (np.abs(ydz - want).max(axis=1) <= TOL * scale).all()
    assert (np.abs(yex - want).max(axis=1) <= TOL * scale).all()
    assert rel_err(ydz, yex) <= 1e-3


def test_deferred_zero_with_activation_outliers(qa, device):
    """Massive activations (a few |x| ~ 2000 among |x| ~ 1) put 1024 * x into the fp32 accumulator before the group's
    bias term is removed; the cancellation error has to stay far below the tolerance."""
    M, K, N, G = 4, 4096, 1024, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=21)
    rng = np.random.default_rng(5)
    x = x.astype(np.float32)
    x[:, rng.integers(0, K, 6)] = rng.choice([-2048.0, 1536.0, 2047.0], size=(M, 6))
    x[2] = np.abs(x[2])                      # one all-positive row: the largest group sums
    x = x.astype(np.float16)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    packed = _pack_dev(iw, s, z, device)
    ydz = qa.gemm_forward(_dev(x, device), *packed, kernel_id=SKINNY_DZ).cpu().numpy()
    yex = qa.gemm_forward(_dev(x, device), *packed, kernel_id=SKINNY_EXACT).cpu().numpy()
    assert np.isfinite(ydz).all()
    assert rel_err(ydz, want) <= TOL and rel_err(yex, want) <= TOL


@pytest.mark.parametrize("ksplit", [2, 3, 8])
@pytest.mark.parametrize("kernel_id", [SKINNY, TILED])
def test_grid_split_k_and_bias(qa, device, kernel_id, ksplit):
    M, K, N, G = 24, 2048, 256, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=99)
    bias = np.linspace(-2, 2, N).astype(np.float16)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32) + bias.astype(np.float32)
    y = qa.gemm_forward(_dev(x, device), *_pack_dev(iw, s, z, device), bias=_dev(bias, device), kernel_id=kernel_id,
                        grid_split_k=ksplit)
    assert rel_err(y.cpu().numpy(), want) <= TOL


# ------------------------------------------------------------------------------------------------
# BASELINE.json sizes: K = N = 4096, G = 128, M in {1, 8, 64, 512}
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def full(qa, device):
    K = N = 4096
    G = 128
    x, iw, s, z = oracle.make_synthetic(512, K, N, G, seed=0)
    wdeq = oracle.dequantize(iw, s, z, G)
    return dict(K=K, N=N, G=G, x=x, wdeq=wdeq, packed=_pack_dev(iw, s, z, device))


@pytest.mark.parametrize("M", [1, 8, 64, 512])
def test_baseline_shapes_against_oracle(qa, device, full, M):
    x = full["x"][:M]
    want = oracle.gemm_fp32acc(x, full["wdeq"])
    y = qa.gemm_forward(_dev(x, device), *full["packed"])
    err = rel_err(y.cpu().numpy(), want)
    assert err <= TOL, err


@pytest.mark.parametrize("M", [1, 8, 64, 512])
def test_baseline_one_hot_rows_reproduce_dequantised_weights_bit_exactly(qa, device, full, M):
    # x = e_k  =>  y = W_deq[k, :] with nothing to round: exercises unpack order, zero point, scale, MFMA
    # operand layout and the epilogue at full size, independent of summation order.
    K = full["K"]
    ks = (np.arange(M) * 2654435761 % K).astype(np.int64)
    x = np.zeros((M, K), dtype=np.float16)
    x[np.arange(M), ks] = 1.0
    y = qa.gemm_forward(_dev(x, device), *full["packed"]).cpu().numpy()
    assert np.array_equal(y, full["wdeq"][ks])        # float compare: exact values, -0 == +0


@pytest.mark.parametrize("M", [1, 64, 512])
def test_baseline_power_of_two_scaling_is_exact_and_deterministic(qa, device, full, M):
    # fp16 subnormals are kept out of x: doubling turns some of them into normals, and the matrix core does
    # not treat the two classes alike, so y(2x) == 2 y(x) would otherwise fail by an ulp in a handful of outputs
    xs = full["x"][:M].copy()
    xs[np.abs(xs) < 2.0 ** -13] = 2.0 ** -13
    x = _dev(xs, device)
    y1 = qa.gemm_forward(x, *full["packed"])
    assert torch.equal(qa.gemm_forward(x, *full["packed"]), y1)          # run-to-run identical (no races)
    y2 = qa.gemm_forward(x * 2, *full["packed"])
    normal = y1.abs() >= 2.0 ** -13          # a subnormal fp16 output has fewer bits than its double: not comparable
    assert torch.equal(y2[normal], (y1 * 2)[normal])
    assert ((y2 - y1 * 2).abs() <= 2.0 ** -23)[~normal].all()
    assert torch.equal(qa.gemm_forward(torch.zeros_like(x), *full["packed"]), torch.zeros_like(y1))


def test_baseline_rows_are_independent_of_batch(qa, device, full):
    # the M=1 (skinny) and M=512 (tiled) kernels must agree on the same row up to summation order
    x = _dev(full["x"], device)
    y512 = qa.gemm_forward(x, *full["packed"])
    for r in (0, 255, 511):
        y1 = qa.gemm_forward(x[r:r + 1].contiguous(), *full["packed"])
        assert rel_err(y1.cpu().numpy(), y512[r:r + 1].cpu().numpy()) <= 1e-3


# ------------------------------------------------------------------------------------------------
# model shapes of the e2e configs, small M
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,N", [(4096, 12288), (4096, 11008), (11008, 4096), (14336, 4096), (4096, 1024), (8192, 1024)])
@pytest.mark.parametrize("M", [1, 16, 64])
def test_model_shapes(qa, device, K, N, M):
    if N % 128 != 0:
        pytest.skip("N not a multiple of 128")
    G = 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=K + N + M)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    y = qa.gemm_forward(_dev(x, device), *_pack_dev(iw, s, z, device))
    assert rel_err(y.cpu().numpy(), want) <= TOL


def _random_layer_and_sampled_oracle(qa, device, M, K, N, G, seed, ncols=256):
    """A layer of random bits made on the GPU (MI355X order; the numpy packer would take minutes at these sizes), x, and
    the ORACLE's result on `ncols` sampled output channels: the sampled channels are unpacked from the packed tensors with
    the oracle's closed form (oracle.unpack_mi355x_columns) and pushed through oracle.w4a16_forward on the CPU."""
    from quick_amd import packing
    g = torch.Generator(device=device).manual_seed(seed)
    qw, sc, qz = packing.random_mi355x(K, N, G, device, g)
    x = (torch.randn(M, K, device=device, generator=g) * 0.5).half()
    rng = np.random.default_rng(seed)
    cols = np.unique(np.concatenate([rng.integers(0, N, ncols), [0, 15, 16, 127, 128, N - 129, N - 128, N - 1]]))
    iw, s, z = oracle.unpack_mi355x_columns(qw.cpu().numpy(), sc.cpu().numpy(), qz.cpu().numpy(), cols)
    want = oracle.w4a16_forward(x.cpu().numpy(), iw, s, z, G).astype(np.float32)
    return (qw, sc, qz), x, cols, want


# every GEMM shape of the three e2e configs (fused qkv and fused gate_up widths included) at the decode
# batch sizes of BASELINE.json (1, 16, 64) -- Mistral-7B bs=64: (4096, 6144), (4096, 28672), (14336, 4096), (4096, 4096)
E2E_SHAPES = [(4096, 4096), (4096, 12288), (4096, 22016), (11008, 4096),                       # Llama-2-7B
              (4096, 6144), (4096, 14336), (4096, 28672), (14336, 4096),                        # Mistral-7B
              (8192, 8192), (8192, 10240), (8192, 28672), (8192, 57344), (28672, 8192)]        # Llama-2-70B


@pytest.mark.parametrize("K,N", E2E_SHAPES)
@pytest.mark.parametrize("M", [1, 16, 64])
def test_e2e_layer_shapes_sampled_channels_against_oracle(qa, device, K, N, M):
    packed, x, cols, want = _random_layer_and_sampled_oracle(qa, device, M, K, N, 128, seed=K + N + M)
    y = qa.gemm_forward(x, *packed)
    assert tuple(y.shape) == (M, N)
    got = y[:, torch.from_numpy(cols).to(device)].float().cpu().numpy()
    assert float(np.abs(got - want).max()) <= TOL * float(np.abs(want).max())


@pytest.mark.parametrize("K,N", E2E_SHAPES[:8] + [(8192, 8192), (8192, 10240)])
@pytest.mark.parametrize("M", [100, 192, 320, 512, 1000])
def test_mid_token_counts_on_layer_shapes_against_oracle(qa, device, K, N, M):
    """96..1024 tokens on the model layers: the four-wave kernels' territory since r04 (whatever the planner picks is checked; the test
    also insists that the family it was written for still runs on at least the bench shape)."""
    from quick_amd import kernels as K_
    packed, x, cols, want = _random_layer_and_sampled_oracle(qa, device, M, K, N, 128, seed=K + N + M, ncols=64)
    y = qa.gemm_forward(x, *packed)
    got = y[:, torch.from_numpy(cols).to(device)].float().cpu().numpy()
    assert float(np.abs(got - want).max()) <= TOL * float(np.abs(want).max())
    assert torch.equal(y, qa.gemm_forward(x, *packed))                     # bit-identical run to run, exchange or not
    if (M, K, N) == (512, 4096, 4096):
        assert K_.plan_describe(M, K, N, 128, 0).startswith("xw ")


@pytest.mark.parametrize("kernel_id", [0, TILED, WIDE, wide(4, 2), wide(8, 2)], ids=["auto", "tiled", "wide", "wide128x256", "wide256x256"])
@pytest.mark.parametrize("M,K,N", [(128, 4096, 12288), (2048, 4096, 12288), (8192, 4096, 6144), (2048, 8192, 10240), (1024, 11008, 4096)])
def test_prefill_shapes_sampled_channels_against_oracle(qa, device, M, K, N, kernel_id):
    """Prefill token counts (bs x 128) on real layer shapes, every large-M kernel family."""
    packed, x, cols, want = _random_layer_and_sampled_oracle(qa, device, M, K, N, 128, seed=M + K + N, ncols=64)
    y = qa.gemm_forward(x, *packed, kernel_id=kernel_id)
    got = y[:, torch.from_numpy(cols).to(device)].float().cpu().numpy()
    assert float(np.abs(got - want).max()) <= TOL * float(np.abs(want).max())


# ------------------------------------------------------------------------------------------------
# BASELINE size pinned by the reference itself: tests/golden/pin_k4096n4096g128.npz (seed + hashes + sampled outputs)
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pin(device):
    from conftest import exact_layer
    g = load_golden(golden_files("pin_")[0])
    iw, s, z = exact_layer(int(g["K"]), int(g["N"]), int(g["G"]), int(g["seed"]))
    return g, iw, s, z


@pytest.mark.parametrize("kernel_id", [0, SKINNY_EXACT, SKINNY_DZ, TILED, WIDE, 4 | (2 << 4), 4 | (4 << 4)],
                         ids=["auto", "skinny-exact", "skinny-dz", "tiled", "wide", "xk64", "xk128"])
def test_baseline_size_reference_pin(qa, device, pin, kernel_id):
    """K = N = 4096, g = 128: the HIP result against sampled outputs of the REFERENCE's CPU path on the same layer."""
    g, iw, s, z = pin
    y = qa.gemm_forward(_dev(g["x"], device), *_pack_dev(iw, s, z, device), kernel_id=kernel_id).cpu().numpy().astype(np.float32)
    ref = g["y_ref"].astype(np.float32)
    assert float(np.abs(y[g["y_rows"], g["y_cols"]] - ref).max()) <= TOL * float(np.abs(ref).max())
    assert float(np.abs(np.abs(y).sum(0) - g["col_abs_sum"]).max()) <= TOL * float(g["col_abs_sum"].max())


@pytest.mark.parametrize("M", [64, 512])
def test_baseline_size_reference_pin_at_bench_token_counts(qa, device, pin, M):
    """The bench's token counts on the pinned layer: rows are the fixture's 16 rows repeated, so every row has a
    reference-made value (rows of a GEMM are independent; test_baseline_rows_are_independent_of_batch)."""
    g, iw, s, z = pin
    x = np.tile(g["x"], (M // g["x"].shape[0], 1))
    packed = _pack_dev(iw, s, z, device)
    ref = g["y_ref"].astype(np.float32)
    for kernel_id in (0, XK | (2 << 4), XK | (4 << 4)):     # the planner's kernel, and the exchange-K tiles (K slices on different CUs)
        y = qa.gemm_forward(_dev(x, device), *packed, kernel_id=kernel_id).cpu().numpy().astype(np.float32)
        for rep in (0, M // 16 - 1):
            assert float(np.abs(y[g["y_rows"] + 16 * rep, g["y_cols"]] - ref).max()) <= TOL * float(np.abs(ref).max())
        assert float(np.abs(np.abs(y).sum(0) - g["col_abs_sum"] * (M // 16)).max()) <= TOL * float(g["col_abs_sum"].max()) * (M // 16)


# ------------------------------------------------------------------------------------------------
# operator interface and error behaviour (csrc/gemm_cuda_quick.cu:1456-1517)
# ------------------------------------------------------------------------------------------------
def test_split_k_reduction_is_stable_across_many_launches(qa, device):
    """In-kernel split-K (last arriver reduces): the arrival counters must come back to zero after every launch and the
    result must not depend on which slice arrives last -- hammer it, alternating shapes that share the workspace."""
    cases = []
    # (4, 4096, 2048): 128 tiles -- more arrival counters than the other cases; a counter region sized by the tile count
    # once put them on top of an earlier launch's partial sums
    for M, K, N, G in ((64, 4096, 1024, 128), (40, 2048, 512, 128), (8, 4096, 256, 128), (130, 2048, 256, 64), (4, 4096, 2048, 128),
                       (16, 8192, 4096, 128)):
        x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + N)
        cases.append((_dev(x, device), _pack_dev(iw, s, z, device), oracle.w4a16_forward(x, iw, s, z, G)))
    first = [None] * len(cases)
    for rep in range(25):
        for i, (xd, packed, want) in enumerate(cases):
            y = qa.gemm_forward(xd, *packed)
            assert rel_err(y.cpu().numpy(), want) <= TOL, rep
            if first[i] is None:
                first[i] = y
            assert torch.equal(y, first[i]), rep      # slabs are summed in slice order: bit-identical every launch


def test_reference_operator_signature_and_errors(qa, device):
    import quick_kernels
    M, K, N, G = 5, 256, 128, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=3)
    packed = [_dev(a, device) for a in oracle.pack_cuda_order(iw, s, z)]       # the REFERENCE's order, as its module holds it
    xd = _dev(x, device)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    y8 = quick_kernels.gemm_forward_cuda_quick(xd, *packed, 8)
    y1 = quick_kernels.gemm_forward_cuda_quick(xd, *packed, 1)
    assert tuple(y8.shape) == (M, N) and tuple(y1.shape) == (1, M, N)        # gemm_cuda_quick.cu:1515-1516
    assert rel_err(y8.cpu().numpy(), want) <= TOL and torch.equal(y1[0], y8)
    with pytest.raises(RuntimeError):                                          # data_ptr<at::Half>() on a float tensor
        quick_kernels.gemm_forward_cuda_quick(xd.float(), *packed, 8)
    with pytest.raises(RuntimeError):
        quick_kernels.gemm_forward_cuda_quick(xd, packed[0].float(), packed[1], packed[2], 8)
    bad_n = [torch.zeros(K // 4, 96 // 2, dtype=torch.int32, device=device), torch.zeros(K // G, 192, dtype=torch.float16, device=device),
             torch.zeros(K // G, 24, dtype=torch.int32, device=device)]
    with pytest.raises(ValueError, match="cta_N"):                             # std::invalid_argument, line 1479
        quick_kernels.gemm_forward_cuda_quick(xd, *bad_n, 8)
    bad_g = [packed[0], torch.zeros(K // 16, 2 * N, dtype=torch.float16, device=device), torch.zeros(K // 16, N // 4, dtype=torch.int32, device=device)]
    with pytest.raises(ValueError, match="multiple of 32"):                    # line 1483
        quick_kernels.gemm_forward_cuda_quick(xd, *bad_g, 8)
    mi = _pack_dev(iw, s, z, device)
    assert tuple(qa.gemm_forward(xd[:0], *mi).shape) == (0, N)                # empty batch
    with pytest.raises(ValueError, match="out must be"):                      # raw pointers are shape-checked on the way in
        qa.gemm_forward(xd, *mi, out=torch.empty(M, N + 128, dtype=torch.float16, device=device))
    with pytest.raises(RuntimeError, match="float16"):
        qa.gemm_forward(xd, *mi, bias=torch.zeros(N, device=device))


@pytest.mark.parametrize("path", GOLD, ids=lambda p: os.path.basename(p)[:-4])
def test_function_level_drop_in_takes_reference_order_tensors(qa, device, path):
    """What the reference's unchanged WQLinear_QUICK.forward does (quick/awq/modules/linear/quick.py:158-166): hand its own
    buffers -- checkpoint order, quick.py:88-150 -- to quick_kernels.gemm_forward_cuda_quick.  The fixtures' ref_q* tensors
    ARE those buffers (made by the reference packer), ref_y the reference CPU path's output for them."""
    import quick_kernels
    from quick_amd import kernels as K_
    g = load_golden(path)
    ref = [_dev(g[k], device) for k in ("ref_qweight", "ref_qscales", "ref_qzeros")]
    x = _dev(g["x"], device)
    y = quick_kernels.gemm_forward_cuda_quick(x, *ref, 8)
    assert tuple(y.shape) == g["ref_y"].shape and rel_err(y.cpu().numpy(), g["ref_y"]) <= TOL
    y1 = quick_kernels.gemm_forward_cuda_quick(x, *ref, 1)                    # split_k == 1: [1, M, N]
    assert tuple(y1.shape) == (1,) + g["ref_y"].shape and torch.equal(y1[0], y)
    n_cached = len(K_._REPACK_CACHE)
    assert torch.equal(quick_kernels.gemm_forward_cuda_quick(x, *ref, 8), y) and len(K_._REPACK_CACHE) == n_cached   # cache hit
    # an in-place rewrite of the buffers (load_state_dict / copy_) must invalidate the cached MI355X-order copy
    other = oracle.make_synthetic(1, int(g["K"]), int(g["N"]), int(g["G"]), seed=77)[1:]
    for t, a in zip(ref, oracle.pack_cuda_order(*other)):
        t.copy_(_dev(a, device))
    y2 = quick_kernels.gemm_forward_cuda_quick(x, *ref, 8)
    assert rel_err(y2.cpu().numpy(), oracle.w4a16_forward(g["x"], *other, int(g["G"]))) <= TOL
    # ... and the entry dies with the tensors
    key = tuple(t.data_ptr() for t in ref)
    assert key in K_._REPACK_CACHE
    del ref, t
    import gc
    gc.collect()
    assert key not in K_._REPACK_CACHE


def test_function_level_drop_in_cache_hits_from_other_streams(qa, device):
    """The cached MI355X-order copy is made on one stream and hit from others: the first eager hit from another stream waits
    for the repack once, on the host, and later hits from that stream neither wait nor record anything; a hit inside a graph capture on a
    third stream must be capturable and replay to the same numbers."""
    import quick_kernels
    from quick_amd import kernels as K_
    M, K, N, G = 5, 1024, 512, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=41)
    ref = [_dev(a, device) for a in oracle.pack_cuda_order(iw, s, z)]
    xd = _dev(x, device)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    maker, other, third = (torch.cuda.Stream(device) for _ in range(3))
    with torch.cuda.stream(maker):
        y0 = quick_kernels.gemm_forward_cuda_quick(xd, *ref, 8)
    ent = K_._REPACK_CACHE[tuple(t.data_ptr() for t in ref)]
    assert ent.stream == maker and not ent.done
    with torch.cuda.stream(other):
        y1 = quick_kernels.gemm_forward_cuda_quick(xd, *ref, 8)
        assert ent.done and (other.stream_id, other.cuda_stream) in ent.seen   # (torch's id AND the raw handle: handles are recycled)
        seen = set(ent.seen)
        y2 = quick_kernels.gemm_forward_cuda_quick(xd, *ref, 8)
        assert ent.seen == seen
    torch.cuda.synchronize()
    for y in (y0, y1, y2):
        assert rel_err(y.cpu().numpy(), want) <= TOL
    assert torch.equal(y0, y1) and torch.equal(y1, y2)
    g = torch.cuda.CUDAGraph()
    static_x = xd.clone()
    with torch.cuda.stream(third):
        with torch.cuda.graph(g, stream=third):
            static_y = quick_kernels.gemm_forward_cuda_quick(static_x, *ref, 8)
    assert (third.stream_id, third.cuda_stream) in ent.seen     # the allocator knows about the capturing stream too
    static_x.copy_(xd * 2)
    g.replay()
    torch.cuda.synchronize()
    assert rel_err(static_y.cpu().numpy(), want.astype(np.float32) * 2) <= TOL


@pytest.mark.parametrize("M,K,N,G", [(1, 96, 128, 32), (7, 320, 256, 64), (40, 192, 128, 96), (130, 1056, 384, 32), (16, 4160, 512, 64)])
def test_in_features_not_a_multiple_of_128(qa, device, M, K, N, G):
    """Shapes the reference accepts (in_features % 32 == 0) and the MI355X weight order does not tile: the function-level
    drop-in and the module both run them on a zero-padded copy (kernels.padded_in_features) -- against the oracle."""
    import quick_kernels
    from quick_amd import WQLinear_QUICK
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    ref = [_dev(a, device) for a in oracle.pack_cuda_order(iw, s, z)]
    y = quick_kernels.gemm_forward_cuda_quick(_dev(x, device), *ref, 8)
    assert tuple(y.shape) == (M, N) and rel_err(y.cpu().numpy(), want) <= TOL
    m = WQLinear_QUICK(4, G, K, N, True, device)
    bias = torch.linspace(-1, 1, N, device=device).half()
    m.load_state_dict({"qweight": ref[0], "scales": ref[1], "qzeros": ref[2], "bias": bias})
    ym = m(_dev(x, device))
    assert rel_err(ym.cpu().numpy(), want.astype(np.float32) + bias.cpu().numpy().astype(np.float32)) <= TOL
    sd = m.state_dict()                                                 # still the reference's bits
    assert all(torch.equal(sd[k], r) for k, r in zip(("qweight", "scales", "qzeros"), ref))
    # the HIP repack kernel's padded flavour writes the bits of the torch packer on the padded logical tensors
    from quick_amd import kernels as K_
    hip = K_._padded_mi355x(*ref)
    cpu = K_._padded_mi355x(*[t.cpu() for t in ref])
    assert torch.equal(hip[0].cpu(), cpu[0]) and torch.equal(hip[1].cpu(), cpu[1])
    # ... and the compiled extension takes the same path
    from quick_amd.build_ext import build_quick_kernels_ext
    ye = build_quick_kernels_ext().gemm_forward_cuda_quick(_dev(x, device), *ref, 8)
    assert torch.equal(ye, y)


def test_compiled_quick_kernels_extension(qa, device):
    """The pybind11 / torch-extension face of the same boundary (quick_amd/csrc/quick_kernels_ext.cpp, the shape of the
    reference's csrc/pybind.cpp): built in-tree by torch.utils.cpp_extension, called with reference-order tensors."""
    from quick_amd.build_ext import build_quick_kernels_ext
    ext = build_quick_kernels_ext()
    for path in GOLD[:4]:
        g = load_golden(path)
        ref = [_dev(g[k], device) for k in ("ref_qweight", "ref_qscales", "ref_qzeros")]
        x = _dev(g["x"], device)
        y = ext.gemm_forward_cuda_quick(x, *ref, 8)
        assert tuple(y.shape) == g["ref_y"].shape and rel_err(y.cpu().numpy(), g["ref_y"]) <= TOL
        y1 = ext.gemm_forward_cuda_quick(x, *ref, 1)
        assert tuple(y1.shape) == (1,) + g["ref_y"].shape and torch.equal(y1[0], y)
        other = oracle.make_synthetic(1, int(g["K"]), int(g["N"]), int(g["G"]), seed=78)[1:]     # in-place rewrite -> repacked again
        for t, a in zip(ref, oracle.pack_cuda_order(*other)):
            t.copy_(_dev(a, device))
        y2 = ext.gemm_forward_cuda_quick(x, *ref, 8)
        assert rel_err(y2.cpu().numpy(), oracle.w4a16_forward(g["x"], *other, int(g["G"]))) <= TOL
    K, G = 256, 128
    bad_n = [torch.zeros(K // 4, 96 // 2, dtype=torch.int32, device=device), torch.zeros(K // G, 192, dtype=torch.float16, device=device),
             torch.zeros(K // G, 24, dtype=torch.int32, device=device)]
    xk = torch.zeros(3, K, dtype=torch.float16, device=device)
    with pytest.raises(ValueError, match="cta_N"):                             # std::invalid_argument, gemm_cuda_quick.cu:1479
        ext.gemm_forward_cuda_quick(xk, *bad_n, 8)
    with pytest.raises(RuntimeError):                                          # data_ptr<at::Half>() on a float tensor
        ext.gemm_forward_cuda_quick(xk.float(), *bad_n, 8)


def test_function_level_drop_in_at_baseline_size(qa, device, pin):
    import quick_kernels
    g, iw, s, z = pin
    ref = [_dev(a, device) for a in oracle.pack_cuda_order(iw, s, z)]
    y = quick_kernels.gemm_forward_cuda_quick(_dev(g["x"], device), *ref, 8).cpu().numpy().astype(np.float32)
    r = g["y_ref"].astype(np.float32)
    assert float(np.abs(y[g["y_rows"], g["y_cols"]] - r).max()) <= TOL * float(np.abs(r).max())


def test_fused_qkv_with_unequal_widths_runs_through_the_gemm(qa, device):
    """GQA: q 4096 / k 1024 / v 1024 (the reference's fuse_qkv_quick raises here, quick/awq/utils/fused_utils.py:138-142):
    three reference-format layers -> fuse_qkv_quick -> forward == the oracle on the concatenated layer."""
    K, G = 4096, 128
    mods, logical = [], []
    for i, N in enumerate((4096, 1024, 1024)):
        x, iw, s, z = oracle.make_synthetic(3, K, N, G, seed=500 + i)
        m = qa.WQLinear_QUICK(4, G, K, N, False, "cpu")
        m.load_state_dict({k: torch.from_numpy(v) for k, v in zip(("qweight", "scales", "qzeros"), oracle.pack_cuda_order(iw, s, z))})
        mods.append(m.to(device))
        logical.append((iw, s, z))
    mods[1].prepare()                                    # a mix of prepared and reference-order inputs
    fused = qa.fuse_qkv_quick(None, *mods)
    assert fused.out_features == 6144
    x = oracle.make_synthetic(64, K, 128, G, seed=9)[0]
    y = fused(_dev(x, device))
    want = oracle.w4a16_forward(x, *[np.concatenate([l[i] for l in logical], axis=1) for i in range(3)], G)
    assert fused.is_prepared and rel_err(y.cpu().numpy(), want) <= TOL
    for m, l, lo in zip(mods, logical, (0, 4096, 5120)):          # and each part equals its own layer (other K split: not bitwise)
        assert rel_err(m(_dev(x, device)).cpu().numpy(), y[:, lo:lo + l[0].shape[1]].cpu().numpy()) <= 1e-3


def test_first_forward_under_inference_mode(qa, device):
    """The reference runs every forward under torch.inference_mode() (quick/awq/modules/fused/model.py:76): the lazy
    prepare() of the first forward creates inference tensors."""
    g = load_golden(GOLD[0])
    m = qa.WQLinear_QUICK(4, int(g["G"]), int(g["K"]), int(g["N"]), False, "cpu")
    m.load_state_dict({"qweight": torch.from_numpy(g["ref_qweight"]), "scales": torch.from_numpy(g["ref_qscales"]),
                       "qzeros": torch.from_numpy(g["ref_qzeros"])})
    m = m.to(device)
    with torch.inference_mode():
        y = m(_dev(g["x"], device))
        y_again = m(_dev(g["x"], device))
    assert m.is_prepared and torch.equal(y, y_again) and rel_err(y.cpu().numpy(), g["ref_y"]) <= TOL
    assert np.array_equal(m.state_dict()["qweight"].cpu().numpy(), g["ref_qweight"])


def test_quantize_linear_end_to_end(qa, device):
    """nn.Linear -> round-to-nearest W4 -> WQLinear_QUICK -> HIP GEMM, against the fake-quantised weight in fp32
    (the `_apply_quant` hook, quick/awq/quantize/quantizer.py:148-174)."""
    from quick_amd import pseudo_quantize_tensor, quantize_linear
    torch.manual_seed(11)
    lin = torch.nn.Linear(1024, 512, bias=True)
    x = torch.randn(7, 1024).half()
    wq = pseudo_quantize_tensor(lin.weight.data.half(), 4, 128)
    want = x.float() @ wq.float().t() + lin.bias.data.half().float()
    for dev_first in (False, True):       # quantise on the CPU then move, or quantise on the GPU
        layer = quantize_linear(lin.to(device) if dev_first else lin.cpu(), 4, 128).to(device)
        y = layer(x.to(device))
        assert rel_err(y.cpu().numpy(), want.numpy()) <= TOL


def test_runs_on_current_stream_and_is_graph_capturable(qa, device):
    M, K, N, G = 4, 512, 256, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=8)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    want = oracle.w4a16_forward(x, iw, s, z, G)
    side = torch.cuda.Stream(device)
    with torch.cuda.stream(side):
        y = qa.gemm_forward(xd, *packed)
    side.synchronize()
    assert rel_err(y.cpu().numpy(), want) <= TOL
    g = torch.cuda.CUDAGraph()
    static_x = xd.clone()
    with torch.cuda.graph(g):
        static_y = qa.gemm_forward(static_x, *packed)
    static_x.copy_(xd * 2)
    g.replay()
    torch.cuda.synchronize()
    assert rel_err(static_y.cpu().numpy(), want.astype(np.float32) * 2) <= TOL


def test_synthetic_decoder_graph_replay_matches_eager(qa, device):
    """The e2e harness (quick_amd/decoder.py): a captured decode step must leave the same KV cache as eager steps."""
    from quick_amd.decoder import CONFIGS, SyntheticDecoder, run_generation
    for fused in (False, True):
        caches = []
        for use_graph in (False, True):
            torch.manual_seed(0)
            model = SyntheticDecoder(CONFIGS["tiny"], batch=3, max_len=48, device=device, seed=1)
            prefill, steps = run_generation(model, ctx=16, n_generate=12, use_graph=use_graph, fused=fused)
            assert prefill > 0 and len(steps) == (11 if use_graph else 12) and all(t > 0 for t in steps)
            caches.append(model.layers[0]["k"][:, :, :28].clone())    # the KV cache written by the 12 steps
        assert torch.equal(caches[0], caches[1])


def test_decode_glue_kernels_against_torch(qa, device):
    """Each HIP glue kernel / GEMM fusion on its own against the torch expression it replaces."""
    import torch.nn.functional as F
    from quick_amd import kernels as K_
    from quick_amd.decoder import _rms_norm, _rope
    torch.manual_seed(0)
    B, H, nh, nkv, D, L, I = 3, 512, 4, 2, 128, 40, 1024
    x = torch.randn(B, H, device=device).half()
    w = (torch.rand(H, device=device) + 0.5).half()
    torch.testing.assert_close(K_.rmsnorm(x, w), _rms_norm(x, w), rtol=2e-3, atol=2e-3)
    gu = torch.randn(B, 2 * I, device=device).half()
    g5 = gu.view(B, I // 8, 2, 8)
    torch.testing.assert_close(K_.silu_mul(gu), (F.silu(g5[:, :, 0]) * g5[:, :, 1]).reshape(B, I), rtol=2e-3, atol=1e-3)
    # RoPE + KV append + attention, split and fused launches, against torch
    ang = torch.outer(torch.arange(L, device=device).float(), 1.0 / (10000 ** (torch.arange(0, D, 2, device=device).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    qkv = torch.randn(B, (nh + 2 * nkv) * D, device=device).half()
    kc0, vc0 = torch.randn(B, nkv, L, D, device=device).half(), torch.randn(B, nkv, L, D, device=device).half()
    p = 17
    pos = torch.full((1,), p, dtype=torch.int64, device=device)
    q, k, v = qkv.split((nh * D, nkv * D, nkv * D), dim=-1)
    qr = _rope(q.view(B, 1, nh, D).transpose(1, 2), cos[p:p + 1], sin[p:p + 1])
    kr = _rope(k.view(B, 1, nkv, D).transpose(1, 2), cos[p:p + 1], sin[p:p + 1])
    kc_ref, vc_ref = kc0.clone(), vc0.clone()
    kc_ref[:, :, p] = kr[:, :, 0]
    vc_ref[:, :, p] = v.view(B, nkv, D)
    ref = F.scaled_dot_product_attention(qr.float(), kc_ref[:, :, :p + 1].float(), vc_ref[:, :, :p + 1].float(), enable_gqa=True)
    ref = ref.transpose(1, 2).reshape(B, nh * D)
    kc1, vc1 = kc0.clone(), vc0.clone()
    qo = torch.empty(B, nh, D, dtype=torch.float16, device=device)
    K_.rope_kv_append(qkv, cos, sin, pos, qo, kc1, vc1, nh, nkv, D)
    close = lambda a, b: torch.testing.assert_close(a, b, rtol=2e-3, atol=2e-3)
    close(qo, qr[:, :, 0]); close(kc1, kc_ref); close(vc1, vc_ref)
    o1 = K_.decode_attention(qo, kc1, vc1, pos, torch.empty(B, nh * D, dtype=torch.float16, device=device), nh, nkv, D)
    kc2, vc2 = kc0.clone(), vc0.clone()
    o2 = K_.rope_attention(qkv, cos, sin, pos, kc2, vc2, torch.empty(B, nh * D, dtype=torch.float16, device=device), nh, nkv, D)
    close(kc2, kc_ref); close(vc2, vc_ref)
    for o in (o1, o2):
        assert (o.float() - ref).abs().max() <= 2e-3 * ref.abs().max() + 1e-3
    # GEMM fusions: RMSNorm prologue, residual and SiLU*mul epilogues
    for M in (1, 5, 40):
        Kd, N, G = 512, 512, 128
        xs, iw, s, z = oracle.make_synthetic(M, Kd, N, G, seed=M)
        packed = _pack_dev(iw, s, z, device)
        xd, lnw = _dev(xs, device), (torch.rand(Kd, device=device) + 0.5).half()
        res = torch.randn(M, N, device=device).half()
        y = qa.gemm_forward(xd, *packed)
        y_res = qa.gemm_forward(xd, *packed, residual=res)
        assert (y_res.float() - (y.float() + res.float())).abs().max() <= 2e-2
        y_act = qa.gemm_forward(xd, *packed, silu_mul=True)
        close(y_act, K_.silu_mul(y))
        assert K_.can_fuse_rmsnorm(M, Kd, N, G) == (M != 5)   # deferred-zero launches carry the norm: table (M = 1), fragments (M = 40)
        if M != 5:
            y_ln = qa.gemm_forward(xd, *packed, rmsnorm_weight=lnw)
            y_two = qa.gemm_forward(K_.rmsnorm(xd, lnw), *packed)
            assert rel_err(y_ln.cpu().numpy(), y_two.cpu().numpy()) <= TOL
        else:
            with pytest.raises(NotImplementedError):
                qa.gemm_forward(xd, *packed, rmsnorm_weight=lnw)


@pytest.mark.parametrize("M,K,N,G", [(1, 4096, 12288, 128), (1, 4096, 4096, 128), (8, 4096, 22016, 128), (16, 1024, 12288, 64),
                                     (3, 11008, 12288, 128), (16, 4096, 12288, 128), (8, 4096, 12288, 128), (24, 4096, 8192, 128),
                                     (16, 8192, 10240, 256)])
def test_rmsnorm_prologue_matches_two_launches(qa, device, M, K, N, G):
    """gemm(rmsnorm(x) * w) in one launch.  Table flavour (x in LDS): the prologue reproduces quick_rmsnorm_f16's rounding
    points, the only difference to the two-launch result is the summation order of the squares.  Fragment and lean flavours:
    the same rounding points, the squares summed in a pass in front of the K loop."""
    from quick_amd import kernels as K_
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device) * 3
    lnw = (torch.rand(K, device=device) + 0.5).half()
    res = torch.randn(M, N, device=device).half()
    # (17..64 tokens [r06]: AUTO's pick is a mid-token kernel, which has no prologue -- can_fuse says "not worth fusing" and the decode loop norms in
    # its own launch; a caller that asks for the prologue anyway is served by the fragment kernel, checked here)
    assert K_.can_fuse_rmsnorm(M, K, N, G) or (16 < M <= 128 and K_.plan_describe(M, K, N, G).startswith("xm"))
    y1 = qa.gemm_forward(xd, *packed, rmsnorm_weight=lnw, rmsnorm_eps=1e-5, residual=res)
    y2 = qa.gemm_forward(K_.rmsnorm(xd, lnw, 1e-5), *packed, residual=res)
    assert rel_err(y1.cpu().numpy(), y2.cpu().numpy()) <= 1e-3
    # and against torch's RMSNorm + the oracle GEMM
    xn = (xd.float() * torch.rsqrt(xd.float().pow(2).mean(-1, keepdim=True) + 1e-5)).half() * lnw
    want = oracle.w4a16_forward(xn.cpu().numpy(), iw, s, z, G).astype(np.float32) + res.cpu().numpy().astype(np.float32)
    assert rel_err(y1.cpu().numpy(), want) <= TOL


@pytest.mark.parametrize("B,nh,nkv", [(2, 8, 8), (3, 8, 2), (32, 32, 32), (32, 32, 8), (64, 16, 8), (64, 64, 8), (16, 64, 8), (24, 32, 8)],
                         ids=["mha-small", "gqa-per-head", "mha-1024-workgroups", "gqa4-shared", "gqa2-shared", "gqa8-shared", "gqa8-two-workgroups", "gqa4-two-workgroups"])
@pytest.mark.parametrize("p", [0, 1, 5, 127, 128, 255, 256, 300, 319])
def test_rope_attention_kernels_against_torch(qa, device, B, nh, nkv, p):
    """RoPE + KV append + single-query attention in one launch: the single-pass (online softmax) kernel with a workgroup
    per query head, and the grouped-query kernels that serve all query heads of a KV head from one sweep, at context
    lengths around the 128-row batch size."""
    import torch.nn.functional as F
    from quick_amd import kernels as K_
    from quick_amd.decoder import _rope
    torch.manual_seed(p + B)
    D, L = 128, 320
    ang = torch.outer(torch.arange(L, device=device).float(), 1.0 / (10000 ** (torch.arange(0, D, 2, device=device).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    qkv = torch.randn(B, (nh + 2 * nkv) * D, device=device).half()
    kc, vc = torch.randn(B, nkv, L, D, device=device).half(), torch.randn(B, nkv, L, D, device=device).half()
    kc[:, :, p:], vc[:, :, p:] = float("nan"), float("nan")     # rows >= p are unwritten in a real cache (torch.empty): they must not leak
    pos = torch.full((1,), p, dtype=torch.int64, device=device)
    q, k, v = qkv.split((nh * D, nkv * D, nkv * D), dim=-1)
    qr = _rope(q.view(B, 1, nh, D).transpose(1, 2), cos[p:p + 1], sin[p:p + 1])
    kr = _rope(k.view(B, 1, nkv, D).transpose(1, 2), cos[p:p + 1], sin[p:p + 1])
    kc_ref, vc_ref = kc.clone(), vc.clone()
    kc_ref[:, :, p] = kr[:, :, 0]
    vc_ref[:, :, p] = v.view(B, nkv, D)
    ref = F.scaled_dot_product_attention(qr.float(), kc_ref[:, :, :p + 1].float(), vc_ref[:, :, :p + 1].float(), enable_gqa=True)
    ref = ref.transpose(1, 2).reshape(B, nh * D)
    o = K_.rope_attention(qkv, cos, sin, pos, kc, vc, torch.empty(B, nh * D, dtype=torch.float16, device=device), nh, nkv, D)
    torch.testing.assert_close(kc[:, :, :p + 1], kc_ref[:, :, :p + 1], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(vc[:, :, :p + 1], vc_ref[:, :, :p + 1], rtol=0, atol=0)
    assert bool(torch.isfinite(o).all()) and (o.float() - ref).abs().max() <= 2e-3 * ref.abs().max() + 1e-3


def test_prefill_rope_kv_write_against_torch(qa, device):
    """Prefill RoPE + cache write in one launch (T tokens per sequence from position *pos0) against the torch ops."""
    from quick_amd import kernels as K_
    from quick_amd.decoder import _rope
    torch.manual_seed(2)
    B, T, nh, nkv, D, L, p0 = 3, 37, 8, 2, 128, 96, 5
    ang = torch.outer(torch.arange(L, device=device).float(), 1.0 / (10000 ** (torch.arange(0, D, 2, device=device).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, device=device).half()
    kc = torch.zeros(B, nkv, L, D, dtype=torch.float16, device=device)
    vc = torch.zeros_like(kc)
    q_out = torch.empty(B, nh, T, D, dtype=torch.float16, device=device)
    K_.rope_kv_write(qkv, cos, sin, torch.full((1,), p0, dtype=torch.int64, device=device), q_out, kc, vc, T, nh, nkv, D)
    q, k, v = qkv.view(B, T, -1).split((nh * D, nkv * D, nkv * D), dim=-1)
    qr = _rope(q.view(B, T, nh, D).transpose(1, 2), cos[p0:p0 + T], sin[p0:p0 + T])
    kr = _rope(k.view(B, T, nkv, D).transpose(1, 2), cos[p0:p0 + T], sin[p0:p0 + T])
    torch.testing.assert_close(q_out, qr, rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(kc[:, :, p0:p0 + T], kr, rtol=2e-3, atol=2e-3)
    assert torch.equal(vc[:, :, p0:p0 + T], v.view(B, T, nkv, D).transpose(1, 2))
    assert kc[:, :, :p0].abs().max() == 0 and kc[:, :, p0 + T:].abs().max() == 0


def test_fused_decode_step_matches_torch_glue(qa, device):
    """HIP glue kernels (RMSNorm, RoPE + KV append, single-query attention, SiLU*mul, residual epilogue) against the
    torch-op decode step on the same synthetic model: same hidden state up to fp16 rounding order."""
    from quick_amd.decoder import CONFIGS, SyntheticDecoder, decode_step_fused
    for batch in (1, 5):
        torch.manual_seed(1)
        ma = SyntheticDecoder(CONFIGS["tiny"], batch=batch, max_len=40, device=device, seed=3)
        mb = SyntheticDecoder(CONFIGS["tiny"], batch=batch, max_len=40, device=device, seed=3)
        ctx = 20
        tokens = torch.randint(0, 512, (batch, ctx), device=device)
        ta = ma.forward(tokens, torch.arange(ctx, device=device), None)
        tb = mb.forward(tokens, torch.arange(ctx, device=device), None)
        assert torch.equal(ta, tb)
        pos = torch.full((1,), ctx, dtype=torch.int64, device=device)
        mask = torch.full((1, 1, 1, 40), float("-inf"), dtype=torch.float16, device=device)
        mask[..., :ctx + 1] = 0
        for step in range(3):
            _, hid_f = decode_step_fused(mb, ta.view(batch, 1), pos)
            # torch-op step on model a, returning the final normed hidden state through the same path
            x_ref = _torch_decode_hidden(ma, ta.view(batch, 1), pos, mask)
            err = (hid_f.float() - x_ref.float()).abs().max() / x_ref.float().abs().max()
            assert err <= 1e-2, (batch, step, float(err))
            for la, lb in zip(ma.layers, mb.layers):
                ka, kb = la["k"][:, :, ctx + step].float(), lb["k"][:, :, ctx + step].float()
                assert (ka - kb).abs().max() <= 1e-2 * ka.abs().max() + 1e-3
            ta = (x_ref @ ma.lm_head.t()).argmax(-1)
            pos += 1
            mask[..., ctx + step + 1] = 0


@pytest.mark.parametrize("B,V,H,norm", [(1, 32000, 4096, True), (2, 32000, 4096, True), (4, 32000, 4096, False), (3, 777, 1024, True),
                                          (1, 1000, 512, False), (4, 128256, 8192, True), (1, 5, 512, True)])
def test_lm_head_argmax_against_torch(qa, device, B, V, H, norm):
    """Final RMSNorm + fp16 lm_head + greedy arg-max in two launches (quick_lm_head_argmax_f16) against torch: the hidden state bit for
    bit (quick_rmsnorm_f16's rounding), the logits within fp16 rounding of an fp32 product, the token = the lowest index among the
    largest of the kernel's own fp16 logits, and that logit within rounding of torch's maximum."""
    from quick_amd import kernels
    g = torch.Generator(device=device).manual_seed(V + H + B)
    x = torch.randn(B, H, device=device, generator=g).half()
    w = (torch.randn(V, H, device=device, generator=g) * 0.02).half()
    nw = (1 + 0.1 * torch.randn(H, device=device, generator=g)).half() if norm else None
    tok, hidden, logits = kernels.lm_head_argmax(x, w, nw, want_hidden=True, want_logits=True)
    torch.cuda.synchronize()
    h_ref = kernels.rmsnorm(x, nw) if norm else x
    assert torch.equal(hidden, h_ref)
    ref = h_ref.float() @ w.float().t()
    torch.testing.assert_close(logits.float(), ref, rtol=2e-3, atol=2e-3 * float(ref.abs().max()))
    for b in range(B):
        top = logits[b].max()
        first = int((logits[b] == top).nonzero()[0])
        assert int(tok[b]) == first, (b, int(tok[b]), first)
        assert abs(float(top) - float(ref[b].max())) <= 2e-3 * float(ref[b].abs().max()) + 1e-3
    # without the optional outputs: same token
    tok2, h2, l2 = kernels.lm_head_argmax(x, w, nw)
    assert h2 is None and l2 is None and torch.equal(tok2, tok)
    with pytest.raises(NotImplementedError):
        kernels.lm_head_argmax(torch.zeros(5, H, device=device, dtype=torch.float16), w, nw)


def _torch_decode_hidden(model, tok, pos, mask):
    from quick_amd.decoder import torch_decode_hidden
    return torch_decode_hidden(model, tok, pos, mask)


@pytest.mark.parametrize("K,N", [(8192, 10240), (8192, 57344), (28672, 8192)])
@pytest.mark.parametrize("M", [1, 16, 80])
def test_llama70b_shapes_against_dense_dequant(qa, device, K, N, M):
    """The largest layers of the e2e configs (Llama-2-70B fused qkv, fused gate_up, down).  The CPU oracle would take minutes
    here, so the reference is x @ W_deq with W_deq from the dequantisation kernel, which the golden tests pin bit-exactly."""
    from quick_amd.decoder import random_wqlinear
    g = torch.Generator(device=device).manual_seed(K + N)
    layer = random_wqlinear(K, N, 128, device, g)
    x = torch.randn(M, K, device=device, generator=g).half()
    w = qa.dequantize_mi355x(layer.qweight, layer.scales, layer.qzeros)
    want = x.float() @ w.float()
    y = layer(x)
    assert tuple(y.shape) == (M, N)
    assert float((y.float() - want).abs().max() / want.abs().max()) <= TOL
    # second net, independent of the GPU's own dequantisation: 256 sampled channels through the CPU oracle
    cols = np.unique(np.random.default_rng(K + N + M).integers(0, N, 256))
    iw, s, z = oracle.unpack_mi355x_columns(layer.qweight.cpu().numpy(), layer.scales.cpu().numpy(), layer.qzeros.cpu().numpy(), cols)
    ref = oracle.w4a16_forward(x.cpu().numpy(), iw, s, z, 128).astype(np.float32)
    got = y[:, torch.from_numpy(cols).to(device)].float().cpu().numpy()
    assert float(np.abs(got - ref).max()) <= TOL * float(np.abs(ref).max())


def test_random_shapes_against_dequantised_matmul(qa, device):
    """60 seeded random (M, K, N, G) draws through whatever the planner picks (skinny / tiled / wide / exchange-K / four-wave tiles up to
    256 x 256, K splits that are not powers of two, ragged M, odd stage counts), twice each with the same workspace, against
    fp32 matmul over the weights dequantised on the GPU (quick_dequantize_mi355x_f16 is bit-exact against the oracle,
    see above).  Not a replacement for the oracle sweeps: a net for planner branches no fixed list thought of."""
    from quick_amd import kernels as K_, packing
    rng = np.random.default_rng(20260928)
    gen = torch.Generator(device=device)
    for case in range(int(os.environ.get("QUICK_AMD_RANDOM_CASES", "60"))):   # (a longer soak: set the variable)
        G = int(rng.choice([32, 64, 128, 128, 128, 256]))
        unit = max(G, 128)                                   # K is a multiple of 128 and of the group size
        kmax = 28672 if case % 5 == 4 else 8192              # every fifth draw may have a long K (the planner's long-K rules)
        K = int(rng.integers(1, kmax // unit + 1)) * unit
        N = int(rng.integers(1, 97)) * 128
        M = int(rng.choice([1, 2, 3, 4, 5, 6, 8, 12, 13, 16, 17, 24, 32, 40, 48, 57, 63, 64, 65, 96, 100, 128, 200, 257, 384, 520, 700, 1100, 2100, 4200]))
        if M * N * K > 2.5e10:
            M = max(1, int(2.5e10 // (N * K)))
        gen.manual_seed(case)
        qw, sc, qz = packing.random_mi355x(K, N, G, device, generator=gen)
        x = (torch.randn(M, K, device=device, generator=gen) * 0.5).half()
        ref = x.float() @ K_.dequantize_mi355x(qw, sc, qz).float()
        y1 = qa.gemm_forward(x, qw, sc, qz)
        y2 = qa.gemm_forward(x, qw, sc, qz)
        assert torch.equal(y1, y2), (case, M, K, N, G, K_.plan_describe(M, K, N, G))
        err = (y1.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        assert err <= TOL, (case, M, K, N, G, err, K_.plan_describe(M, K, N, G))
        _check_sampled_columns_against_oracle(y1, x, qw, sc, qz, G, seed=case, what=(case, M, K, N, G, K_.plan_describe(M, K, N, G)))
    print(f"{case + 1} random shapes checked")


def _check_sampled_columns_against_oracle(y, x, qw, sc, qz, G, seed, what, add=None, ncols=128, tol=TOL):
    """Second net of the random-shape tests, independent of the GPU's own dequantisation kernel: `ncols` sampled output channels
    of a layer made on the GPU, evaluated by the CPU oracle's closed form (oracle.unpack_mi355x_columns + w4a16_forward)."""
    N = y.shape[1]
    cols = np.unique(np.random.default_rng(seed).integers(0, N, ncols))
    iw, s, z = oracle.unpack_mi355x_columns(qw.cpu().numpy(), sc.cpu().numpy(), qz.cpu().numpy(), cols)
    ref = oracle.w4a16_forward(x.cpu().numpy(), iw, s, z, G).astype(np.float32)
    if add is not None:
        ref = ref + add[:, cols] if add.ndim == 2 else ref + add[cols]
    got = y[:, torch.from_numpy(cols).to(y.device)].float().cpu().numpy()
    assert float(np.abs(got - ref).max()) <= tol * max(float(np.abs(ref).max()), 1e-30), what


def test_random_shapes_with_fused_epilogues_and_prologue(qa, device):
    """The same kind of net for the fusions: seeded random shapes through whatever kernel the planner picks, with a random
    one of {bias, residual, bias + residual, SiLU*mul, RMSNorm prologue (where the planner's kernel takes it) + residual},
    against torch ops around the fp32 matmul over the GPU-dequantised weights."""
    from quick_amd import kernels as K_, packing
    rng = np.random.default_rng(77)
    gen = torch.Generator(device=device)
    seen = set()
    for case in range(int(os.environ.get("QUICK_AMD_RANDOM_CASES", "80"))):
        G = int(rng.choice([64, 128, 128, 128, 256]))
        unit = max(G, 128)
        K = int(rng.integers(1, (16384 if case % 4 == 3 else 4096) // unit + 1)) * unit
        N = int(rng.integers(1, 65)) * 256                   # (SiLU*mul pairs gate / up channels: N / 2 must stay a multiple of 128)
        M = int(rng.choice([1, 2, 4, 6, 8, 12, 16, 24, 48, 64, 96, 130, 300, 520, 1030, 2500]))
        if M * N * K > 1.2e10:
            M = max(1, int(1.2e10 // (N * K)))
        gen.manual_seed(1000 + case)
        qw, sc, qz = packing.random_mi355x(K, N, G, device, generator=gen)
        x = (torch.randn(M, K, device=device, generator=gen) * 0.5).half()
        w = K_.dequantize_mi355x(qw, sc, qz).float()
        bias = (torch.randn(N, device=device, generator=gen) * 0.5).half()
        res = torch.randn(M, N, device=device, generator=gen).half()
        kind = int(rng.integers(0, 5))
        if kind == 4 and not K_.can_fuse_rmsnorm(M, K, N, G):
            kind = 1
        seen.add(kind)
        what = (case, kind, M, K, N, G, K_.plan_describe(M, K, N, G))
        if kind == 0:
            y, ref = qa.gemm_forward(x, qw, sc, qz, bias=bias), x.float() @ w + bias.float()
            _check_sampled_columns_against_oracle(y, x, qw, sc, qz, G, 1000 + case, what, add=bias.float().cpu().numpy())
        elif kind == 1:
            y, ref = qa.gemm_forward(x, qw, sc, qz, residual=res), x.float() @ w + res.float()
            _check_sampled_columns_against_oracle(y, x, qw, sc, qz, G, 1000 + case, what, add=res.float().cpu().numpy())
        elif kind == 2:
            y, ref = qa.gemm_forward(x, qw, sc, qz, bias=bias, residual=res), x.float() @ w + bias.float() + res.float()
            _check_sampled_columns_against_oracle(y, x, qw, sc, qz, G, 1000 + case, what, add=(bias.float()[None, :] + res.float()).cpu().numpy())
        elif kind == 3:
            gu = (x.float() @ w).half().view(M, N // 16, 2, 8)                 # gate / up interleaved by 8
            ref = (torch.nn.functional.silu(gu[:, :, 0].float()).half() * gu[:, :, 1]).reshape(M, N // 2).float()
            y = qa.gemm_forward(x, qw, sc, qz, silu_mul=True)
        else:
            lnw = (torch.rand(K, device=device, generator=gen) + 0.5).half()
            xn = ((x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5)).half() * lnw)
            y, ref = qa.gemm_forward(x, qw, sc, qz, rmsnorm_weight=lnw, rmsnorm_eps=1e-5, residual=res), xn.float() @ w + res.float()
        err = (y.float() - ref).abs().max().item() / max(ref.abs().max().item(), 1e-30)
        assert err <= (2 if kind == 3 else 1) * TOL, (case, kind, M, K, N, G, err, K_.plan_describe(M, K, N, G))
    assert len(seen) == 5


@pytest.mark.parametrize("kernel_id", [wide(2, 1), wide(2, 2), wide(4, 1), wide(4, 2), wide(8, 1), wide(8, 2), wide(2, 1) | WIDE_NORING,
                                       wide(4, 2) | WIDE_NORING, wide(2, 1) | WIDE_8WAVES, wide(2, 2) | WIDE_8WAVES, wide(4, 1) | WIDE_8WAVES],
                         ids=["64x128", "64x256", "128x128", "128x256", "256x128", "256x256", "64x128nr", "128x256nr", "64x128w8", "64x256w8", "128x128w8"])
@pytest.mark.parametrize("M,K,N", [(300, 512, 512), (77, 1152, 768), (1, 256, 1024), (513, 384, 256)])
def test_wide_family_way_out(qa, device, M, K, N, kernel_id):
    """Every tile of the 32x32x16 family through its LDS-staged way out: ragged token counts (last tile 44 / 13 / 1 rows), bias +
    residual (the residual is added to the ROUNDED product, as GEMM-then-add does), SiLU*mul (half the channels), and a forced K
    split of 2 and 3 slices (the last arriver's exit)."""
    from quick_amd import kernels as K_
    if ((kernel_id >> 8) & 15) == 2 and N % 256 != 0:
        pytest.skip("256-channel tiles need N % 256 == 0")
    G = 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + 11)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    assert K_.plan_describe(M, K, N, G, kernel_id).startswith("wide")
    y = qa.gemm_forward(xd, *packed, kernel_id=kernel_id)
    assert rel_err(y.cpu().numpy(), want) <= TOL
    yb = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kernel_id)
    two = (qa.gemm_forward(xd, *packed, bias=bias, kernel_id=kernel_id).float() + res.float()).half()
    assert torch.equal(yb, two)                                     # bit for bit the two-step result
    assert rel_err(yb.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL
    for ks in (2, 3):
        y2 = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kernel_id, grid_split_k=ks)
        assert rel_err(y2.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL
        assert torch.equal(y2, qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kernel_id, grid_split_k=ks))   # order of arrival does not matter
    y_act = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kernel_id)
    assert y_act.shape == (M, N // 2)
    torch.testing.assert_close(y_act, K_.silu_mul(y), rtol=2e-3, atol=2e-3)
    y_act2 = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kernel_id, grid_split_k=2)
    torch.testing.assert_close(y_act2, K_.silu_mul(y), rtol=2e-3, atol=2e-3)


@pytest.mark.parametrize("kernel_id", [TILED_WIDE, TILED_BIG], ids=["64x256", "128x256"])
@pytest.mark.parametrize("M,K,N,G", [(300, 512, 512, 128), (129, 1152, 768, 64), (640, 256, 1024, 32), (1100, 384, 512, 128)])
def test_wide_tiles_epilogues_and_k_split(qa, device, M, K, N, G, kernel_id):
    """The 256-channel tile variants with every epilogue (bias, residual, SiLU*mul) and with a forced K split, ragged M."""
    from quick_amd import kernels as K_
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G + 5)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    assert f"channels=256" in K_.plan_describe(M, K, N, G, kernel_id)
    y = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kernel_id)
    ref = want + bias.float().cpu().numpy() + res.float().cpu().numpy()
    assert rel_err(y.cpu().numpy(), ref) <= TOL
    for ks in (2, 3):
        y2 = qa.gemm_forward(xd, *packed, kernel_id=kernel_id, grid_split_k=ks)
        assert rel_err(y2.cpu().numpy(), want) <= TOL
    y_act = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kernel_id)
    torch.testing.assert_close(y_act, K_.silu_mul(qa.gemm_forward(xd, *packed, kernel_id=kernel_id)), rtol=2e-3, atol=2e-3)



def test_fused_decode_step_llama2_7b_layer_matches_torch_glue(qa, device):
    """The stack bench.py times, at its real widths: ONE Llama-2-7B decoder layer (4096 hidden, 11008 intermediate, 32 heads) at
    bs = 1 and 16 -- the fused decode step (HIP glue kernels, GEMM epilogues, RMSNorm prologues) against the torch-op step."""
    import dataclasses
    from quick_amd.decoder import CONFIGS, SyntheticDecoder, decode_step_fused
    cfg = dataclasses.replace(CONFIGS["llama2-7b"], layers=1, vocab=2048)
    for batch in (1, 16):
        ma = SyntheticDecoder(cfg, batch=batch, max_len=48, device=device, seed=5)
        mb = SyntheticDecoder(cfg, batch=batch, max_len=48, device=device, seed=5)
        ctx = 24
        tokens = torch.randint(0, cfg.vocab, (batch, ctx), device=device)
        ta = ma.forward(tokens, torch.arange(ctx, device=device), None)
        tb = mb.forward(tokens, torch.arange(ctx, device=device), None)
        assert torch.equal(ta, tb)
        pos = torch.full((1,), ctx, dtype=torch.int64, device=device)
        mask = torch.full((1, 1, 1, 48), float("-inf"), dtype=torch.float16, device=device)
        mask[..., :ctx + 1] = 0
        for step in range(2):
            _, hid_f = decode_step_fused(mb, ta.view(batch, 1), pos)
            x_ref = _torch_decode_hidden(ma, ta.view(batch, 1), pos, mask)
            err = (hid_f.float() - x_ref.float()).abs().max() / x_ref.float().abs().max()
            assert err <= 1e-2, (batch, step, float(err))
            ta = (x_ref @ ma.lm_head.t()).argmax(-1)
            pos += 1
            mask[..., ctx + step + 1] = 0


# ------------------------------------------------------------------------------------------------
# exchange-K kernels (quick_amd/csrc/w4a16_xk.hpp): K slices of a tile on different CUs, partial tiles swapped through mailboxes
# ------------------------------------------------------------------------------------------------
def xk(mb, s=0):
    return XK | (mb << 4) | (s << 8)


@pytest.mark.parametrize("S", [1, 2, 4, 8])
@pytest.mark.parametrize("mb", [2, 4], ids=["64tok", "128tok"])
@pytest.mark.parametrize("M,K,N,G", [(300, 512, 512, 128), (77, 1152, 768, 128), (1, 1024, 1024, 128), (513, 1024, 256, 128),
                                     (64, 2048, 384, 128), (130, 4096, 256, 256), (40, 1536, 128, 512)])
def test_xk_family_against_oracle(qa, device, M, K, N, G, mb, S):
    """Every slice count x both tile sizes: ragged token counts, odd stage counts (K / 128 not a multiple of S: the planner lowers S),
    group sizes above 128; plain, bias + residual (bit for bit the two-step result), SiLU * mul where a wave finishes whole
    32-token blocks; every result twice (the sums are taken in slice order: no dependence on timing)."""
    from quick_amd import kernels as K_
    kid = xk(mb, S)
    plan = K_.plan_describe(M, K, N, G, kid)
    assert plan.startswith("xk"), plan
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G + S)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    y = qa.gemm_forward(xd, *packed, kernel_id=kid)
    assert rel_err(y.cpu().numpy(), want) <= TOL, plan
    assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=kid)), plan
    yb = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid)
    two = (qa.gemm_forward(xd, *packed, bias=bias, kernel_id=kid).float() + res.float()).half()
    assert torch.equal(yb, two), plan
    assert rel_err(yb.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL, plan
    slices = int(plan.split("slices=")[1].split()[0])
    # r04: with a poll limit of two ticks every wave gives its part up at once and the LAST slice to arrive finishes it from the boxes --
    # the same sums in the same order: bit for bit the same result (no trap, no co-residency requirement)
    os.environ["QUICK_AMD_EXCHANGE_POLL_LOG2"] = "1"
    try:
        assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=kid)), plan
        assert torch.equal(yb, qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid)), plan
        if (mb // 2 * 16) % (16 * slices) == 0:
            assert torch.equal(qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid), qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)), plan
            y_gu = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)
    finally:
        del os.environ["QUICK_AMD_EXCHANGE_POLL_LOG2"]
    if (mb // 2 * 16) % (16 * slices) == 0:
        y_act = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)
        assert y_act.shape == (M, N // 2)
        torch.testing.assert_close(y_act, K_.silu_mul(y), rtol=2e-3, atol=2e-3)
        assert torch.equal(y_act, y_gu), plan
    else:
        with pytest.raises(NotImplementedError):
            qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)


def test_xk_exchange_under_uneven_load(qa, device):
    """The mailbox protocol under uneven load: launches of different slice counts and tile sizes alternate on ONE workspace (the exchange
    zone is shared and must be all-zero again after every launch) while a second stream keeps part of the chip busy with dense
    GEMMs of changing size, so that the slices of a tile finish at different times and some arrive long before their partners.
    Every word of every result is compared with the first launch's, and the first launch with the oracle."""
    cases = []
    for (M, K, N), kid in (((512, 4096, 4096), xk(4, 2)), ((512, 4096, 4096), xk(2, 1)), ((256, 4096, 4096), xk(4, 4)), ((128, 4096, 4096), xk(4, 8)),
                           ((64, 4096, 4096), xk(2, 8)), ((64, 8192, 2048), xk(2, 4)), ((200, 2048, 1024), xk(2, 2)), ((130, 1024, 3072), xk(4, 2))):
        x, iw, s, z = oracle.make_synthetic(M, K, N, 128, seed=M + N + K)
        cols = np.unique(np.random.default_rng(M + N).integers(0, N, 96))
        want = oracle.w4a16_forward(x, iw[:, cols], s[:, cols], z[:, cols], 128).astype(np.float32)
        cases.append((_dev(x, device), _pack_dev(iw, s, z, device), kid, torch.from_numpy(cols).to(device), want))
    side = torch.cuda.Stream()
    a = torch.randn(2048, 2048, device=device).half()
    first = [None] * len(cases)
    for rep in range(12):
        with torch.cuda.stream(side):
            for i in range(3 + rep % 4):
                n = 256 * (1 + (rep + i) % 8)
                torch.matmul(a[:n], a)
        for i, (xd, packed, kid, cols, want) in enumerate(cases):
            y = qa.gemm_forward(xd, *packed, kernel_id=kid)
            if first[i] is None:
                first[i] = y
                got = y[:, cols].float().cpu().numpy()
                assert float(np.abs(got - want).max()) <= TOL * float(np.abs(want).max()), (rep, i)
            assert torch.equal(y, first[i]), (rep, i)
        torch.cuda.synchronize()
        from quick_amd import kernels as K_
        for ws in K_._WORKSPACES.values():   # counters and exchange zone: handed back all-zero, every launch
            assert int(ws[: (64 << 10) + (16 << 20)].count_nonzero()) == 0, rep


# ------------------------------------------------------------------------------------------------
# four-wave kernels with generated hand-placed K loops (quick_amd/csrc/w4a16_xw.hpp, tools/gen_xw_loop.py): 128 x 256, 128 x 128 and
# 64 x 128 tiles; K slices of a tile on different CUs exchange fp16 parts and give up on partners that are not there
# ------------------------------------------------------------------------------------------------
XW = 5


def xw(mb, pairs, s=0, poll_log2=0):
    return XW | ((mb << 4) if mb != 4 else 0) | ((1 << 12) if pairs == 1 else 0) | (s << 8) | (poll_log2 << 22)


@pytest.mark.gpu
@pytest.mark.parametrize("kid", [5 | (8 << 4) | (1 << 12), 5 | (8 << 4), 5 | (1 << 12), 5 | (2 << 4)], ids=["256tok+bit12", "256tok", "bit12", "64tok"])
def test_forced_four_wave_id_with_half_a_256_channel_tile(qa, device, kid):
    """N % 256 == 128 under a forced four-wave id -- every output channel is written (NaN-poisoned output), whichever
    kernel the id resolves to."""
    M, K, N, G = 256, 1024, 384, 128
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=kid)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=device)
    y = qa.gemm_forward(_dev(x, device), *_pack_dev(iw, s, z, device), kernel_id=kid, out=out)
    assert not torch.isnan(y).any()
    assert rel_err(y.cpu().numpy(), want) <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("M", [9, 13, 16])
@pytest.mark.parametrize("K,N,ks", [(8192, 1024, 1), (8192, 1024, 2), (8192, 512, 4), (4096, 2048, 1), (4096, 1024, 2), (2048, 1024, 1), (7168, 1024, 1), (28672, 256, 4)],
                         ids=["T8", "T4x2", "T2x4", "T4", "T2x2", "T2", "T7", "T7x4"])
def test_eight_tile_fragment_kernel_against_oracle(qa, device, M, K, N, ks):
    """[r05] w4a16_frag8_kernel -- eight channel tiles per workgroup, straight-line, every wave exactly T k tiles -- forced by kernel id
    (SKINNY, 8 tiles) over every T it is built for and 1 / 2 / 4 K slices: against the oracle into a NaN-poisoned output, three times
    (the loop form of this instantiation failed from run to run), with bias + residual (bias before the product's rounding, the residual after it, as the four-tile kernel), and SiLU * mul."""
    from quick_amd import kernels as K_
    kid = K_.KERNEL_SKINNY | (8 << 4)
    plan = K_.plan_describe(M, K, N, 128, kid, ks)
    assert plan.startswith("skinny ntw=8 ") and f"ksplit={ks}" in plan, plan
    x, iw, s, z = oracle.make_synthetic(M, K, N, 128, seed=M + K + N + ks)
    want = oracle.w4a16_forward(x, iw, s, z, 128).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    ys = []
    for _ in range(3):
        out = torch.full((M, N), float("nan"), dtype=torch.float16, device=device)
        ys.append(qa.gemm_forward(xd, *packed, kernel_id=kid, grid_split_k=ks, out=out))
        assert rel_err(ys[-1].cpu().numpy(), want) <= TOL, plan
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[1], ys[2]), plan
    y4 = qa.gemm_forward(xd, *packed, kernel_id=K_.KERNEL_SKINNY | (4 << 4) | (2 << 8))
    assert rel_err(ys[0].cpu().numpy(), y4.float().cpu().numpy()) <= 1e-3
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    yb = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid, grid_split_k=ks)   # (skinny_finish: GEMM-then-add rounding)
    assert rel_err(yb.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL, plan
    assert torch.equal(yb, qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=K_.KERNEL_SKINNY | (4 << 4) | (2 << 8), grid_split_k=ks)) or \
        rel_err(yb.cpu().numpy(), qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=K_.KERNEL_SKINNY | (4 << 4) | (2 << 8)).float().cpu().numpy()) <= 1e-3
    ysm = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid, grid_split_k=ks)
    yf = ys[0].float().view(M, N // 16, 2, 8)
    ref = (torch.nn.functional.silu(yf[:, :, 0].half().float()).half().float() * yf[:, :, 1]).half().view(M, N // 2)
    assert (ysm.float() - ref.float()).abs().max() <= 2e-3 * ref.float().abs().max() + 1e-3, plan
    with pytest.raises(NotImplementedError):
        qa.gemm_forward(xd, *packed, kernel_id=kid, grid_split_k=ks, rmsnorm_weight=torch.ones(K, dtype=torch.float16, device=device))


@pytest.mark.gpu
@pytest.mark.parametrize("M", [9, 13, 16])
@pytest.mark.parametrize("N", [896, 1792, 2688])
def test_seven_tile_fragment_kernel_against_oracle(qa, device, M, N):
    """[r06, late] the straight-line fragment kernel with SEVEN channel tiles per workgroup (T = 8: K = 8192, one slice) -- the launch AUTO runs on layers whose block
    count makes whole rounds that way (16 x 8192 x 57344: 448 blocks of 128 channels -> 512 of 112).  Forced by kernel id (SKINNY, 7 tiles) on widths of 8, 16 and 24
    blocks: against the oracle into a NaN-poisoned output, three times bit-equal, against the four-tile kernel, with bias + residual, SiLU * mul, and no RMSNorm prologue."""
    from quick_amd import kernels as K_
    K = 8192
    kid = K_.KERNEL_SKINNY | (7 << 4)
    plan = K_.plan_describe(M, K, N, 128, kid)
    assert plan.startswith("skinny ntw=7 ") and "ksplit=1" in plan and f"grid={N // 112}x" in plan, plan
    x, iw, s, z = oracle.make_synthetic(M, K, N, 128, seed=M + N)
    want = oracle.w4a16_forward(x, iw, s, z, 128).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    ys = []
    for _ in range(3):
        out = torch.full((M, N), float("nan"), dtype=torch.float16, device=device)
        ys.append(qa.gemm_forward(xd, *packed, kernel_id=kid, out=out))
        assert rel_err(ys[-1].cpu().numpy(), want) <= TOL, plan
    assert torch.equal(ys[0], ys[1]) and torch.equal(ys[1], ys[2]), plan
    y4 = qa.gemm_forward(xd, *packed, kernel_id=K_.KERNEL_SKINNY | (1 << 4))
    assert rel_err(ys[0].cpu().numpy(), y4.float().cpu().numpy()) <= 1e-3
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    yb = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid)
    assert rel_err(yb.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL, plan
    ysm = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)
    yf = ys[0].float().view(M, N // 16, 2, 8)
    ref = (torch.nn.functional.silu(yf[:, :, 0].half().float()).half().float() * yf[:, :, 1]).half().view(M, N // 2)
    assert (ysm.float() - ref.float()).abs().max() <= 2e-3 * ref.float().abs().max() + 1e-3, plan
    with pytest.raises(NotImplementedError):
        qa.gemm_forward(xd, *packed, kernel_id=kid, rmsnorm_weight=torch.ones(K, dtype=torch.float16, device=device))


@pytest.mark.gpu
def test_llama2_70b_gate_up_shape_runs_seven_tiles_and_equals_eight(qa, device):
    """AUTO at 16 x 8192 x 57344 (Llama-2-70B gate_up at bs = 16) takes the seven-tile launch (two whole rounds of workgroups); the whole output against the forced
    eight-tile launch -- the same sums in the same order per output: bit-equal (sampled channels against the oracle: test_e2e_layer_shapes_sampled_channels_against_oracle)."""
    from quick_amd import kernels as K_, packing
    M, K, N = 16, 8192, 57344
    assert K_.plan_describe(M, K, N, 128).startswith("skinny ntw=7 "), K_.plan_describe(M, K, N, 128)
    gen = torch.Generator(device=device).manual_seed(7)
    qw, sc, qz = packing.random_mi355x(K, N, 128, device, gen)
    x = (torch.randn(M, K, device=device, generator=gen) * 0.5).half()
    out = torch.full((M, N), float("nan"), dtype=torch.float16, device=device)
    y7 = qa.gemm_forward(x, qw, sc, qz, out=out)
    y8 = qa.gemm_forward(x, qw, sc, qz, kernel_id=K_.KERNEL_SKINNY | (8 << 4))
    assert not torch.isnan(y7).any()
    assert torch.equal(y7, y8)


XW_TILES = [(4, 2), (4, 1), (2, 1), (8, 2)]
XW_IDS = ["128x256", "128x128", "64x128", "256x256"]


@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("mb,pairs", XW_TILES, ids=XW_IDS)
@pytest.mark.parametrize("M,K,N,G", [(300, 512, 512, 128), (77, 1152, 768, 128), (1, 1024, 1024, 128), (513, 1024, 256, 128),
                                     (64, 2048, 512, 128), (130, 4096, 256, 256), (40, 1536, 256, 512), (128, 128, 256, 128)])
def test_xw_family_against_oracle(qa, device, M, K, N, G, mb, pairs, S):
    """Every tile shape x slice count: ragged token counts, stage counts that are not multiples of S (the planner lowers S), one-stage
    slices, group sizes above 128; plain, bias + residual (bit for bit the two-step result), SiLU * mul; every result twice (sums are
    taken in slice order over the same fp16-rounded parts: no dependence on timing) -- and once more with a poll limit of two ticks, where
    every wave gives its block up at once and the LAST partner to arrive finishes it from the boxes: bit for bit the same result."""
    from quick_amd import kernels as K_
    if S > mb or (mb == 8 and S > 1):
        pytest.skip("whole 32-token blocks per slice; the 256 x 256 tile runs one slice")
    kid = xw(mb, pairs, S)
    plan = K_.plan_describe(M, K, N, G, kid)
    assert plan.startswith("xw"), plan
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G + S)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    y = qa.gemm_forward(xd, *packed, kernel_id=kid)
    assert rel_err(y.cpu().numpy(), want) <= TOL, plan
    assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=kid)), plan
    assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=xw(mb, pairs, S, poll_log2=1))), plan      # everybody gives up
    yb = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid)
    two = (qa.gemm_forward(xd, *packed, bias=bias, kernel_id=kid).float() + res.float()).half()
    assert torch.equal(yb, two), plan
    assert torch.equal(yb, qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=xw(mb, pairs, S, poll_log2=1))), plan
    assert rel_err(yb.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL, plan
    y_act = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)
    assert y_act.shape == (M, N // 2)
    torch.testing.assert_close(y_act, K_.silu_mul(y), rtol=2e-3, atol=2e-3)
    assert torch.equal(y_act, qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=xw(mb, pairs, S, poll_log2=1))), plan


@pytest.mark.parametrize("mb,pairs", XW_TILES, ids=XW_IDS)
def test_xw_golden_fixtures_and_reference_pin(qa, device, pin, mb, pairs):
    """The reference-made fixtures end to end (reference-format checkpoint -> HIP repack -> the four-wave kernels), and the 4096 x 4096 pin
    of the reference packer / CPU path at the bench's token counts (the fixture's 16 rows repeated), one slice and as many as fit."""
    for path in GOLD:
        g = load_golden(path)
        if int(g["G"]) % 128 or int(g["N"]) % (pairs * 128):
            continue
        qw, qs, qz = qa.repack_cuda_to_mi355x(_dev(g["ref_qweight"], device), _dev(g["ref_qscales"], device), _dev(g["ref_qzeros"], device))
        for S in (1, 2):
            y = qa.gemm_forward(_dev(g["x"], device), qw, qs, qz, kernel_id=xw(mb, pairs, S))
            assert rel_err(y.cpu().numpy(), g["ref_y"]) <= TOL, (path, S)
    g, iw, s, z = pin
    packed = _pack_dev(iw, s, z, device)
    ref = g["y_ref"].astype(np.float32)
    for M in (64, 512):
        x = np.tile(g["x"], (M // g["x"].shape[0], 1))
        for kid in (xw(mb, pairs), xw(mb, pairs, 1)):
            y = qa.gemm_forward(_dev(x, device), *packed, kernel_id=kid).cpu().numpy().astype(np.float32)
            for rep in (0, M // 16 - 1):
                assert float(np.abs(y[g["y_rows"] + 16 * rep, g["y_cols"]] - ref).max()) <= TOL * float(np.abs(ref).max())
            assert float(np.abs(np.abs(y).sum(0) - g["col_abs_sum"] * (M // 16)).max()) <= TOL * float(g["col_abs_sum"].max()) * (M // 16)


@pytest.mark.parametrize("M,K,N,G", [(256, 256, 256, 128), (129, 384, 512, 128), (1000, 1024, 768, 128), (2049, 384, 512, 128), (4100, 1280, 1024, 256),
                                     (300, 128, 256, 128)])
def test_xw_256x256_tile_equals_the_r02_kernel_bit_for_bit(qa, device, M, K, N, G):
    """The generated 256 x 256 loop (waves of 256 tokens x 64 channels, ring of two slots) sums every output in the same k order as r02's
    hipcc-scheduled 256 x 256 kernel: equal bits, whatever the token count does to the two 128-row halves of the way out (rows past M in
    the first half only, in the second, a whole half missing), several tiles per XCD, one- to nine-stage K (the r02 kernel pinned to one K slice: its split launches add fp32 slabs); and against the oracle."""
    from quick_amd import kernels as K_
    kid = xw(8, 2, 1)
    assert K_.plan_describe(M, K, N, G, kid).startswith("xw tokens=256 channels=256")
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    y = qa.gemm_forward(xd, *packed, kernel_id=kid)
    assert rel_err(y.cpu().numpy(), want) <= TOL
    assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=wide(8, 2) | WIDE_NORING, grid_split_k=1))
    bias = torch.linspace(-1, 1, N, device=device).half()
    res = torch.randn(M, N, device=device).half()
    assert torch.equal(qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid),
                       qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=wide(8, 2) | WIDE_NORING, grid_split_k=1))
    assert torch.equal(qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid), qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=wide(8, 2) | WIDE_NORING, grid_split_k=1))


def test_xw_exchange_when_partners_are_not_there(qa, device):
    """The slices of a tile need not be co-resident: (a) an S = 4 launch while a long-running kernel on another
    stream holds most of the chip -- partner workgroups are dispatched one kernel-length apart; (b) two S > 1 launches on two streams at
    the same time, each on its own workspace; (c) the same with a poll limit of 2.5 us, so that give-ups and in-time exchanges mix inside
    one launch.  No trap, no hang, every word equals the undisturbed launch's -- written into NaN-poisoned buffers, so that a block nobody
    finished shows whatever the allocator hands back -- and counters and exchange zone of every workspace are all-zero again after every
    round (this check found the store hazard described at xw_mail_store; tools/exchange_stress.py is the long form of this test)."""
    from quick_amd import kernels as K_

    def poisoned(y0):
        return torch.full_like(y0, float("nan"))

    def workspaces_clean():
        for ws in K_._WORKSPACES.values():
            if int(ws[: (64 << 10) + (16 << 20)].count_nonzero()) != 0:
                return False
        return True
    cases = []
    for (M, K, N), kid in (((512, 4096, 4096), xw(4, 2, 4)), ((512, 4096, 4096), xw(4, 1, 2)), ((256, 4096, 4096), xw(2, 1, 2)),
                           ((1024, 4096, 4096), xw(4, 2, 2)), ((128, 8192, 2048), xw(4, 1, 4)),
                           ((128, 4096, 4096), xk(2, 4)), ((64, 11008, 4096), xk(2, 8)), ((512, 4096, 4096), xk(4, 2)),
                           ((200, 4096, 2048), xk(4, 4)), ((64, 4096, 6144), xk(2, 4))):
        x, iw, s, z = oracle.make_synthetic(M, K, N, 128, seed=M + N + K)
        cols = np.unique(np.random.default_rng(M + N).integers(0, N, 96))
        want = oracle.w4a16_forward(x, iw[:, cols], s[:, cols], z[:, cols], 128).astype(np.float32)
        xd, packed = _dev(x, device), _pack_dev(iw, s, z, device)
        y0 = qa.gemm_forward(xd, *packed, kernel_id=kid)
        got = y0[:, torch.from_numpy(cols).to(device)].float().cpu().numpy()
        assert float(np.abs(got - want).max()) <= TOL * float(np.abs(want).max())
        cases.append((xd, packed, kid, y0))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(8192, 8192, device=device).half()
    for rep in range(6):
        # (a) a dense 8192^3 GEMM (256+ workgroups, ~1 ms) on the side stream while the S > 1 launches run
        with torch.cuda.stream(side):
            torch.matmul(big, big)
        for xd, packed, kid, y0 in cases:
            for poll in (0, 8):
                if (kid & 15) == XK:   # (the exchange-K kernel ids use bits 22.. for their ring depth: the limit comes from the environment)
                    os.environ["QUICK_AMD_EXCHANGE_POLL_LOG2"] = str(poll)
                y = qa.gemm_forward(xd, *packed, kernel_id=kid | ((poll << 22) if (kid & 15) == XW else 0), out=poisoned(y0))
                os.environ.pop("QUICK_AMD_EXCHANGE_POLL_LOG2", None)
                assert torch.equal(y, y0), (rep, kid, poll)
        torch.cuda.synchronize()
        assert workspaces_clean(), rep
        # (b) two exchange launches at once on two streams (the Python face keeps one workspace per stream)
        xa, pa, ka, ya = cases[rep % len(cases)]
        xb, pb, kb, yb = cases[(rep + 1) % len(cases)]
        if rep % 2:
            os.environ["QUICK_AMD_EXCHANGE_POLL_LOG2"] = "8"
        with torch.cuda.stream(side):
            outs_b = [qa.gemm_forward(xb, *pb, kernel_id=kb, out=poisoned(yb)) for _ in range(4)]
        outs_a = [qa.gemm_forward(xa, *pa, kernel_id=ka, out=poisoned(ya)) for _ in range(4)]
        os.environ.pop("QUICK_AMD_EXCHANGE_POLL_LOG2", None)
        torch.cuda.synchronize()
        assert all(torch.equal(o, ya) for o in outs_a) and all(torch.equal(o, yb) for o in outs_b), rep
        assert workspaces_clean(), rep


def test_decode_full_stack_llama2_7b_fused_against_torch_ops(qa, device):
    """What bench.py's decode leg times, whole: the 32-layer Llama-2-7B synthetic stack (random packed weights of the real shapes), bs = 1
    and 16, four decode steps -- the fused step (HIP glue, GEMM epilogues, RMSNorm prologues, lm_head kernel) against the torch-op step
    (the methodology restated from the reference's examples/benchmark.py:38-67): final hidden state within tolerance at every step and
    the same greedy tokens wherever the torch-op logits separate the top two candidates by more than the tolerance."""
    from quick_amd.decoder import CONFIGS, SyntheticDecoder, decode_step_fused
    cfg = CONFIGS["llama2-7b"]
    for batch in (1, 16):
        ma = SyntheticDecoder(cfg, batch=batch, max_len=40, device=device, seed=11)
        mb_ = SyntheticDecoder(cfg, batch=batch, max_len=40, device=device, seed=11)
        ctx = 16
        tokens = torch.randint(0, cfg.vocab, (batch, ctx), device=device)
        ta = ma.forward(tokens, torch.arange(ctx, device=device), None)
        tb = mb_.forward(tokens, torch.arange(ctx, device=device), None)
        assert torch.equal(ta, tb)
        pos = torch.full((1,), ctx, dtype=torch.int64, device=device)
        mask = torch.full((1, 1, 1, 40), float("-inf"), dtype=torch.float16, device=device)
        mask[..., :ctx + 1] = 0
        for step in range(4):
            tok_f, hid_f = decode_step_fused(mb_, ta.view(batch, 1), pos)
            x_ref = _torch_decode_hidden(ma, ta.view(batch, 1), pos, mask)
            err = (hid_f.float() - x_ref.float()).abs().max() / x_ref.float().abs().max()
            assert err <= 2e-2, (batch, step, float(err))      # 32 layers of fp16 round-off between two different op orders
            logits = (x_ref.float() @ ma.lm_head.float().t())
            top2 = logits.topk(2, dim=-1).values
            clear = (top2[:, 0] - top2[:, 1]) > 4e-2 * logits.abs().max()
            ta = logits.argmax(-1)
            assert torch.equal(tok_f.view(-1)[clear], ta[clear]), (batch, step)
            pos += 1
            mask[..., ctx + step + 1] = 0
        del ma, mb_
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------
# lean small-M kernels (r05, w4a16_lean.hpp): x by LDS-DMA first in the memory queue, every weight tile of a wave requested
# up front, unit sums and the RMSNorm sum of squares from the matrix core
# ------------------------------------------------------------------------------------------------
LEAN = 6


def lean(ntw, waves):
    return LEAN | (ntw << 4) | ((waves // 4) << 8)


LEAN_SHAPES = [(1, 1024, 256, 128), (3, 2048, 384, 128), (16, 1024, 128, 128), (5, 1536, 256, 256), (9, 4096, 512, 128), (2, 1152, 256, 384),
               (20, 1024, 256, 128), (4, 2176, 256, 128), (7, 8192, 256, 128), (1, 11008, 128, 128), (13, 1280, 1280, 128), (2, 8192, 256, 128),
               (4, 4096, 384, 256), (1, 5120, 256, 128), (3, 14336, 128, 128), (4, 7168, 256, 128)]


@pytest.mark.parametrize("ntw,waves", [(1, 8), (1, 16), (2, 8), (2, 16)])
@pytest.mark.parametrize("M,K,N,G", LEAN_SHAPES)
def test_lean_family_against_oracle(qa, device, M, K, N, G, ntw, waves):
    """Every build of the lean kernel on ragged k ranges (k tiles that do not divide by the waves, partly filled x segments), one and
    two token blocks, G = 128 / 256 / 384; the plain GEMM twice (bit-identical), bias + residual, SiLU * mul and the RMSNorm prologue."""
    from quick_amd import kernels as K_
    kid = lean(ntw, waves)
    if "tiles_per_wave<=0" in K_.plan_describe(M, K, N, G, kid):
        pytest.skip("no lean build for this k range / LDS footprint")
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G + waves)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    y = qa.gemm_forward(xd, *packed, kernel_id=kid)
    assert rel_err(y.cpu().numpy(), want) <= TOL
    assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=kid))
    bias = np.linspace(-1, 1, N).astype(np.float16)
    res = (np.random.default_rng(M + N).standard_normal((M, N)) * 0.5).astype(np.float16)
    y = qa.gemm_forward(xd, *packed, bias=_dev(bias, device), residual=_dev(res, device), kernel_id=kid)
    assert rel_err(y.cpu().numpy(), want + bias.astype(np.float32) + res.astype(np.float32)) <= TOL
    gu = torch.from_numpy(want).half().view(M, N // 16, 2, 8)                  # gate / up interleaved by 8
    ref = (torch.nn.functional.silu(gu[:, :, 0].float()).half() * gu[:, :, 1]).reshape(M, N // 2).float().numpy()
    y = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)
    assert tuple(y.shape) == (M, N // 2) and rel_err(y.cpu().numpy(), ref) <= 2 * TOL
    lnw = (torch.rand(K, device=device) + 0.5).half()
    x3 = xd * 3
    xn = (x3.float() * torch.rsqrt(x3.float().pow(2).mean(-1, keepdim=True) + 1e-5)).half() * lnw
    want_ln = oracle.w4a16_forward(xn.cpu().numpy(), iw, s, z, G).astype(np.float32) + res.astype(np.float32)
    y = qa.gemm_forward(x3, *packed, rmsnorm_weight=lnw, rmsnorm_eps=1e-5, residual=_dev(res, device), kernel_id=kid)
    assert rel_err(y.cpu().numpy(), want_ln) <= TOL


def test_lean_reference_pin_and_poisoned_output(qa, device, pin):
    """The reference-made 4096^2 pin through every lean build (sampled outputs of the REFERENCE's CPU path on the same layer), results
    into a NaN-poisoned buffer: every element of y is written, nothing next to it is."""
    from quick_amd import kernels as K_
    g, iw, s, z = pin
    packed = _pack_dev(iw, s, z, device)
    ref = g["y_ref"].astype(np.float32)
    x = _dev(g["x"], device)
    M, N = x.shape[0], packed[0].shape[1] // 4 * 8
    for kid in (lean(1, 8), lean(1, 16), lean(2, 8), lean(2, 16), 0):
        if "tiles_per_wave<=0" in K_.plan_describe(M, 4096, N, 128, kid):
            continue                                        # (16 tokens x 4096 k of x beside 16 waves' partials: beyond 160 KiB of LDS)
        out = torch.full((M + 2, N), float("nan"), dtype=torch.float16, device=device)
        y = qa.gemm_forward(x, *packed, kernel_id=kid, out=out[1:M + 1]).cpu().numpy().astype(np.float32)
        assert float(np.abs(y[g["y_rows"], g["y_cols"]] - ref).max()) <= TOL * float(np.abs(ref).max())
        assert float(np.abs(np.abs(y).sum(0) - g["col_abs_sum"]).max()) <= TOL * float(g["col_abs_sum"].max())
        assert torch.isnan(out[0]).all() and torch.isnan(out[M + 1]).all() and not torch.isnan(out[1:M + 1]).any()
    assert K_.plan_describe(1, 4096, 4096, 128).startswith("lean")


def test_workspace_check_detects_a_dirty_exchange_zone(qa, device):
    """The K slices of an exchange launch cannot tell a stale granule from a partner's partial sum (include/quick_amd.h,
    quick_w4a16_workspace_check): the contract is "all-zero between launches".  The check proves it after real launches, finds a planted
    granule, the Python layer zeroes the buffer again; with QUICK_AMD_CHECK_WORKSPACE=1 (own process: the switch is read once) a launch
    into a dirty workspace answers QUICK_ERR_WORKSPACE instead of computing with it."""
    import subprocess
    import sys
    from quick_amd import kernels as K_, packing
    M, K, N, G = 512, 1024, 512, 128
    assert "slices=2" in K_.plan_describe(M, K, N, G, 5 | (4 << 4) | (1 << 12) | (2 << 8))
    kid = 5 | (4 << 4) | (1 << 12) | (2 << 8)                      # xw 128 x 128, two slices
    gen = torch.Generator(device=device).manual_seed(5)
    qw, sc, qz = packing.random_mi355x(K, N, G, device, generator=gen)
    x = (torch.randn(M, K, device=device, generator=gen) * 0.5).half()
    y0 = qa.gemm_forward(x, qw, sc, qz, kernel_id=kid)
    assert K_.workspace_check(device)
    ws = K_._WORKSPACES[(device.index, torch.cuda.current_stream().cuda_stream)]
    ws[65536 + 4096 * 3 + 32:65536 + 4096 * 3 + 48] = 0x3c       # a granule nobody sent
    with pytest.raises(RuntimeError, match="not zero at byte 77856"):
        K_.workspace_check(device)
    assert K_.workspace_check(device)                              # ... zeroed again by the Python layer
    assert torch.equal(y0, qa.gemm_forward(x, qw, sc, qz, kernel_id=kid))
    ws[1000:1004] = 7                                              # a part state word
    with pytest.raises(RuntimeError, match="arrival counters"):
        K_.workspace_check(device)
    code = f"""
import torch, sys
sys.path.insert(0, {os.path.dirname(os.path.dirname(os.path.abspath(__file__)))!r})
import quick_amd
from quick_amd import kernels as K_, packing
dev = torch.device("cuda:0")
qw, sc, qz = packing.random_mi355x({K}, {N}, {G}, dev)
x = torch.randn({M}, {K}, device=dev).half()
y0 = quick_amd.gemm_forward(x, qw, sc, qz, kernel_id={kid})
ws = K_._WORKSPACES[(0, torch.cuda.current_stream().cuda_stream)]
ws[65536 + 64:65536 + 80] = 0x3c
try:
    quick_amd.gemm_forward(x, qw, sc, qz, kernel_id={kid})
    print("NO ERROR")
except RuntimeError as e:
    print("ERR", e)
y1 = quick_amd.gemm_forward(x, qw, sc, qz, kernel_id={kid})
print("EQUAL", bool(torch.equal(y0, y1)))
"""
    env = dict(os.environ, QUICK_AMD_CHECK_WORKSPACE="1")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, timeout=300)
    assert "ERR" in r.stdout and "not zero at byte 65600 (exchange zone)" in r.stdout and "EQUAL True" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("ntw,waves,slots", [(1, 8, 1), (2, 8, 1), (1, 8, 2)])
@pytest.mark.parametrize("M,K,N,G", [(1, 1024, 8320, 128), (4, 2048, 8448, 128), (16, 1024, 4224, 128), (9, 4096, 12288, 128), (3, 4096, 22016, 128),
                                     (2, 8192, 8448, 128)])
def test_lean_persistent_launches_equal_the_one_block_launches(qa, device, M, K, N, G, ntw, waves, slots):
    """Persistent lean launches (a workgroup walks several channel blocks; the next block's requests, invisible to hipcc's wait counting,
    are in flight under this block's tiles): bit-identical to the one-block-per-workgroup launch of the same build -- same arithmetic,
    block by block -- for the plain GEMM, bias + residual, SiLU * mul and the RMSNorm prologue; and the one-block launch against the oracle."""
    from quick_amd import kernels as K_
    one, per = lean(ntw, waves), lean(ntw, waves) | (slots << 22)
    p1, pp = K_.plan_describe(M, K, N, G, one), K_.plan_describe(M, K, N, G, per)
    if "tiles_per_wave<=0" in p1 or p1.split("grid=")[1].split()[0] == pp.split("grid=")[1].split()[0]:
        pytest.skip("no build, or nothing to walk (as many workgroups as blocks)")
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + waves)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    y1 = qa.gemm_forward(xd, *packed, kernel_id=one)
    cols = np.random.default_rng(N).choice(N, 512, replace=False)
    want = oracle.w4a16_forward(x, iw[:, cols], s[:, cols], z[:, cols], G).astype(np.float32)
    assert rel_err(y1.cpu().numpy()[:, cols], want) <= TOL
    for _ in range(3):
        assert torch.equal(y1, qa.gemm_forward(xd, *packed, kernel_id=per))
    bias = _dev(np.linspace(-1, 1, N).astype(np.float16), device)
    res = torch.randn(M, N, device=device).half()
    lnw = (torch.rand(K, device=device) + 0.5).half()
    for kw in (dict(bias=bias, residual=res), dict(silu_mul=True), dict(rmsnorm_weight=lnw, rmsnorm_eps=1e-5, residual=res)):
        assert torch.equal(qa.gemm_forward(xd, *packed, kernel_id=one, **kw), qa.gemm_forward(xd, *packed, kernel_id=per, **kw)), kw.keys()


# ------------------------------------------------------------------------------------------------
# [r06] mid-token kernels (w4a16_xm.hpp): 17..128 tokens, one workgroup per 32 / 64 tokens x 1..3 channel pairs, eight waves splitting K
# ------------------------------------------------------------------------------------------------
XM = 7


def xm(pr, tile=0):
    """pr channel pairs per workgroup; tile: 0 = by the token count, 64 / 32 = forced token tile"""
    return XM | (pr << 4) | ((2 << 8) if tile == 64 else 0) | ((1 << 8) if tile == 32 else 0)


XM_SHAPES = [(17, 1024, 256, 128), (33, 1024, 256, 128), (63, 1152, 384, 128), (64, 4096, 512, 128), (65, 1536, 256, 256), (127, 2048, 640, 128),
             (20, 2176, 128, 128), (50, 11008, 256, 128), (32, 8192, 256, 128), (48, 1024, 1280, 512)]


@pytest.mark.parametrize("tile", [32, 64])
@pytest.mark.parametrize("pr", [1, 2, 3])
@pytest.mark.parametrize("M,K,N,G", XM_SHAPES)
def test_xm_family_against_oracle(qa, device, M, K, N, G, pr, tile):
    """Every build of the mid-token kernel (32- / 64-token tiles x 1 / 2 / 3 channel pairs per workgroup): ragged token counts incl. the
    verdict's 17 / 33 / 63 / 65 / 127 (two token tiles), k tiles that do not divide by the eight waves (9, 12, 17, 86), a ragged last
    channel block (N / 32 not a multiple of the pairs), G = 256 / 512; against the oracle, three runs bit-identical, results into a
    NaN-poisoned buffer (every element of y written, nothing next to it), bias + residual, SiLU * mul; the RMSNorm prologue is refused."""
    from quick_amd import kernels as K_
    kid = xm(pr, tile)
    plan = K_.plan_describe(M, K, N, G, kid)
    assert plan.startswith(f"xm tokens={tile} channels={32 * pr}"), plan
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G + pr)
    want = oracle.w4a16_forward(x, iw, s, z, G).astype(np.float32)
    packed = _pack_dev(iw, s, z, device)
    xd = _dev(x, device)
    out = torch.full((M + 2, N), float("nan"), dtype=torch.float16, device=device)
    y = qa.gemm_forward(xd, *packed, kernel_id=kid, out=out[1:M + 1])
    assert rel_err(y.cpu().numpy(), want) <= TOL, plan
    assert torch.isnan(out[0]).all() and torch.isnan(out[M + 1]).all() and not torch.isnan(out[1:M + 1]).any()
    for _ in range(2):
        assert torch.equal(y, qa.gemm_forward(xd, *packed, kernel_id=kid)), plan
    bias = _dev(np.linspace(-1, 1, N).astype(np.float16), device)
    res = torch.randn(M, N, device=device).half()
    yb = qa.gemm_forward(xd, *packed, bias=bias, residual=res, kernel_id=kid)
    assert rel_err(yb.cpu().numpy(), want + bias.float().cpu().numpy() + res.float().cpu().numpy()) <= TOL, plan
    gu = torch.from_numpy(want).half().view(M, N // 16, 2, 8)                  # gate / up interleaved by 8
    ref = (torch.nn.functional.silu(gu[:, :, 0].float()).half() * gu[:, :, 1]).reshape(M, N // 2).float().numpy()
    ya = qa.gemm_forward(xd, *packed, silu_mul=True, kernel_id=kid)
    assert tuple(ya.shape) == (M, N // 2) and rel_err(ya.cpu().numpy(), ref) <= 2 * TOL, plan
    with pytest.raises(NotImplementedError):
        qa.gemm_forward(xd, *packed, kernel_id=kid, rmsnorm_weight=torch.ones(K, dtype=torch.float16, device=device))


@pytest.mark.parametrize("pr,tile", [(1, 32), (2, 32), (3, 64), (1, 64)])
def test_xm_golden_fixtures_reference_pin_and_exact_dequantisation(qa, device, pin, pr, tile):
    """The reference-made fixtures end to end (reference-format checkpoint -> HIP repack -> the mid-token kernels); the 4096 x 4096 pin of
    the reference packer / CPU path at 64 tokens (the fixture's 16 rows repeated), also through the planner's own pick; and one-hot
    activations: y[m] is then exactly one row of the dequantised matrix -- fp16((w - z) * s) bit for bit, the reference's per-weight arithmetic
    (csrc/gemm_cuda_quick.cu:52-60), whatever wave, stage and register it travelled through."""
    from quick_amd import kernels as K_
    kid = xm(pr, tile)
    for path in GOLD:
        g = load_golden(path)
        if int(g["G"]) % 128:
            continue                                    # (k tiles fewer than the waves: some waves add zeros)
        qw, qs, qz = qa.repack_cuda_to_mi355x(_dev(g["ref_qweight"], device), _dev(g["ref_qscales"], device), _dev(g["ref_qzeros"], device))
        y = qa.gemm_forward(_dev(g["x"], device), qw, qs, qz, kernel_id=kid)
        assert rel_err(y.cpu().numpy(), g["ref_y"]) <= TOL, path
    g, iw, s, z = pin
    packed = _pack_dev(iw, s, z, device)
    ref = g["y_ref"].astype(np.float32)
    M = 64
    x = np.tile(g["x"], (M // g["x"].shape[0], 1))
    assert K_.plan_describe(M, 4096, 4096, 128).startswith("xm tokens=32 channels=32")
    for k in (kid, 0):
        y = qa.gemm_forward(_dev(x, device), *packed, kernel_id=k).cpu().numpy().astype(np.float32)
        for rep in (0, M // 16 - 1):
            assert float(np.abs(y[g["y_rows"] + 16 * rep, g["y_cols"]] - ref).max()) <= TOL * float(np.abs(ref).max())
        assert float(np.abs(np.abs(y).sum(0) - g["col_abs_sum"] * (M // 16)).max()) <= TOL * float(g["col_abs_sum"].max()) * (M // 16)
    K, N, G = 2048, 384, 128
    _, iw2, s2, z2 = oracle.make_synthetic(1, K, N, G, seed=77)
    wd = oracle.dequantize(iw2, s2, z2, G)                      # fp16 [K, N]
    rows = np.random.default_rng(5).choice(K, 48, replace=False)
    xh = np.zeros((48, K), np.float16)
    xh[np.arange(48), rows] = 1.0
    y = qa.gemm_forward(_dev(xh, device), *_pack_dev(iw2, s2, z2, device), kernel_id=kid).cpu().numpy()
    assert np.array_equal(y.view(np.uint16), wd[rows].astype(np.float16).view(np.uint16))


def test_xm_planner_picks_against_oracle_on_layer_shapes(qa, device):
    """What AUTO runs at 17..128 tokens on the decode layer shapes (sampled channels against the oracle): the mid-token kernels where the audits
    have them ahead, the r03-r05 picks elsewhere -- every one right, and the picks are the ones profiles/r06_xm_audit.txt and
    r06_xm_audit_65_128.txt were measured with."""
    from quick_amd import kernels as K_
    G = 128
    seen = set()
    for (K, N) in ((4096, 4096), (4096, 12288), (4096, 22016), (4096, 6144), (8192, 8192), (11008, 4096), (5120, 5120), (4096, 28672), (4096, 8192), (8192, 4096)):
        _, iw, s, z = oracle.make_synthetic(1, K, N, G, seed=K + N)
        packed = _pack_dev(iw, s, z, device)
        cols = np.random.default_rng(N).choice(N, 256, replace=False)
        for M in (17, 32, 33, 48, 64, 65, 80, 95, 96, 113, 128):
            x = (np.random.default_rng(M).standard_normal((M, K)) * 0.5).astype(np.float16)
            want = oracle.w4a16_forward(x, iw[:, cols], s[:, cols], z[:, cols], G).astype(np.float32)
            y = qa.gemm_forward(_dev(x, device), *packed)
            assert rel_err(y.cpu().numpy()[:, cols], want) <= TOL, (M, K, N)
            seen.add(K_.plan_describe(M, K, N, G).split()[0] + (" 65+" if M > 64 else ""))
    assert "xm" in seen and "xm 65+" in seen and len(seen) >= 5
