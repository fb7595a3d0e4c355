"""The staggered two-slice launch of the four-wave 128 x 128 kernels (kernel-id bits 27-28 = d, w4a16_xw.hpp): each slice finishes the two
32-token blocks it does NOT own 2 d stages early, mails them from inside the K loop and goes on multiplying for its own blocks.  Needs an MI355X.

K ranges at KT = K / 128 k tiles: slice 0 phase 1 [0, KT/2 - d), slice 1 phase 1 [KT/2 + d, KT), phase 2 of both [KT/2 - d, KT/2 + d) --
slice 0 for blocks 0, 1 and slice 1 for blocks 2, 3 of every 128-token tile.  Each output is still the fp32 sum, in slice order, of two parts
rounded to fp16: the tolerance is the module-wide one of tests/test_gemm_gpu.py (summation order), and everything order-independent is bit-exact.
"""
import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

TOL = 2e-3                         # tests/test_gemm_gpu.py
XW = 5
XW128x128x2 = XW | (4 << 4) | (2 << 8) | (1 << 12)


def stag(d, poll=0):
    return XW128x128x2 | (d << 27) | (poll << 22)


def _dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _pack_dev(iw, s, z, device):
    return [_dev(a, device) for a in oracle.pack_mi355x(iw, s, z)]


@pytest.fixture(scope="module")
def qa(device):
    import quick_amd
    from quick_amd import _lib
    _lib.load()
    return quick_amd


def _plan(M, K, N, G, kid):
    from quick_amd import kernels
    return kernels.plan_describe(M, K, N, G, kid)


def _workspaces_clean():
    """arrival counters / state words (64 KiB) and the exchange zone (16 MiB) of every workspace the Python face holds"""
    from quick_amd import kernels
    return all(int(ws[: (64 << 10) + (16 << 20)].count_nonzero()) == 0 for ws in kernels._WORKSPACES.values())


@pytest.fixture(scope="module")
def layers(device):
    out = {}
    for K, N in ((4096, 4096), (11008, 4096)):
        x, iw, s, z = oracle.make_synthetic(513, K, N, 128, seed=K + N)
        out[(K, N)] = dict(x=x, iw=iw, s=s, z=z, wdeq=oracle.dequantize(iw, s, z, 128), packed=_pack_dev(iw, s, z, device))
    return out


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("M,K,N", [(512, 4096, 4096), (300, 4096, 4096), (509, 4096, 4096), (512, 11008, 4096)])
def test_staggered_launch_against_the_oracle(qa, device, layers, M, K, N, d):
    L = layers[(K, N)]
    plan = _plan(M, K, N, 128, stag(d))
    assert plan.startswith("xw tokens=128 channels=128 waves=4 ring=4 queue=4") and f" slices=2 " in plan and f" stagger={d} workspace=" in plan, plan
    x = L["x"][:M]
    want = oracle.gemm_fp32acc(x, L["wdeq"]).astype(np.float32)
    y = qa.gemm_forward(_dev(x, device), *L["packed"], kernel_id=stag(d), out=torch.full((M, N), float("nan"), dtype=torch.float16, device=device))
    torch.cuda.synchronize()
    err = float(np.abs(y.float().cpu().numpy() - want).max()) / float(np.abs(want).max())
    print(f"staggered d={d} {M}x{K}x{N}: max rel err {err:.3e}")
    assert err <= TOL
    assert _workspaces_clean()


@pytest.mark.parametrize("M,K,N", [(512, 4096, 4096), (512, 11008, 4096)])
def test_auto_against_the_oracle_where_it_staggers(qa, device, layers, M, K, N):
    """AUTO (kernel id 0) on the shapes its rule admits: the plan says so, and the result holds the same tolerance."""
    L = layers[(K, N)]
    plan = _plan(M, K, N, 128, 0)
    print(plan)
    x = L["x"][:M]
    want = oracle.gemm_fp32acc(x, L["wdeq"]).astype(np.float32)
    y = qa.gemm_forward(_dev(x, device), *L["packed"], out=torch.full((M, N), float("nan"), dtype=torch.float16, device=device))
    err = float(np.abs(y.float().cpu().numpy() - want).max()) / float(np.abs(want).max())
    print(f"auto {M}x{K}x{N}: max rel err {err:.3e}")
    assert err <= TOL
    if " stagger=" in plan:   # AUTO's pick IS the forced launch of the same d
        d = int(plan.split(" stagger=")[1].split()[0])
        assert torch.equal(y, qa.gemm_forward(_dev(x, device), *L["packed"], kernel_id=stag(d)))
    assert _workspaces_clean()


@pytest.mark.parametrize("d", [1, 2, 3])
@pytest.mark.parametrize("K", [4096, 11008])
def test_one_hot_rows_reproduce_the_dequantised_weights(qa, device, layers, K, d):
    """Row m of x is 1.0 at one k: y[m] is row k of the dequantised weights, bit for bit (the other slice's part is zero).  The k tiles: first
    and last of the layer and both sides of each boundary of the four ranges; m % len(tiles) picks the tile, so every 32-token block -- those
    a slice owns and those it mails -- meets every range."""
    N, KT = 4096, K // 128
    L = layers[(K, N)]
    h = KT // 2
    tiles = sorted({0, KT - 1, h - d - 1, h - d, h - 1, h, h + d - 1, h + d, 1, KT - 2})
    M = 512
    ks = np.array([tiles[m % len(tiles)] * 128 + (37 * m + 5) % 128 for m in range(M)])
    x = np.zeros((M, K), dtype=np.float16)
    x[np.arange(M), ks] = 1.0
    y = qa.gemm_forward(_dev(x, device), *L["packed"], kernel_id=stag(d), out=torch.full((M, N), float("nan"), dtype=torch.float16, device=device))
    got = y.cpu().numpy()
    want = L["wdeq"][ks, :]
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    assert _workspaces_clean()


@pytest.mark.parametrize("d", [1, 2, 3])
def test_power_of_two_scaling_is_exact_and_runs_are_bit_equal(qa, device, layers, d):
    L = layers[(4096, 4096)]
    xs = L["x"][:512].copy()
    xs[np.abs(xs) < 2.0 ** -13] = 2.0 ** -13          # (fp16 subnormals kept out of x, as test_baseline_power_of_two_scaling_is_exact_and_deterministic)
    x = _dev(xs, device)
    nan = lambda: torch.full((512, 4096), float("nan"), dtype=torch.float16, device=device)
    y1 = qa.gemm_forward(x, *L["packed"], kernel_id=stag(d), out=nan())
    for _ in range(3):
        assert torch.equal(qa.gemm_forward(x, *L["packed"], kernel_id=stag(d), out=nan()), y1)
    y2 = qa.gemm_forward(x * 2, *L["packed"], kernel_id=stag(d), out=nan())
    normal = y1.abs() >= 2.0 ** -13
    assert torch.equal(y2[normal], (y1 * 2)[normal])
    assert ((y2 - y1 * 2).abs() <= 2.0 ** -23)[~normal].all()
    assert torch.equal(qa.gemm_forward(torch.zeros_like(x), *L["packed"], kernel_id=stag(d), out=nan()), torch.zeros_like(y1))
    assert _workspaces_clean()


def test_give_up_paths_of_the_staggered_launch(qa, device, layers):
    """The method of test_xw_exchange_when_partners_are_not_there: a poll limit of 2 ticks (every wave that does not find its partner's part
    at its first look gives its block up) and of 2.5 us, alone and while a long kernel on a second stream holds most of the chip, and two
    staggered launches on two streams at once.  Every word equals the undisturbed staggered launch's, in NaN-poisoned outputs; the exchange zone
    and the state words are all-zero after every round."""
    cases = []
    for (M, K, N), d in (((512, 4096, 4096), 2), ((512, 4096, 4096), 1), ((512, 4096, 4096), 3), ((300, 11008, 4096), 2)):
        L = layers[(K, N)]
        xd = _dev(L["x"][:M], device)
        y0 = qa.gemm_forward(xd, *L["packed"], kernel_id=stag(d))
        cases.append((xd, L["packed"], d, y0))
    torch.cuda.synchronize()
    assert _workspaces_clean()
    side = torch.cuda.Stream()
    big = torch.randn(8192, 8192, device=device).half()
    for rep in range(4):
        for held in (False, True):
            if held:
                with torch.cuda.stream(side):
                    torch.matmul(big, big)
            for xd, packed, d, y0 in cases:
                for poll in (0, 1, 8):
                    y = qa.gemm_forward(xd, *packed, kernel_id=stag(d, poll), out=torch.full_like(y0, float("nan")))
                    assert torch.equal(y, y0), (rep, held, d, poll)
            torch.cuda.synchronize()
            assert _workspaces_clean(), (rep, held)
        xa, pa, da, ya = cases[rep % len(cases)]
        xb, pb, db, yb = cases[(rep + 1) % len(cases)]
        with torch.cuda.stream(side):
            outs_b = [qa.gemm_forward(xb, *pb, kernel_id=stag(db, 8 if rep % 2 else 0), out=torch.full_like(yb, float("nan"))) for _ in range(4)]
        outs_a = [qa.gemm_forward(xa, *pa, kernel_id=stag(da, 8 if rep % 2 else 0), out=torch.full_like(ya, float("nan"))) for _ in range(4)]
        torch.cuda.synchronize()
        assert all(torch.equal(o, ya) for o in outs_a) and all(torch.equal(o, yb) for o in outs_b), rep
        assert _workspaces_clean(), rep


@pytest.mark.parametrize("M,K,N,G,kid,why", [
    (512, 1024, 4096, 128, stag(1), "phase 1 of 3 stages is shorter than the ring of four"),
    (512, 1280, 4096, 128, stag(2), "phase 1 of 3 stages is shorter than the ring of four"),
    (512, 4096, 4096, 128, XW | (4 << 4) | (2 << 8) | (2 << 27), "128 x 256 tiles"),
    (256, 4096, 4096, 128, XW | (4 << 4) | (4 << 8) | (1 << 12) | (2 << 27), "four slices"),
    (512, 4096, 4096, 128, XW | (4 << 4) | (1 << 8) | (1 << 12) | (2 << 27), "one slice"),
    (256, 4096, 4096, 128, XW | (2 << 4) | (2 << 8) | (2 << 27), "64 x 128 tiles"),
    (512, 4096, 4096, 256, stag(2), "group size 256"),
    (512, 4224, 4096, 128, stag(2), "an odd number of k tiles"),
    (513, 4096, 4096, 128, stag(2), "160 tiles: two slices each do not fit the 256 workgroups of an exchange launch, one slice"),
])
def test_a_forced_stagger_the_variant_cannot_run_is_planned_without_it(qa, device, M, K, N, G, kid, why):
    """... and then runs exactly the launch of the same id without the bits."""
    plain = kid & ~(3 << 27)
    assert "stagger" not in _plan(M, K, N, G, kid), why
    assert _plan(M, K, N, G, kid) == _plan(M, K, N, G, plain), why
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=K + G)
    xd, packed = _dev(x, device), _pack_dev(iw, s, z, device)
    assert torch.equal(qa.gemm_forward(xd, *packed, kernel_id=kid), qa.gemm_forward(xd, *packed, kernel_id=plain)), why
    assert _workspaces_clean()
