"""quick_w4a16_gemm_span (in-kernel span stamps, include/quick_amd.h) through every launcher's span selection.  Needs an MI355X.

A kernel either has a span-stamped twin -- then the span launch computes, bit for bit, what the plain launch computes, and reports a span --
or it has none -- then the launcher refuses before anything is launched (QUICK_ERR_UNSUPPORTED, y untouched) and the refusal leaves nothing
behind for the next launch of the thread.  Every row forces one kernel with a kernel id and asserts what the planner says it runs, so a
planner change cannot silently move a row to another kernel.  Shapes: the smallest K, N in 256..1024 at which the planner runs the named
kernel (the straight-line fragment kernels need K / 128 == 8 waves x T k tiles; the staggered launch K / 256 - d >= 4).
Every stamped row is held to bit equality, the rows whose K slices meet through the workspace (xk / xw with two slices) included: at these
shapes they repeat bit for bit.
"""
import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import oracle
from conftest import rel_err

pytestmark = pytest.mark.gpu

TOL = 2e-3                 # (tests/test_gemm_gpu.py: fp32 accumulation, one final rounding; only the summation order differs)
OK, UNSUPPORTED = 0, 4
ITERS = 2
SENTINEL = 7.0
SKINNY, TILED, WIDE, XK, XW, LEAN, XM = 1, 2, 3, 4, 5, 6, 7
SK1 = SKINNY | (1 << 4)                                  # one channel tile per workgroup
NO_XLDS, EXACT, TABLE = 1 << 12, 1 << 25, 1 << 26        # SKINNY bits
RING64 = WIDE | (2 << 4) | (1 << 8)                      # 64 x 128 tiles
XW128 = XW | (4 << 4) | (1 << 12)                        # 128 x 128 tiles


def waves(n):
    return (n // 4) << 8


def slices(n):
    return n << 8


# (name, kernel id, M, K, N, G, what plan_describe must say)
STAMPED = [
    ("lean_1_token", LEAN, 1, 1024, 256, 128, r"^lean ntw=1 waves=8 tiles_per_wave<=4 "),
    ("skinny_8_waves_table_1_token", SK1 | waves(8) | TABLE, 1, 256, 256, 128, r"^skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table .* ksplit=1 "),
    ("skinny_exact_no_lds_copy_8_tokens", SK1 | waves(8) | NO_XLDS | EXACT, 8, 256, 256, 128, r"^skinny ntw=1 waves=8 x=l2 dequant=exact .* ksplit=1 "),
    ("skinny_4_tiles_fragment_64_tokens", SKINNY | (4 << 4) | waves(8), 64, 256, 256, 128, r"^skinny ntw=4 waves=8 x=l2 dequant=deferred-zero-fragment .* ksplit=1 "),
    ("skinny_16_waves_table", SK1 | waves(16) | TABLE, 1, 256, 256, 128, r"^skinny ntw=1 waves=16 x=lds dequant=deferred-zero-table .* ksplit=1 "),
    ("skinny_16_waves_exact", SK1 | waves(16) | NO_XLDS | EXACT, 1, 256, 256, 128, r"^skinny ntw=1 waves=16 x=l2 dequant=exact .* ksplit=1 "),
    ("fragment_8_tiles", SKINNY | (8 << 4), 16, 2048, 256, 128, r"^skinny ntw=8 waves=8 x=l2 dequant=deferred-zero-fragment grid=2x1x1 ksplit=1 "),
    ("fragment_7_tiles", SKINNY | (7 << 4), 16, 8192, 896, 128, r"^skinny ntw=7 waves=8 x=l2 dequant=deferred-zero-fragment grid=8x1x1 ksplit=1 "),
    ("ring_64x128_4_waves_6_slots", RING64, 64, 256, 256, 128, r"^wide tokens=64 channels=128 waves=4 ring=6 "),
    ("ring_64x128_8_waves_4_slots", RING64 | (1 << 15) | (4 << 22), 64, 256, 256, 128, r"^wide tokens=64 channels=128 waves=8 ring=4 "),
    ("xk_64_tokens_1_slice", XK | (2 << 4) | slices(1), 64, 256, 256, 128, r"^xk tokens=64 channels=128 waves=8 ring=5 queue=4 grid=2 slices=1 "),
    ("xk_64_tokens_2_slices", XK | (2 << 4) | slices(2), 64, 256, 256, 128, r"^xk tokens=64 channels=128 waves=8 ring=5 queue=4 grid=4 slices=2 "),
    ("xk_128_tokens_1_slice", XK | (4 << 4) | slices(1), 128, 256, 256, 128, r"^xk tokens=128 channels=128 waves=8 ring=5 queue=4 grid=2 slices=1 "),
    ("xk_128_tokens_2_slices", XK | (4 << 4) | slices(2), 128, 256, 256, 128, r"^xk tokens=128 channels=128 waves=8 ring=5 queue=4 grid=4 slices=2 "),
    ("xw_64x128_1_slice", XW | (2 << 4) | slices(1), 64, 256, 256, 128, r"^xw tokens=64 channels=128 waves=4 .* grid=2 slices=1 xcd_rows=\d+ workspace"),
    ("xw_64x128_2_slices", XW | (2 << 4) | slices(2), 64, 256, 256, 128, r"^xw tokens=64 channels=128 waves=4 .* grid=4 slices=2 xcd_rows=\d+ workspace"),
    ("xw_128x128_1_slice", XW128 | slices(1), 128, 256, 256, 128, r"^xw tokens=128 channels=128 waves=4 .* grid=2 slices=1 xcd_rows=\d+ workspace"),
    ("xw_128x128_2_slices", XW128 | slices(2), 128, 256, 256, 128, r"^xw tokens=128 channels=128 waves=4 .* grid=4 slices=2 xcd_rows=\d+ workspace"),
    ("xw_128x128_2_slices_staggered", XW128 | slices(2) | (1 << 27), 128, 1280, 256, 128, r"^xw tokens=128 channels=128 waves=4 .* grid=4 slices=2 xcd_rows=\d+ stagger=1 "),
    ("xm_32_token_tiles", XM | (1 << 8), 32, 256, 256, 128, r"^xm tokens=32 "),
    ("xm_64_token_tiles", XM | (2 << 8), 64, 256, 256, 128, r"^xm tokens=64 "),
]
UNSTAMPED = [
    ("tiled", TILED, 64, 256, 256, 128, r"^tiled "),
    ("wide_no_ring", RING64 | (1 << 12), 64, 256, 256, 128, r"^wide tokens=64 channels=128 waves=4 ring=0 "),
    ("ring_G_256", RING64, 64, 256, 256, 256, r"^wide tokens=64 channels=128 waves=4 ring=6 "),
    ("skinny_G_64", SK1 | waves(8) | TABLE, 1, 256, 256, 64, r"^skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table "),
    ("skinny_4_waves", SK1 | waves(4), 1, 256, 256, 128, r"^skinny ntw=1 waves=4 "),
    ("skinny_2_tiles", SKINNY | (2 << 4), 1, 256, 256, 128, r"^skinny ntw=2 "),
]


@functools.lru_cache(maxsize=None)
def _layer(M, K, N, G):
    """inputs, packed weights and the oracle's answer for a shape: computed once, shared by the rows of that shape, never written"""
    x, iw, s, z = oracle.make_synthetic(M, K, N, G, seed=M + K + N + G)
    return x, oracle.pack_mi355x(iw, s, z), oracle.w4a16_forward(x, iw, s, z, G)


class _Bench:
    def __init__(self, device):
        from quick_amd import _lib
        self.lib, self.last_error, self.device = _lib.load(), _lib.last_error, device
        self.ws = torch.zeros(32 << 20, dtype=torch.uint8, device=device)
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def tensors(self, M, K, N, G):
        x, packed, want = _layer(M, K, N, G)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)
        return dev(x), [dev(a) for a in packed], want

    def span(self, x, packed, y, M, K, N, G, kid):
        ptr = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())
        us = (ctypes.c_float * ITERS)()
        rc = self.lib.quick_w4a16_gemm_span(x.data_ptr(), ptr(packed[0]), ptr(packed[1]), ptr(packed[2]), 1, y.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                            M, K, N, G, kid, 0, ITERS, us, self.stream)
        torch.cuda.synchronize()
        return rc, list(us)

    def plain(self, x, packed, y, M, K, N, G, kid):
        rc = self.lib.quick_w4a16_gemm_f16_ex(x.data_ptr(), packed[0].data_ptr(), packed[1].data_ptr(), packed[2].data_ptr(), None, y.data_ptr(),
                                              self.ws.data_ptr(), self.ws.numel(), M, K, N, G, kid, 0, self.stream)
        torch.cuda.synchronize()
        return rc

    def workspace_clean(self):
        return self.lib.quick_w4a16_workspace_check(self.ws.data_ptr(), self.ws.numel(), self.stream) == OK


@pytest.fixture(scope="module")
def bench(device):
    return _Bench(device)


def _planned(M, K, N, G, kid, says):
    from quick_amd import kernels
    text = kernels.plan_describe(M, K, N, G, kid)
    assert re.search(says, text), text
    return text


@pytest.mark.parametrize("name,kid,M,K,N,G,says", STAMPED, ids=[r[0] for r in STAMPED])
def test_span_launch_of_a_stamped_kernel_equals_the_plain_launch(bench, name, kid, M, K, N, G, says):
    text = _planned(M, K, N, G, kid, says)
    x, packed, _ = bench.tensors(M, K, N, G)
    y_span = torch.full((M, N), float("nan"), dtype=torch.float16, device=bench.device)
    y_plain = torch.full((M, N), float("nan"), dtype=torch.float16, device=bench.device)
    rc, us = bench.span(x, packed, y_span, M, K, N, G, kid)
    assert rc == OK, (text, rc, bench.last_error())
    print(name, "span us:", us)
    assert all(np.isfinite(u) and u > 0 for u in us), us
    assert bench.plain(x, packed, y_plain, M, K, N, G, kid) == OK, bench.last_error()
    assert not torch.isnan(y_span).any() and torch.equal(y_span, y_plain), (text, rel_err(y_span.cpu().numpy(), y_plain.cpu().numpy().astype(np.float32)))
    assert bench.workspace_clean(), bench.last_error()


@pytest.mark.parametrize("name,kid,M,K,N,G,says", UNSTAMPED, ids=[r[0] for r in UNSTAMPED])
def test_span_launch_of_a_kernel_without_stamps_is_refused_and_leaves_nothing_behind(bench, name, kid, M, K, N, G, says):
    text = _planned(M, K, N, G, kid, says)
    x, packed, want = bench.tensors(M, K, N, G)
    y = torch.full((M, N), SENTINEL, dtype=torch.float16, device=bench.device)
    rc, us = bench.span(x, packed, y, M, K, N, G, kid)
    assert rc == UNSUPPORTED and "no span-stamped build" in bench.last_error(), (text, rc, bench.last_error())
    assert bool((y == SENTINEL).all()), text          # a refused launcher launches nothing
    assert bench.workspace_clean(), bench.last_error()
    # the refusal does not outlive the call: the plain launch of the same shape, same thread, right behind it runs and is right
    assert bench.plain(x, packed, y, M, K, N, G, kid) == OK, bench.last_error()
    assert rel_err(y.cpu().numpy(), want) <= TOL, text
