"""Load-time cost of the format bridges: `repack_awq_gemm_to_mi355x` (GEMM packing, staged through LDS) next to the existing
`repack_cuda_to_mi355x` (QUICK packing, one gather thread per output dword) on the same layer shapes.  Event pairs around each
call (all launches of a conversion), median of 20 after 3 warm-up calls.  Run on the GPU box:

    timeout -k 10 300 python tools/repack_bench.py > profiles/awq_gemm_repack.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quick_amd import kernels  # noqa: E402


def _time(fn, args, warmup=3, runs=20):
    for _ in range(warmup):
        fn(*args)
    torch.cuda.synchronize()
    us = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(*args)
        b.record()
        b.synchronize()
        us.append(a.elapsed_time(b) * 1e3)
    return statistics.median(us), min(us), max(us)


def main():
    dev = torch.device("cuda:0")
    print(f"# {torch.cuda.get_device_name(0)}, torch {torch.__version__}; median (min .. max) of 20 calls in us, 3 warm-up calls;")
    print("# each call allocates its three outputs (torch caching allocator) and enqueues every launch of the conversion")
    rnd = lambda *shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev)
    G = 128
    for K, N in ((4096, 11008), (8192, 28672)):
        gemm = (rnd(K, N // 8), rnd(K // G, N // 8), torch.rand((K // G, N), device=dev).half())
        quick = (rnd(K // 4, N // 2), torch.rand((K // G, 2 * N), device=dev).half(), rnd(K // G, N // 4))
        mbytes = K * N / 2 / 1e6
        rows = []
        for name, fn, args in (("repack_awq_gemm_to_mi355x", kernels.repack_awq_gemm_to_mi355x, gemm),
                               ("repack_cuda_to_mi355x", kernels.repack_cuda_to_mi355x, quick)):
            med, lo, hi = _time(fn, args)
            rows.append(med)
            print(f"K={K} N={N} G={G}  {name:<28} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})  "
                  f"{2 * mbytes / med * 1e-3:7.1f} GB/s of weight traffic (read + write {2 * mbytes:.0f} MB)")
        print(f"K={K} N={N} G={G}  new / existing = {rows[0] / rows[1]:.2f}"
              + ("   <-- the staged kernel is SLOWER than the gather kernel here" if rows[0] > rows[1] else ""))
        del gemm, quick
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
