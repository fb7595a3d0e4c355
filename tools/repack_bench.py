"""Load-time cost of the format bridges: `repack_awq_gemm_to_mi355x` (GEMM packing, staged through LDS) next to the existing
`repack_cuda_to_mi355x` (QUICK packing, one gather thread per output dword) on the same layer shapes.  Event pairs around each
call (all launches of a conversion), median of 20 after 3 warm-up calls.  Then the gate / up interleave and split kernels
(`interleave_gate_up_mi355x`, `split_gate_up_mi355x`: one launch, whole 16-byte pieces) on the MLP of the same sizes, each beside
`repack_cuda_to_mi355x` of ONE projection of that layer from the same run -- which moves about half the bytes, so the comparison is per
byte.  Run on the GPU box:

    timeout -k 10 300 python tools/repack_bench.py > profiles/gate_up_interleave.txt
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from quick_amd import kernels, packing  # noqa: E402


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
    print("#")
    print("# gate / up interleave: K x I per projection; bytes = read + write of all three tensors; ratio = (us per byte) / (us per byte of")
    print("# repack_cuda_to_mi355x on one projection in this run); spread = (max - min) / median of the 20 calls")
    for K, I in ((4096, 11008), (8192, 28672)):
        gate, up = packing.random_mi355x(K, I, G, dev), packing.random_mi355x(K, I, G, dev)
        fused = kernels.interleave_gate_up_mi355x(gate, up)
        one = sum(t.numel() * t.element_size() for t in gate)          # bytes of one projection's three tensors
        ref_med, ref_lo, ref_hi = _time(kernels.repack_cuda_to_mi355x, gate)   # (its input order does not matter to its cost: a gather per dword)
        ref_spread = (ref_hi - ref_lo) / ref_med
        print(f"K={K} I={I} G={G}  {'repack_cuda_to_mi355x (1 proj)':<32} {ref_med:9.1f} us  ({ref_lo:.1f} .. {ref_hi:.1f})  "
              f"{2 * one / 1e6:7.1f} MB  {2 * one / ref_med * 1e-3:7.1f} GB/s  spread {ref_spread:.2f}")
        for name, fn, args in (("interleave_gate_up_mi355x", kernels.interleave_gate_up_mi355x, (gate, up)),
                               ("split_gate_up_mi355x", kernels.split_gate_up_mi355x, fused)):
            med, lo, hi = _time(fn, args)
            ratio = (med / (4 * one)) / (ref_med / (2 * one))
            spread = max((hi - lo) / med, ref_spread)
            note = "   <-- SLOWER per byte than the existing repack beyond the run's spread" if ratio > 1 + spread else ""
            print(f"K={K} I={I} G={G}  {name:<32} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})  {4 * one / 1e6:7.1f} MB  "
                  f"{4 * one / med * 1e-3:7.1f} GB/s  per-byte ratio to the repack {ratio:.2f}{note}")
        del gate, up, fused
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
