"""The gate / up interleave kernels' lane function on the CPU, under the address and undefined-behaviour sanitizers, against
packing.py's restatement bit for bit.  Builds tools/gate_up_host_check.cpp (a stand-alone program: nothing is loaded into Python) with the
ROCm clang and runs it on the five (K, I, G) cases of tests/test_gate_up_cpu.py plus one with 64 k tiles.  No GPU.

    python tools/gate_up_host_check.py
"""
import os
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from quick_amd import packing  # noqa: E402

CASES = [(128, 64, 128), (256, 192, 64), (384, 64, 32), (512, 320, 128), (256, 384, 128), (8192, 64, 128)]


def _clang():
    for c in (os.environ.get("CXX"), "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no clang++ found (looked at $CXX and under /opt/rocm)")


def _projection(K, I, G, gen):
    """Random MI355X-order tensors of one projection (any I % 16 == 0: random_mi355x needs no N % 128)."""
    return packing.random_mi355x(K, I, G, "cpu", generator=gen)


def main():
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "gate_up_host_check")
        subprocess.run([_clang(), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "gate_up_host_check.cpp"), "-o", exe], check=True)
        gen = torch.Generator().manual_seed(5)
        for K, I, G in CASES:
            gate, up = _projection(K, I, G, gen), _projection(K, I, G, gen)
            fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
            with open(fin, "wb") as f:
                for t in gate + up:
                    f.write(t.contiguous().numpy().tobytes())
            subprocess.run([exe, str(K), str(I), str(G), fin, fout], check=True)
            fused = packing.interleave_gate_up_mi355x(gate, up)
            want = b"".join(t.contiguous().numpy().tobytes() for t in fused + gate + up)
            got = open(fout, "rb").read()
            assert got == want, f"K={K} I={I} G={G}: first differing byte {next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)}"
            print(f"K={K} I={I} G={G}: {len(got)} bytes identical to the restatement, sanitizers silent")


if __name__ == "__main__":
    main()
