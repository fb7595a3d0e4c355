"""Experiment: overlap the fixed cost of DEPENDENT small-M launches.  The weights of launch i + 1 do not depend on launch i --
only x does.  An experiment build of the lean kernels (tools/patches/lean_launch_overlap.patch as the patch argument of tools/build_variant.sh: tools/patches/README.md) lets a launch start without waiting for its
predecessor: it requests its weight tiles at entry, polls an arrival word the predecessor's storing waves raise behind their rows, then asks for x.
Here: the o_proj -> gate_up pair of a Llama-2-7B layer at one token (4096 x 4096 with the residual, then 4096 x 22016 with the RMSNorm prologue and
SiLU * mul), R pairs in one hipGraph, HBM-cold weight sets; `chain` = ordinary edges on one stream, `overlap` = every gate_up on a second stream forked
in front of its o_proj.  Gate: the pair <= 11.5 us in the chain with identical outputs.
    QUICK_AMD_LIB_OVERRIDE=tools/bin/ab_overlap.so python tools/launch_overlap.py"""
import ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from quick_amd import _lib, packing, kernels
lib = _lib.load()
assert hasattr(lib, "quick_amd_exp_lean_overlap"), "needs the build of tools/patches/lean_launch_overlap.patch (QUICK_AMD_LIB_OVERRIDE)"
lib.quick_amd_exp_lean_overlap.restype = None
lib.quick_amd_exp_lean_overlap.argtypes = [ctypes.c_void_p, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
dev = torch.device("cuda:0")
H, I, G = 4096, 11008, 128
NSETS = 12      # 12 x (8.4 + 45 MB) of weights: beyond the Infinity Cache
R = 48          # pairs per graph
o_sets = [packing.random_mi355x(H, H, G, dev) for _ in range(NSETS)]
gu_sets = [packing.random_mi355x(H, 2 * I, G, dev) for _ in range(NSETS)]
ln = (1.0 + 0.1 * torch.randn(H, device=dev)).half()
att = (torch.randn(1, H, device=dev) * 0.5).half()
print("plans:", kernels.plan_describe(1, H, H, G), "|", kernels.plan_describe(1, H, 2 * I, G))
o_waves = H // 16          # storing waves of the o_proj launch (lean ntw = 1: one per workgroup)


def run(mode):
    """-> (us per pair, list of act outputs of the last replay)"""
    gen = torch.Generator(device=dev).manual_seed(7)
    x2 = [(torch.randn(1, H, device=dev, generator=gen) * 0.5).half() for _ in range(R)]          # residual streams, one per pair, the same in every mode
    x2_0 = [t.clone() for t in x2]
    acts = [torch.empty(1, I, dtype=torch.float16, device=dev) for _ in range(R)]
    sig = torch.zeros(64, dtype=torch.int32, device=dev)
    cnt = torch.zeros(64, dtype=torch.int32, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()

    def pair(r):
        o, gu = o_sets[r % NSETS], gu_sets[r % NSETS]
        if mode.startswith("chain"):
            kernels.gemm_forward(att, *o, residual=x2[r], out=x2[r])
            kernels.gemm_forward(x2[r], *gu, rmsnorm_weight=ln, silu_mul=True, out=acts[r])
        elif mode.startswith("anyorder"):
            # ONE stream: gate_up's packet carries no barrier (hipExtAnyOrderLaunch) -- dispatched behind o_proj's workgroups, running beside them
            lib.quick_amd_exp_lean_overlap(None, 0, None, sig.data_ptr(), 0)
            kernels.gemm_forward(att, *o, residual=x2[r], out=x2[r])
            lib.quick_amd_exp_lean_overlap(sig.data_ptr(), o_waves, cnt.data_ptr(), None, 1)
            kernels.gemm_forward(x2[r], *gu, rmsnorm_weight=ln, silu_mul=True, out=acts[r])
        else:
            s2.wait_stream(s1)                                                   # fork: gate_up does not wait for o_proj
            lib.quick_amd_exp_lean_overlap(None, 0, None, sig.data_ptr(), 0)        # o_proj: raise the arrival word behind the rows
            kernels.gemm_forward(att, *o, residual=x2[r], out=x2[r])
            with torch.cuda.stream(s2):
                lib.quick_amd_exp_lean_overlap(sig.data_ptr(), o_waves, cnt.data_ptr(), None, 0)
                kernels.gemm_forward(x2[r], *gu, rmsnorm_weight=ln, silu_mul=True, out=acts[r])
            s1.wait_stream(s2)                                                   # join

    with torch.cuda.stream(s1):
        for r in range(2):
            pair(r)                                                              # (first launches outside the capture: attributes, workspaces)
    torch.cuda.synchronize()
    sig.zero_(); cnt.zero_()
    for t, t0 in zip(x2, x2_0):
        t.copy_(t0)
    eager = mode.endswith("-eager")
    if not eager:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s1):
            for r in range(R):
                pair(r)
    times = []
    for rep in range(12):
        for t, t0 in zip(x2, x2_0):
            t.copy_(t0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(s1):
            a.record()
            if eager:
                for r in range(R):
                    pair(r)
            else:
                g.replay()
            b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) * 1e3 / R)
    return float(np.median(times[2:])), [t.clone() for t in acts], times


base_us, base_acts, bt = run("chain")
print(f"chain   : {base_us:6.2f} us per o_proj -> gate_up pair   (replays: {' '.join(f'{t:.2f}' for t in bt)})")
best = None
for mode in ("chain-eager", "anyorder-eager", "anyorder", "overlap"):
    try:
        ov_us, ov_acts, ot = run(mode)
    except Exception as e:
        print(f"{mode:15s}: {type(e).__name__}: {str(e)[:200]}")
        continue
    same = all(torch.equal(a, b) for a, b in zip(base_acts, ov_acts))
    worst = max(float((a.float() - b.float()).abs().max()) for a, b in zip(base_acts, ov_acts))
    finite = all(torch.isfinite(a).all().item() for a in ov_acts)
    print(f"{mode:15s}: {ov_us:6.2f} us per pair   outputs identical to the chain's: {same} (max abs diff {worst:.3g})  finite: {finite}   (replays: {' '.join(f'{t:.2f}' for t in ot)})")
    if same and mode in ("anyorder", "overlap") and (best is None or ov_us < best):
        best = ov_us
print(f"gate (pair <= 11.5 us in a hipGraph chain with identical outputs): {'MET' if best is not None and best <= 11.5 else 'NOT met'} (best graph mode: {best})")
