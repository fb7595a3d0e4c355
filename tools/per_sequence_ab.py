"""Per-sequence attention launches against the shared ones, and this tree's shared launches against the parent commit's, on the same box
in the same session, the variants alternating inside one process per shape:

    parent      the shared entry of the PARENT commit's library (--parent: a libquick_amd.so built from the parent's tree), twice per round:
                the ratio of its two medians is the spread the box shows against itself
    shared      the shared entry of this tree's library
    seq-equal   the per-sequence entry with every position equal to the shared one
    seq-mixed   the per-sequence entry with positions drawn uniformly over 1 .. L - 1 (decode) or 0 .. L - T (prefill)
    longest     the shared entry at the largest of those positions: what the mixed batch cost as a padded batch

Decode: quick_decode_rope_attention(_seq)_f16 at the shapes of profiles/r05_attention.txt, a cache of 1024 rows, positions 192 and 512.
Prefill: quick_rope_kv_write(_seq)_f16 + quick_prefill_attention(_seq)_f16 at the shapes of profiles/prefill_attention.txt.  Every variant
is a captured graph of 5 passes over 4 cache sets (HBM-cold like a model's layers); a sample is an event pair around two replays; the
table gives the median of 15 samples in us per launch (decode) or per pair of launches (prefill).

    timeout -k 10 1100 python tools/per_sequence_ab.py --parent /path/to/parent/libquick_amd.so --out profiles/per_sequence_attention.txt
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, L_DEC = 128, 1024
# (name, query heads, KV heads, B)
DECODE = [("Llama-2-7B 32/32", 32, 32, 1), ("Llama-2-7B 32/32", 32, 32, 64), ("Mistral-7B 32/8", 32, 8, 64), ("Llama-2-70B 64/8", 64, 8, 16)]
DECODE_POS = (192, 512)
# (name, query heads, KV heads, B, T, pos0)
PREFILL = [(n, nh, nkv, B, T, p0) for n, nh, nkv, B, T in
           [("Llama-2-7B 32/32", 32, 32, 1, 128), ("Llama-2-7B 32/32", 32, 32, 64, 128), ("Llama-2-7B 32/32", 32, 32, 1, 2048),
            ("Mistral-7B 32/8", 32, 8, 64, 128), ("Llama-2-70B 64/8", 64, 8, 16, 128)] for p0 in (0, 512)]
CASES = [("decode",) + s + (p,) for s in DECODE for p in DECODE_POS] + [("prefill",) + s for s in PREFILL]
SETS, PASSES, ROUNDS = 4, 5, 15
CHILD_LIMIT = 150      # seconds per shape


def _parent_lib(path):
    from quick_amd import _lib
    lib = ctypes.CDLL(path)
    for name in ("quick_decode_rope_attention_f16", "quick_rope_kv_write_f16", "quick_prefill_attention_f16"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib._SIGNATURES[name]
    return lib


def _case(index, parent_path):
    import torch
    from quick_amd import _lib
    tree = _lib.load()
    parent = _parent_lib(parent_path) if parent_path else None
    kind, name, nh, nkv, B = CASES[index][:5]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(index)
    if kind == "decode":
        p, T, L = CASES[index][5], 1, L_DEC
        lo, hi = 1, L - 1
    else:
        T, p = CASES[index][5:7]
        L = 512 + T
        lo, hi = 0, L - T
    ang = torch.outer(torch.arange(L, device=dev).float(), 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=dev).half()
    kc = [torch.randn(B, nkv, L, D, generator=g, device=dev).half() for _ in range(SETS)]
    vc = [torch.randn(B, nkv, L, D, generator=g, device=dev).half() for _ in range(SETS)]
    q = torch.empty((B, nh, T, D), dtype=torch.float16, device=dev)
    out = torch.empty((B * T, nh * D), dtype=torch.float16, device=dev)
    one = torch.full((1,), p, dtype=torch.int64, device=dev)
    equal = torch.full((B,), p, dtype=torch.int64, device=dev)
    mixed = torch.randint(lo, hi + 1, (B,), generator=g, device=dev)
    longest = mixed.max().reshape(1).clone()
    scale = D ** -0.5

    def launcher(lib, seq, pos):
        suffix = "_seq_f16" if seq else "_f16"
        if kind == "decode":
            fn = getattr(lib, "quick_decode_rope_attention" + suffix)

            def run(i):
                rc = fn(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), kc[i].data_ptr(), vc[i].data_ptr(), out.data_ptr(), B, nh,
                        nkv, D, L, scale, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
        else:
            write, attend = getattr(lib, "quick_rope_kv_write" + suffix), getattr(lib, "quick_prefill_attention" + suffix)

            def run(i):
                st = torch.cuda.current_stream().cuda_stream
                rc = write(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), q.data_ptr(), kc[i].data_ptr(), vc[i].data_ptr(), B, T,
                           nh, nkv, D, L, st)
                rc = rc or attend(q.data_ptr(), kc[i].data_ptr(), vc[i].data_ptr(), pos.data_ptr(), out.data_ptr(), B, T, nh, nkv, D, L, scale, st)
                assert rc == 0, rc
        for i in range(SETS):
            run(i)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(PASSES):
                for i in range(SETS):
                    run(i)
        graph.replay()
        torch.cuda.synchronize()
        return graph

    variants = {}
    if parent is not None:
        variants["parent"] = variants["parent again"] = launcher(parent, False, one)
    variants["shared"] = launcher(tree, False, one)
    variants["seq-equal"] = launcher(tree, True, equal)
    same = out.clone()
    variants["shared"].replay()
    torch.cuda.synchronize()
    assert torch.equal(same.view(torch.int16), out.view(torch.int16)), "seq-equal and shared differ"
    variants["seq-mixed"] = launcher(tree, True, mixed)
    variants["longest"] = launcher(tree, False, longest)

    def timed(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        graph.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / (2 * PASSES * SETS)

    samples = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for k, graph in variants.items():
            samples[k].append(timed(graph))
    med = {k: statistics.median(v) for k, v in samples.items()}
    where = f"pos={p}" if kind == "decode" else f"T={T} pos0={p}"
    text = f"{kind:<7} {name:<17} B={B:<3} {where:<16}"
    if parent is not None:
        lo_p, hi_p = sorted((med["parent"], med["parent again"]))
        spread = hi_p / lo_p
        text += f" parent {med['parent']:8.2f} / {med['parent again']:8.2f} us  spread {spread:.3f}  shared {med['shared']:8.2f}  shared/parent {med['shared'] / lo_p:.3f}"
        text += "   <-- SLOWER than the parent beyond its spread" if med["shared"] / lo_p > spread else ""
    else:
        text += f" shared {med['shared']:8.2f} us"
    text += (f"  | seq-equal {med['seq-equal']:8.2f}  seq-equal/shared {med['seq-equal'] / med['shared']:.3f}"
             f"  | seq-mixed {med['seq-mixed']:8.2f}  longest({int(longest)}) {med['longest']:8.2f}  mixed/longest {med['seq-mixed'] / med['longest']:.3f}"
             f"  mean pos {float(mixed.float().mean()):.0f}")
    print(text, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--parent", default=None, help="libquick_amd.so built from the parent commit (omitted: no parent columns)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "per_sequence_attention.txt"))
    args = ap.parse_args()
    if args.case is not None:
        return _case(args.case, args.parent)
    lines = ["# per-sequence attention launches: us per launch (decode) or per rope_kv_write + prefill_attention pair (prefill); medians of",
             f"# {ROUNDS} samples, a sample = an event pair around two replays of a graph of {PASSES} passes over {SETS} cache sets; the variants",
             "# alternate inside one process per shape.  parent = the parent commit's library, measured twice per round (spread = its two",
             "# medians against each other); shared / seq-equal / seq-mixed / longest: see tools/per_sequence_ab.py"]
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        clocks = [ln.strip() for ln in smi.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
        lines.append("# clocks (rocm-smi --showclocks, GPU 0, before the run): " + ("; ".join(clocks) if clocks else "not reported"))
    except (OSError, subprocess.TimeoutExpired):
        lines.append("# clocks: rocm-smi not available")
    print("\n".join(lines), flush=True)
    head, ok = len(lines), True
    for i in range(len(CASES)):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--case", str(i)]
        r = subprocess.run(cmd + (["--parent", args.parent] if args.parent else []), capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"# case {i} {CASES[i]} ended with status {r.returncode}: the run stops here\n# " + r.stderr.strip().replace("\n", "\n# ")[-2000:])
            print(lines[-1], flush=True)
            ok = False
            break
        lines.append(r.stdout.strip())
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok and len(lines) == head + len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main())
