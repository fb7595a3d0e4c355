"""The one-byte (e4m3) KV cache launches against the fp16 launches of the PARENT commit's library, on the same box in the same session,
the routes alternating inside one process per shape (the method of tools/per_sequence_ab.py):

    parent      the fp16 entry of the parent commit's library (--parent: a libquick_amd.so built from the parent's tree), twice per round:
                the ratio of its two medians is the spread the box shows against itself
    fp16        the fp16 entry of this tree's library (the same sources: it should sit inside that spread)
    fp8         the fp8 entry of this tree's library on byte caches of the same shape

Decode: quick_decode_rope_attention_f16 / _fp8 at positions 256, 1024 and 2048 (a cache of pos + 128 rows).  Prefill: quick_rope_kv_write +
quick_prefill_attention, f16 / fp8, chunks of 128 tokens at pos0 = 0 and 1024.  Every variant is a captured graph of 5 passes over 4 cache
sets (HBM-cold like a model's layers); a sample is an event pair around two replays; the table gives the median of 15 samples in us per
launch (decode) or per pair of launches (prefill).  Halving the bytes predicts fp8/parent -> 0.5 where the fp16 launch is bound by cache
traffic and ~1 where it is bound by latency (bs 1) or by the MFMA products (prefill).

--accuracy (one more child process) records one accuracy figure: the module test's stack (hidden 512, 4 query / 2 KV heads,
quantize_linear-made projections) on N(0, 1) activations, a 48-token prefill and 16 decode steps, B = 2: the largest and the RMS
difference of the attention output (in front of o_proj) between the fp8 and the fp16 cache, relative to the output's RMS, at scale 1.0 and
at a scale set from the observed absolute maximum of the fp16 caches (absmax / 448).  Informative, not a gate.

    timeout -k 10 1100 python tools/fp8_kv_ab.py --parent /path/to/parent/libquick_amd.so --out profiles/fp8_kv_cache.txt
"""
import argparse
import ctypes
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 128
# (name, query heads, KV heads, B)
SHAPES = [("Llama-2-7B 32/32", 32, 32, 1), ("Llama-2-7B 32/32", 32, 32, 16), ("Llama-2-7B 32/32", 32, 32, 64), ("Mistral-7B 32/8", 32, 8, 64),
          ("Llama-2-70B 64/8", 64, 8, 16)]
DECODE_POS = (256, 1024, 2048)
PREFILL = [(128, 0), (128, 1024)]      # (T, pos0)
CASES = [("decode",) + s + (1, p) for s in SHAPES for p in DECODE_POS] + [("prefill",) + s + tp for s in SHAPES for tp in PREFILL]
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
    from quick_amd.attention import quantize_kv
    tree = _lib.load()
    parent = _parent_lib(parent_path) if parent_path else None
    kind, name, nh, nkv, B, T, p = CASES[index]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(index)
    L = p + 128
    ang = torch.outer(torch.arange(L, device=dev).float(), 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=dev).half()
    kc = [torch.randn(B, nkv, L, D, generator=g, device=dev).half() for _ in range(SETS)]
    vc = [torch.randn(B, nkv, L, D, generator=g, device=dev).half() for _ in range(SETS)]
    kb = [quantize_kv(t, 1.0) for t in kc]
    vb = [quantize_kv(t, 1.0) for t in vc]
    q = torch.empty((B, nh, T, D), dtype=torch.float16, device=dev)
    out = torch.empty((B * T, nh * D), dtype=torch.float16, device=dev)
    pos = torch.full((1,), p, dtype=torch.int64, device=dev)
    scale = D ** -0.5

    def launcher(lib, fp8):
        ks, vs = (kb, vb) if fp8 else (kc, vc)
        tail = (1.0, 1.0, 0) if fp8 else ()
        suffix = "_fp8" if fp8 else "_f16"
        if kind == "decode":
            fn = getattr(lib, "quick_decode_rope_attention" + suffix)

            def run(i):
                rc = fn(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), ks[i].data_ptr(), vs[i].data_ptr(), out.data_ptr(), B, nh,
                        nkv, D, L, scale, *tail, torch.cuda.current_stream().cuda_stream)
                assert rc == 0, rc
        else:
            write, attend = getattr(lib, "quick_rope_kv_write" + suffix), getattr(lib, "quick_prefill_attention" + suffix)

            def run(i):
                st = torch.cuda.current_stream().cuda_stream
                rc = write(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), q.data_ptr(), ks[i].data_ptr(), vs[i].data_ptr(), B, T,
                           nh, nkv, D, L, *tail, st)
                rc = rc or attend(q.data_ptr(), ks[i].data_ptr(), vs[i].data_ptr(), pos.data_ptr(), out.data_ptr(), B, T, nh, nkv, D, L, scale,
                                  *tail, st)
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
        variants["parent"] = variants["parent again"] = launcher(parent, False)
    variants["fp16"] = launcher(tree, False)
    variants["fp8"] = launcher(tree, True)

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
    rows = p + T
    mb16 = B * nkv * rows * D * 2 * 2 / 1e6
    text = f"{kind:<7} {name:<17} B={B:<3} {where:<16} cache read fp16 {mb16:7.1f} MB"
    if parent is not None:
        lo_p, hi_p = sorted((med["parent"], med["parent again"]))
        spread = hi_p / lo_p
        text += (f"  parent {med['parent']:8.2f} / {med['parent again']:8.2f} us  spread {spread:.3f}  fp16 {med['fp16']:8.2f}  fp16/parent "
                 f"{med['fp16'] / lo_p:.3f}  fp8 {med['fp8']:8.2f}  fp8/parent {med['fp8'] / lo_p:.3f}")
        text += "   <-- fp8 NOT ahead of the parent beyond its spread" if med["fp8"] * spread >= lo_p else ""
    else:
        text += f"  fp16 {med['fp16']:8.2f} us  fp8 {med['fp8']:8.2f}  fp8/fp16 {med['fp8'] / med['fp16']:.3f}"
    print(text, flush=True)


def _accuracy():
    import torch
    from quick_amd import QuantAttentionFused, quantize_linear
    dev = torch.device("cuda:0")
    hidden, nh, nkv, B, T0, steps = 512, 4, 2, 2, 48, 16
    os.environ["AWQ_BATCH_SIZE"] = str(B)
    g = torch.Generator().manual_seed(2024)
    lin = lambda n_out: torch.nn.Linear(hidden, n_out, bias=False, dtype=torch.float16)
    qkv_lin, o_lin = lin((nh + 2 * nkv) * D), lin(hidden)
    qkv_lin.weight.data = (torch.randn(qkv_lin.weight.shape, generator=g) * 0.06).half()
    o_lin.weight.data = (torch.randn(o_lin.weight.shape, generator=g) * 0.04).half()
    qkv, o = quantize_linear(qkv_lin, 4, 128).to(dev), quantize_linear(o_lin, 4, 128).to(dev)
    x = torch.randn(B, T0 + steps, hidden, generator=g).half().to(dev)

    def run(**kw):
        m = QuantAttentionFused(hidden, nh, nkv, qkv, o, dev, 128, **kw)
        att = [m(x[:, :T0])[1]] + [m(x[:, T0 + i:T0 + i + 1])[1] for i in range(steps)]
        return torch.cat(att, 1).float(), m
    ref, m16 = run()
    n = T0 + steps
    kmax, vmax = float(m16.k_cache[:, :, :n].abs().max()), float(m16.v_cache[:, :, :n].abs().max())
    rms = float(ref.pow(2).mean().sqrt())
    for label, ks, vs in (("scale 1.0", 1.0, 1.0), (f"scale absmax / 448 (K {kmax:.3f}, V {vmax:.3f})", kmax / 448, vmax / 448)):
        got, _ = run(kv_cache_dtype="fp8_e4m3", k_scale=ks, v_scale=vs)
        diff = got - ref
        print(f"accuracy  hidden {hidden} {nh}/{nkv} B={B} prefill {T0} + {steps} decode steps, N(0, 1) activations, {label}: attention output "
              f"fp8 - fp16 cache, relative to the output's RMS ({rms:.4f}): largest {float(diff.abs().max()) / rms:.4f}  RMS "
              f"{float(diff.pow(2).mean().sqrt()) / rms:.4f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--accuracy", action="store_true", help="(child) the accuracy figure alone")
    ap.add_argument("--parent", default=None, help="libquick_amd.so built from the parent commit (omitted: no parent columns)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp8_kv_cache.txt"))
    args = ap.parse_args()
    if args.accuracy:
        return _accuracy()
    if args.case is not None:
        return _case(args.case, args.parent)
    lines = ["# one-byte (e4m3) KV cache: us per launch (decode) or per rope_kv_write + prefill_attention pair (prefill); medians of",
             f"# {ROUNDS} samples, a sample = an event pair around two replays of a graph of {PASSES} passes over {SETS} cache sets; the routes",
             "# alternate inside one process per shape.  parent = the parent commit's library (fp16), measured twice per round (spread = its two",
             "# medians against each other); fp16 = this tree's fp16 launch; fp8 = this tree's launch over byte caches: see tools/fp8_kv_ab.py"]
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        clocks = [ln.strip() for ln in smi.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
        lines.append("# clocks (rocm-smi --showclocks, GPU 0, before the run): " + ("; ".join(clocks) if clocks else "not reported"))
    except (OSError, subprocess.TimeoutExpired):
        lines.append("# clocks: rocm-smi not available")
    print("\n".join(lines), flush=True)
    head, ok = len(lines), True
    jobs = [["--case", str(i)] + (["--parent", args.parent] if args.parent else []) for i in range(len(CASES))] + [["--accuracy"]]
    for job in jobs:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__)] + job
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"# {' '.join(job)} ended with status {r.returncode}: the run stops here\n# " + r.stderr.strip().replace("\n", "\n# ")[-2000:])
            print(lines[-1], flush=True)
            ok = False
            break
        lines.append(r.stdout.strip())
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok and len(lines) == head + len(jobs) else 1


if __name__ == "__main__":
    sys.exit(main())
