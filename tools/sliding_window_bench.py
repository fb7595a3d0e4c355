"""The sliding-window launches over a ring cache (kernels.rope_attention / kernels.prefill_attention with window=4096) against the
existing fp16 launches over a linear cache (the same calls with window=None: quick_decode_rope_attention_f16 and
quick_prefill_attention_f16, whose sources this tree does not touch), on the same box in the same session, the routes alternating inside
one process per (model, batch) (the method of tools/fp8_kv_ab.py):

    linear@4095   the existing launch at position 4095 of a linear cache: the same number of attended rows as a full window.  Twice per
                  round: the ratio of its two medians is the spread the box shows against itself
    window@p      the windowed launch at position p = 4095, 8192, 32000 of a ring of 4096 + 128 - 1 = 4223 rows
    linear@p      for p = 8192 and 32000, the existing launch at that position of a linear cache of p + 128 rows: what a user pays today

(a) decode: one fused step (RoPE + append + attention).  (b) prefill: the attention launch of a 128-token chunk at pos0 = p (the chunk's
rows are in the cache; the write launch is the same work on both routes and is left out).  Llama-2-7B (32 / 32 heads) and Mistral-7B
(32 / 8) at batch sizes 1 and 64.  Every variant is a captured graph of PASSES passes over its cache sets (as many sets, up to 4, as fit
12 GB: HBM-cold like a model's layers); a sample is an event pair around one replay; the table gives the median of ROUNDS samples in us
per launch.  The expectation: window@p level with linear@4095 at every p, and linear@p / window@p about (p + 1) / 4096.

    timeout -k 10 1100 python tools/sliding_window_bench.py --out profiles/sliding_window.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, W, T = 128, 4096, 128
RING = W + T - 1
POSITIONS = (4095, 8192, 32000)
NP = POSITIONS[-1] + T          # table rows: the exclusive bound on positions
# (name, query heads, KV heads, B)
GROUPS = [("Llama-2-7B 32/32", 32, 32, 1), ("Llama-2-7B 32/32", 32, 32, 64), ("Mistral-7B 32/8", 32, 8, 1), ("Mistral-7B 32/8", 32, 8, 64)]
PASSES, ROUNDS, MAX_SETS, SET_BYTES = 3, 11, 4, 12e9
CHILD_LIMIT = 240      # seconds per (model, batch)


def _group(index):
    import torch
    from quick_amd import kernels
    name, nh, nkv, B = GROUPS[index]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(index)
    ang = torch.outer(torch.arange(NP, device=dev).float(), 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=dev).half()
    q = torch.randn(B, nh, T, D, generator=g, device=dev).half()
    out1 = torch.empty((B, nh * D), dtype=torch.float16, device=dev)
    outT = torch.empty((B * T, nh * D), dtype=torch.float16, device=dev)

    def caches(rows):
        n = max(1, min(MAX_SETS, int(SET_BYTES // (B * nkv * rows * D * 2 * 2))))
        return [(torch.empty(B, nkv, rows, D, dtype=torch.float16, device=dev).normal_(generator=g),
                 torch.empty(B, nkv, rows, D, dtype=torch.float16, device=dev).normal_(generator=g)) for _ in range(n)]

    def variant(kind, p, window):
        """A captured graph of PASSES passes over the cache sets of one route at one position; -> (graph, launches per replay, keep-alive)."""
        sets = caches(RING if window else p + T)
        pos = torch.full((1,), p, dtype=torch.int64, device=dev)
        kw = dict(window=W, table_rows=NP) if window else {}

        def run(k, v):
            if kind == "decode":
                kernels.rope_attention(qkv, cos, sin, pos, k, v, out1, nh, nkv, D, **kw)
            else:
                kernels.prefill_attention(q, k, v, pos, outT, nh, nkv, D, **kw)
        for k, v in sets:
            run(k, v)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(PASSES):
                for k, v in sets:
                    run(k, v)
        graph.replay()
        torch.cuda.synchronize()
        return graph, PASSES * len(sets), (sets, pos)

    def timed(v):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        v[0].replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / v[1]

    for kind in ("decode", "prefill"):
        base = variant(kind, POSITIONS[0], False)
        for p in POSITIONS:
            variants = {"linear@4095": base, "linear@4095 again": base, "window": variant(kind, p, True)}
            if p != POSITIONS[0]:
                variants["linear@p"] = variant(kind, p, False)
            samples = {k: [] for k in variants}
            for _ in range(ROUNDS):
                for k, v in variants.items():
                    samples[k].append(timed(v))
            med = {k: statistics.median(v) for k, v in samples.items()}
            lo_p, hi_p = sorted((med["linear@4095"], med["linear@4095 again"]))
            spread = hi_p / lo_p
            where = f"pos={p}" if kind == "decode" else f"T={T} pos0={p}"
            text = (f"{kind:<7} {name:<17} B={B:<3} {where:<18} linear@4095 {med['linear@4095']:9.2f} / {med['linear@4095 again']:9.2f} us  spread "
                    f"{spread:.3f}  window@p {med['window']:9.2f}  window/linear@4095 {med['window'] / lo_p:.3f}")
            if "linear@p" in med:
                text += f"  linear@p {med['linear@p']:10.2f}  linear@p/window {med['linear@p'] / med['window']:6.2f}  (rows {(p + 1) / W:.2f}x)"
            if med["window"] > hi_p * spread:
                text += "   <-- window slower than linear@4095 beyond its spread"
            print(text, flush=True)
            del variants, samples
            torch.cuda.empty_cache()
        del base
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=None, help="(child) one (model, batch) of GROUPS")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliding_window.txt"))
    args = ap.parse_args()
    if args.group is not None:
        return _group(args.group)
    lines = ["# sliding window (W = 4096) over a ring of 4223 rows against the existing fp16 launches over a linear cache: us per launch, medians",
             f"# of {ROUNDS} samples, a sample = an event pair around one replay of a graph of {PASSES} passes over up to {MAX_SETS} cache sets; the",
             "# routes alternate inside one process per (model, batch).  linear@4095 = the existing launch at position 4095 (the rows of a full",
             "# window), measured twice per round (spread = its two medians against each other); window@p = the windowed launch at position p;",
             "# linear@p = the existing launch at position p of a linear cache of p + 128 rows: see tools/sliding_window_bench.py"]
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        clocks = [ln.strip() for ln in smi.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
        lines.append("# clocks (rocm-smi --showclocks, GPU 0, before the run): " + ("; ".join(clocks) if clocks else "not reported"))
    except (OSError, subprocess.TimeoutExpired):
        lines.append("# clocks: rocm-smi not available")
    print("\n".join(lines), flush=True)
    ok = True
    for i in range(len(GROUPS)):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--group", str(i)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.stdout.strip():
            lines.append(r.stdout.strip())
            print(lines[-1], flush=True)
        if r.returncode != 0:
            lines.append(f"# --group {i} ended with status {r.returncode}: the run stops here\n# " + r.stderr.strip().replace("\n", "\n# ")[-2000:])
            print(lines[-1], flush=True)
            ok = False
            break
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
