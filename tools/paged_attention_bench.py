"""The paged launches (kernels.rope_attention / kernels.prefill_attention with block_table=..., per_sequence=True) against the existing
per-sequence fp16 launches over a linear cache (the same calls without a block table: quick_decode_rope_attention_seq_f16 and
quick_prefill_attention_seq_f16, whose sources this tree does not touch), on the same box in the same session, the routes alternating
inside one process per (model, batch) (the method of tools/sliding_window_bench.py):

    linear        the existing per-sequence launch over caches [B, nkv, p + 128, 128].  Twice per round: the ratio of its two medians is
                  the spread the box shows against itself
    P64  / P256   the paged launch over a pool of B * ceil((p + 128) / P) pages with a CONTIGUOUS table (sequence b holds pages b n ..
                  b n + n - 1 in order: the linear cache's addresses but for the page's head stride)
    P64s / P256s  the same pool with a SCRAMBLED table (a random permutation of the pool's pages)

(a) decode: one fused step (RoPE + append + attention) at position p.  (b) prefill: the attention launch of a 128-token chunk at pos0 = p
(the chunk's rows are in the cache; the write launch touches 128 rows on either route and is left out).  Llama-2-7B (32 / 32 heads),
Mistral-7B (32 / 8) and Llama-2-70B (64 / 8) at batch sizes 1, 16 and 64 and p = 190, 1024 and 4096.  Every variant is a captured graph
of PASSES passes over its cache sets (as many sets, up to 4, as fit 8 GB: HBM-cold like a model's layers); a sample is an event pair
around one replay; the table gives the median of ROUNDS samples in us per launch.

    timeout -k 10 1100 python tools/paged_attention_bench.py --out profiles/paged_attention.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, T = 128, 128
POSITIONS = (190, 1024, 4096)
NP = POSITIONS[-1] + T          # table rows: the exclusive bound on positions
MODELS = [("Llama-2-7B 32/32", 32, 32), ("Mistral-7B 32/8", 32, 8), ("Llama-2-70B 64/8", 64, 8)]
GROUPS = [(name, nh, nkv, B) for name, nh, nkv in MODELS for B in (1, 16, 64)]
PAGED = (("P64", 64, False), ("P64s", 64, True), ("P256", 256, False), ("P256s", 256, True))
PASSES, ROUNDS, MAX_SETS, SET_BYTES = 3, 11, 4, 8e9
CHILD_LIMIT = 150      # seconds per (model, batch)


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

    def caches(shape):
        elems = shape[0] * shape[1] * shape[2] * D
        n = max(1, min(MAX_SETS, int(SET_BYTES // (elems * 2 * 2))))
        return [(torch.empty(*shape, D, dtype=torch.float16, device=dev).normal_(generator=g),
                 torch.empty(*shape, D, dtype=torch.float16, device=dev).normal_(generator=g)) for _ in range(n)]

    def variant(kind, p, page, scrambled):
        """A captured graph of PASSES passes over the cache sets of one route at one position; -> (graph, launches per replay, keep-alive)."""
        pos = torch.full((B,), p, dtype=torch.int64, device=dev)
        if page is None:
            sets, kw = caches((B, nkv, p + T)), {}
        else:
            n = -(-(p + T) // page)
            sets = caches((B * n, nkv, page))
            ids = torch.randperm(B * n, generator=torch.Generator().manual_seed(p + page)) if scrambled else torch.arange(B * n)
            kw = dict(block_table=ids.to(torch.int32).view(B, n).contiguous().to(dev), page_size=page, table_rows=NP)

        def run(k, v):
            if kind == "decode":
                kernels.rope_attention(qkv, cos, sin, pos, k, v, out1, nh, nkv, D, per_sequence=True, **kw)
            else:
                kernels.prefill_attention(q, k, v, pos, outT, nh, nkv, D, per_sequence=True, **kw)
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
        return graph, PASSES * len(sets), (sets, pos, kw)

    def timed(v):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        v[0].replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / v[1]

    for kind in ("decode", "prefill"):
        for p in POSITIONS:
            base = variant(kind, p, None, False)
            variants = {"linear": base, "linear again": base}
            for label, page, scrambled in PAGED:
                variants[label] = variant(kind, p, page, scrambled)
            samples = {k: [] for k in variants}
            for _ in range(ROUNDS):
                for k, v in variants.items():
                    samples[k].append(timed(v))
            med = {k: statistics.median(v) for k, v in samples.items()}
            lo_p, hi_p = sorted((med["linear"], med["linear again"]))
            spread = hi_p / lo_p
            where = f"pos={p}" if kind == "decode" else f"T={T} pos0={p}"
            text = (f"{kind:<7} {name:<17} B={B:<3} {where:<18} linear {med['linear']:9.2f} / {med['linear again']:9.2f} us  spread {spread:.3f} |")
            for label, _, _ in PAGED:
                text += f" {label} {med[label]:9.2f} ({med[label] / lo_p:.3f})"
                if med[label] > hi_p * spread:
                    text += "*"
            print(text, flush=True)
            del variants, samples, base
            torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", type=int, default=None, help="(child) one (model, batch) of GROUPS")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "paged_attention.txt"))
    args = ap.parse_args()
    if args.group is not None:
        return _group(args.group)
    lines = ["# paged attention (pages of 64 and 256 positions; contiguous and scrambled tables) against the existing per-sequence fp16 launches",
             f"# over a linear cache: us per launch, medians of {ROUNDS} samples, a sample = an event pair around one replay of a graph of {PASSES}",
             f"# passes over up to {MAX_SETS} cache sets; the routes alternate inside one process per (model, batch).  linear = the existing launch",
             "# over caches of p + 128 rows, measured twice per round (spread = its two medians against each other); in brackets: paged / the",
             "# faster linear median; * = slower than the linear launch beyond its spread: see tools/paged_attention_bench.py"]
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
