"""Prefill attention, two routes for the same job on the same box in the same session:

    new     kernels.rope_kv_write + kernels.prefill_attention               (two launches, out [B * T, H] as o_proj wants it)
    parent  kernels.rope_kv_write + F.scaled_dot_product_attention + the transpose copy to [B * T, H]; is_causal=True on the chunk's
            own rows where pos0 == 0, a materialised additive [T, pos0 + T] mask over the cache (built once, outside the timed
            window) where pos0 > 0 -- what the package did before it had the kernel

Each shape runs in a child process of its own under a time limit; the first child that fails ends the run.  Per shape: 5 warm-up
calls of each route, then 15 rounds of (new, parent, parent again), each an event pair around 10 calls; the table gives the medians per
call.  "spread" is the ratio of the parent's two medians (the larger over the smaller): what the parent's route shows against itself.
The new route is marked SLOWER where new / parent exceeds that spread.  The box's clocks as rocm-smi reports them are noted on top.

    timeout -k 10 900 python tools/prefill_attention_ab.py --out profiles/prefill_attention.txt
"""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 128
# (name, query heads, KV heads, B, T)
SHAPES = [("Llama-2-7B 32/32", 32, 32, 1, 128), ("Llama-2-7B 32/32", 32, 32, 64, 128), ("Llama-2-7B 32/32", 32, 32, 1, 2048),
          ("Mistral-7B 32/8", 32, 8, 64, 128), ("Llama-2-70B 64/8", 64, 8, 16, 128)]
POS0 = (0, 512)
CASES = [(s, p) for s in SHAPES for p in POS0]
WARMUP, ROUNDS, INNER = 5, 15, 10
CHILD_LIMIT = 120      # seconds per shape


def _case(index):
    import torch
    import torch.nn.functional as F
    from quick_amd import kernels
    (name, nh, nkv, B, T), p0 = CASES[index]
    dev = torch.device("cuda:0")
    L = p0 + T
    g = torch.Generator(device=dev).manual_seed(index)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=dev).half()
    kc = torch.randn(B, nkv, L, D, generator=g, device=dev).half()
    vc = torch.randn(B, nkv, L, D, generator=g, device=dev).half()
    ang = torch.outer(torch.arange(L, device=dev).float(), 1.0 / (10000.0 ** (torch.arange(0, D, 2, device=dev).float() / D)))
    cos, sin = torch.cat((ang.cos(), ang.cos()), -1).half(), torch.cat((ang.sin(), ang.sin()), -1).half()
    pos = torch.full((1,), p0, dtype=torch.int64, device=dev)
    q = torch.empty((B, nh, T, D), dtype=torch.float16, device=dev)
    out = torch.empty((B * T, nh * D), dtype=torch.float16, device=dev)
    mask = None
    if p0 > 0:
        mask = torch.full((T, L), float("-inf"), dtype=torch.float16, device=dev).triu(p0 + 1)

    def new():
        kernels.rope_kv_write(qkv, cos, sin, pos, q, kc, vc, T, nh, nkv, D)
        kernels.prefill_attention(q, kc, vc, pos, out, nh, nkv, D)
        return out

    def parent():
        kernels.rope_kv_write(qkv, cos, sin, pos, q, kc, vc, T, nh, nkv, D)
        if mask is None:
            att = F.scaled_dot_product_attention(q, kc[:, :, :T], vc[:, :, :T], is_causal=True, enable_gqa=nkv != nh)
        else:
            att = F.scaled_dot_product_attention(q, kc, vc, attn_mask=mask, enable_gqa=nkv != nh)
        return att.transpose(1, 2).reshape(B * T, nh * D)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(INNER):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / INNER

    for _ in range(WARMUP):
        a, b = new(), parent()
    torch.cuda.synchronize()
    diff = float((a.float() - b.float()).abs().max())          # (the two routes compute the same thing)
    t_new, t_p1, t_p2 = [], [], []
    for _ in range(ROUNDS):
        t_new.append(timed(new))
        t_p1.append(timed(parent))
        t_p2.append(timed(parent))
    med = statistics.median
    n, p1, p2 = med(t_new), med(t_p1), med(t_p2)
    p, spread = min(p1, p2), max(p1, p2) / min(p1, p2)
    ratio = n / p
    flop = 4.0 * B * nh * D * sum(p0 + t + 1 for t in range(T))       # both products, causal
    note = "   <-- SLOWER than the parent's route beyond its spread" if ratio > spread else ""
    print(f"{name:<17} B={B:<3} T={T:<5} pos0={p0:<4} new {n:9.1f} us ({min(t_new):.1f} .. {max(t_new):.1f})  parent {p1:9.1f} / {p2:9.1f} us  "
          f"spread {spread:.3f}  new/parent {ratio:.2f}  {flop / n * 1e-6:7.1f} TFLOP/s  max|new - parent| {diff:.2e}{note}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", type=int, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_attention.txt"))
    args = ap.parse_args()
    if args.case is not None:
        return _case(args.case)
    lines = ["# prefill attention: rope_kv_write + prefill_attention (new) against rope_kv_write + SDPA + transpose copy (parent); us per call,",
             f"# medians of {ROUNDS} event pairs around {INNER} calls after {WARMUP} warm-up calls, the routes alternating; one process per shape;",
             "# spread = the parent's two medians against each other; TFLOP/s = 4 B nh D sum_t (pos0 + t + 1) over the new route's time (RoPE included)"]
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=60).stdout
        clocks = [ln.strip() for ln in smi.splitlines() if "GPU[0]" in ln and ("sclk" in ln or "mclk" in ln)]
        lines.append("# clocks (rocm-smi --showclocks, GPU 0, before the run): " + ("; ".join(clocks) if clocks else "not reported"))
    except (OSError, subprocess.TimeoutExpired):
        lines.append("# clocks: rocm-smi not available")
    print("\n".join(lines), flush=True)
    for i in range(len(CASES)):
        r = subprocess.run(["timeout", "-k", "10", str(CHILD_LIMIT), sys.executable, os.path.abspath(__file__), "--case", str(i)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            lines.append(f"# case {i} {CASES[i]} ended with status {r.returncode}: the run stops here\n# " + r.stderr.strip().replace("\n", "\n# ")[-2000:])
            print(lines[-1], flush=True)
            break
        lines.append(r.stdout.strip())
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if len(lines) >= 4 + len(CASES) else 1


if __name__ == "__main__":
    sys.exit(main())
