"""Offline: the four-wave kernels' launch-time models (pick_family in w4a16_plan.hip, `xwc`) against the three-box planner audit of the final r06 tree, a relative least-squares refit of their
coefficients on the per-shape median, and which forced four-wave launch each set of coefficients would pick.
    python tools/xw_model_refit.py profiles/r06_planner_audit_raw/planner_audit_{c,d,e}.jsonl.gz
Result (profiles/r06_xw_model_refit.txt): the shipped coefficients read 1.04-1.05 x the measured time (rms 5-8 %); refitted 2.6-4.9 %.  Among the forced four-wave variants the
refit picks better (geomean pick / best 1.0044 -> 1.0016, worst 1.156 -> 1.095) -- most of it the 160..256-token rows on N = 4096 layers, which became a planner rule instead -- but
it also moves picks the wrong way (2048 x 4096 x 12288, 320 x 4096 x 22016), and a simulation of the whole decision (four-wave against the other families at any threshold) changes
the audit's geometric mean by less than the sampling noise between two forced runs of the same launch.  The coefficients stay; the audit's consistent gaps became rules."""
import collections, gzip, json, sys
import numpy as np

OLD = {(4, 2): (-2.8632, 5.8843, 0.8799, 0.6018, -0.6402 - 0.5, 1.2461, 5.8244), (4, 1): (-0.3015, 1.9468, 0.5116, 0.3473, -0.0715 - 0.5, 1.0316, 4.3280),
       (2, 1): (1.8009, 3.7953, 0.3277, 0.2559, 0.1770 - 0.5, 0.3541, 0.0325)}
VAR = {'xw21s1': (2, 1, 1), 'xw21s2': (2, 1, 2), 'xw41s1': (4, 1, 1), 'xw41s2': (4, 1, 2), 'xw41s4': (4, 1, 4), 'xw42s1': (4, 2, 1), 'xw42s2': (4, 2, 2), 'xw42s4': (4, 2, 4)}


def load(path):
    by = collections.defaultdict(dict)
    op = gzip.open if path.endswith(".gz") else open
    for l in op(path, "rt"):
        r = json.loads(l)
        by[r["shape"]][r["variant"]] = r
    return by


def feats(M, K, N, mb, pairs, sx):
    KT = K // 128
    T = ((M + mb * 32 - 1) // (mb * 32)) * (N // (pairs * 128))
    f, n, st = T * sx / 256.0, (T * sx + 255) // 256, (KT + sx - 1) // sx
    return np.array([1, n, st * n, st * f, 1.0 if sx > 1 else 0.0, sx if sx > 1 else 0.0, f], dtype=float), T


data = [load(p) for p in sys.argv[1:]]
rows = collections.defaultdict(list)
for s in data[0]:
    M, K, N = (int(v) for v in s.split("x"))
    for v, (mb, pairs, sx) in VAR.items():
        ts = [d[s][v]["kernel_us"] for d in data if v in d[s] and d[s][v].get("kernel_us")]
        plan = data[0][s].get(v, {}).get("plan", "")
        if len(ts) < 2 or f"tokens={mb * 32} channels={pairs * 128}" not in plan or f"slices={sx}" not in plan:
            continue
        ft, T = feats(M, K, N, mb, pairs, sx)
        rows[(mb, pairs)].append((s, v, float(np.median(ts)), ft, T, sx))
new = {}
for key, rs in sorted(rows.items()):
    A = np.array([r[3] for r in rs])
    meas = np.array([r[2] for r in rs])
    rel = (A @ np.array(OLD[key])) / meas
    coef = np.linalg.lstsq(A / meas[:, None], np.ones(len(rs)), rcond=None)[0]
    rel2 = (A @ coef) / meas
    new[key] = coef
    print(f"tile {key[0] * 32} x {key[1] * 128}: {len(rs)} launches; shipped coefficients: mean model / measured {rel.mean():.3f}, rms {np.sqrt(np.mean((rel - 1) ** 2)):.3f}; "
          f"refit: rms {np.sqrt(np.mean((rel2 - 1) ** 2)):.3f}, range {rel2.min():.3f} .. {rel2.max():.3f}\n   refit coefficients (c, a, b_ceil, b_frac, s0, s1, d): {np.round(coef, 4).tolist()}")
for name, coefs in (("shipped", OLD), ("refit", new)):
    ratios, bad = [], []
    for s in data[0]:
        M, K, N = (int(v) for v in s.split("x"))
        cand = {}
        for key, rs in rows.items():
            for r in rs:
                if r[0] == s and not (r[5] > 1 and r[4] * r[5] > 256):
                    cand[r[1]] = (r[2], float(r[3] @ np.array(coefs[key])))
        if len(cand) < 2:
            continue
        pick, best = min(cand, key=lambda v: cand[v][1]), min(cand, key=lambda v: cand[v][0])
        ratios.append(cand[pick][0] / cand[best][0])
        if ratios[-1] > 1.04:
            bad.append(f"{s}: {pick} for {best} {ratios[-1]:.3f}")
    g = np.array(ratios)
    print(f"{name}: pick / best among the forced four-wave launches, {len(g)} shapes: geomean {np.exp(np.mean(np.log(g))):.4f}, worst {g.max():.3f}, > 3 %: {(g > 1.03).sum()}\n   " + "; ".join(bad))
