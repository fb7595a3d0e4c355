"""The planner's answer for a fixed grid of launches, one line each: (M, K, N, G, kernel id, grid_split_k, environment) ->
quick_w4a16_plan_describe (with the launch-time models' estimates), quick_w4a16_workspace_bytes_ex, quick_w4a16_can_fuse_rmsnorm.
Host-only (no GPU); the instrument for planner refactors and rule edits.

    python tools/plan_table.py [--lib LIB] [--against OTHER_LIB] [--env NAME ...]

--lib: the library to ask (default: the in-tree product library).  --against: a second library with the same C ABI (say, the parent
commit's build); only the rows where the two differ are printed, and the exit status is 1 if any do.  Switches the library reads once per
process (QUICK_AMD_XM, QUICK_AMD_EXCHANGE_CUS) get a fresh process per environment."""
import ctypes
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

AUTO, SKINNY, TILED, WIDE, XK, XW, LEAN, XM = range(8)
ENVS = {"default": {}, "xm0": {"QUICK_AMD_XM": "0"}, "xw256_0": {"QUICK_AMD_XW256": "0"},
        "cus0": {"QUICK_AMD_EXCHANGE_CUS": "0"}, "cus60": {"QUICK_AMD_EXCHANGE_CUS": "60"},
        "cus100": {"QUICK_AMD_EXCHANGE_CUS": "100"}, "cus128": {"QUICK_AMD_EXCHANGE_CUS": "128"},
        "poll1": {"QUICK_AMD_EXCHANGE_POLL_LOG2": "1"}}
_ENV_KEYS = sorted({k for e in ENVS.values() for k in e})

MS_ALL = list(range(1, 161)) + [192, 224, 256, 257, 300, 320, 384, 448, 512, 513, 640, 768, 1000, 1024, 1536, 2048, 2049, 3072, 4096, 4100, 6144, 8192]
MS_COARSE = [1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13, 16, 17, 24, 32, 33, 40, 48, 56, 57, 64, 65, 80, 96, 128, 129, 160, 192, 256, 257, 300, 512, 513,
             1000, 2049, 4100, 8192]
SHAPES = [  # (K, N): the plan pins' and the decode models' layers, small layers, N % 256 == 128
    (4096, 4096), (4096, 6144), (4096, 8192), (4096, 11008), (4096, 12288), (4096, 13824), (4096, 22016), (4096, 28672), (11008, 4096), (14336, 4096),
    (5120, 5120), (5120, 13824), (5120, 15360), (5120, 27648), (13824, 5120), (8192, 8192), (8192, 10240), (8192, 16384), (8192, 28672),
    (8192, 57344), (28672, 8192), (8192, 1792), (18944, 3584), (3584, 18944), (20480, 7168), (7168, 7168), (4608, 4096), (1536, 4096),
    (128, 128), (256, 256), (512, 384), (1024, 256), (1024, 384), (1024, 512), (1024, 1024), (384, 640), (2048, 640), (8192, 1152), (4096, 4224)]
GS = [32, 64, 128, 256, 384]
SPLITS = [1, 2, 3, 4, 8]

# kernel-id fields (include/quick_amd.h, "kernel id") and the values each family documents
_F = lambda v, sh: v << sh
BITS = {
    AUTO: [_F(1, 12), _F(4, 4), _F(2, 8), _F(1, 14), _F(1, 21)],
    SKINNY: [_F(m, 4) for m in (1, 2, 4, 7, 8)] + [_F(w, 8) for w in (1, 2, 4)] + [_F(1, 12), _F(1, 21), _F(1, 22), _F(2, 22), _F(1, 25), _F(1, 26), _F(1, 28),
             _F(1, 4) | _F(4, 8), _F(1, 4) | _F(1, 21), _F(1, 4) | _F(2, 22) | _F(1, 26), _F(2, 4) | _F(1, 12), _F(4, 4) | _F(1, 25), _F(8, 4) | _F(4, 8)],
    TILED: [_F(m, 4) for m in (2, 4, 8)] + [_F(w, 8) for w in (2, 4)] + [_F(1, 13), _F(1, 14), _F(1, 15), _F(1, 27), _F(1, 29), _F(1, 30),
            _F(4, 4) | _F(1, 15), _F(2, 4) | _F(1, 29), _F(1, 16), _F(17, 16)],
    WIDE: [_F(m, 4) for m in (2, 4, 8)] + [_F(1, 8), _F(2, 8), _F(1, 12), _F(1, 14), _F(1, 15), _F(3, 22), _F(4, 22), _F(6, 22),
           _F(2, 4) | _F(1, 8) | _F(1, 15) | _F(4, 22), _F(8, 4) | _F(2, 8), _F(4, 4) | _F(2, 8) | _F(1, 15), _F(1, 16)],
    XK: [_F(m, 4) for m in (2, 4)] + [_F(s, 8) for s in (1, 2, 4, 8, 15)] + [_F(1, 12), _F(1, 13), _F(1, 14), _F(3, 22), _F(6, 22), _F(3, 26), _F(6, 26),
         _F(2, 4) | _F(1, 13), _F(2, 4) | _F(2, 8), _F(4, 4) | _F(4, 8), _F(1, 16), _F(20, 16)],
    XW: [_F(m, 4) for m in (2, 4, 8)] + [_F(s, 8) for s in (1, 2, 4)] + [_F(1, 12), _F(1, 14), _F(1, 22), _F(12, 22),
         _F(4, 4) | _F(1, 12), _F(2, 4) | _F(2, 8), _F(4, 4) | _F(4, 8), _F(8, 4) | _F(2, 8), _F(2, 4) | _F(2, 8) | _F(1, 22), _F(1, 16)],
    LEAN: [_F(m, 4) for m in (1, 2)] + [_F(w, 8) for w in (1, 2, 4)] + [_F(1, 22), _F(2, 22), _F(2, 4) | _F(2, 8), _F(1, 22) | _F(2, 8), _F(1, 16)],
    XM: [_F(m, 4) for m in (1, 2, 3)] + [_F(t, 8) for t in (1, 2)] + [_F(3, 4) | _F(2, 8), _F(1, 4) | _F(1, 8), _F(1, 16)],
}


def rows():
    """(M, K, N, G, kernel id, grid_split_k) of the grid"""
    for K, N in SHAPES:
        for G in GS:
            if K % G:
                continue
            for fam in range(8):   # AUTO and every family bare: every M, every G
                for M in MS_ALL:
                    yield M, K, N, G, fam, 0
            if G == 128:   # every slice count and kernel-id field: the coarse ladder
                for fam in range(8):
                    for M in MS_COARSE:
                        for s in SPLITS:
                            yield M, K, N, G, fam, s
                        for b in BITS[fam]:
                            yield M, K, N, G, fam | b, 0


class Planner:
    def __init__(self, path):
        from quick_amd import _lib
        self.lib = _lib.load() if path is None else _lib.load_other(path)
        self.buf = ctypes.create_string_buffer(512)
        self.fuse = {}

    def row(self, M, K, N, G, kid, s):
        lib, buf = self.lib, self.buf
        rc = lib.quick_w4a16_plan_describe(M, K, N, G, kid, s, buf, len(buf))
        text = buf.value.decode() if rc == 0 else "rc=%d" % rc
        key = (M, K, N, G)
        if key not in self.fuse:
            self.fuse[key] = lib.quick_w4a16_can_fuse_rmsnorm(M, K, N, G)
        return "%s | workspace_ex=%d | fuse=%d" % (text, lib.quick_w4a16_workspace_bytes_ex(M, K, N, G, kid, s), self.fuse[key])


def worker(env, lib, against):
    a = Planner(lib)
    b = Planner(against) if against else None
    n = ndiff = 0
    out = sys.stdout
    for r in rows():
        n += 1
        key = "%d %d %d %d 0x%08x %d %s" % (r + (env,))
        ra = a.row(*r)
        if b is None:
            out.write("%s: %s\n" % (key, ra))
            continue
        rb = b.row(*r)
        if ra != rb:
            ndiff += 1
            out.write("%s:\n  lib:     %s\n  against: %s\n" % (key, ra, rb))
    sys.stderr.write("plan_table: env %s: %d rows, %d differ\n" % (env, n, ndiff))
    return 1 if ndiff else 0


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--against", default=None)
    ap.add_argument("--env", nargs="*", default=list(ENVS), choices=list(ENVS))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.worker:
        return worker(args.worker, args.lib, args.against)
    rc = 0
    for name in args.env:
        env = {k: v for k, v in os.environ.items() if k not in _ENV_KEYS}
        env.update(ENVS[name], QUICK_AMD_PLAN_ESTIMATES="1")
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", name]
        cmd += ["--lib", os.path.abspath(args.lib)] if args.lib else []
        cmd += ["--against", os.path.abspath(args.against)] if args.against else []
        sys.stdout.flush()
        rc |= subprocess.run(cmd, env=env).returncode
    return rc


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
