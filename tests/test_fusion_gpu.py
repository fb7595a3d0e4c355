"""The fusion contract of quick_w4a16_gemm_f16_fused (include/quick_amd.h) in every kernel family that carries fusions.  Needs an MI355X.

Epilogues, bit for bit: on exact-arithmetic inputs (power-of-two scales, small-integer sparse activations) every fp32 sum is exact and, in
the exchange families, every fp16 partial a K slice mails is exact too, so the only roundings left are the epilogue's.  A float64 model
of the documented rounding points -- bias in fp32 before the product's one rounding, the residual added to the ROUNDED product with a
second rounding (GEMM-then-add) -- predicts every bit; each case also checks that the other model ("round once") fails on its inputs.

Prologue, per row: rows with massive channels, tiny rows, an all-zero row and a constant row through every RMSNorm flavour, against a
float64 model of torch's rounding points fp16(fp16(x * rstd) * w) followed by the oracle GEMM, and against the two-launch path.
"""
import zlib

import numpy as np
import pytest
import torch

import oracle

pytestmark = pytest.mark.gpu

SKINNY, TILED, WIDE, XK, XW, LEAN, XM = 1, 2, 3, 4, 5, 6, 7
UNIT = 2.0 ** -10          # x in units of 2^-3 times scales of 2^-7 / 2^-6: every product is a multiple of 2^-10


def _wide(mb, pairs, bits=0):
    return WIDE | (mb << 4) | (pairs << 8) | bits


def _xk(mb, s):
    return XK | (mb << 4) | (s << 8)


def _xw(mb, pairs, s, poll_log2=0):
    return XW | ((mb << 4) if mb != 4 else 0) | ((1 << 12) if pairs == 1 else 0) | (s << 8) | (poll_log2 << 22)


def _lean(ntw, waves, slots=0):
    return LEAN | (ntw << 4) | ((waves // 4) << 8) | (slots << 22)


def _xm(pr, tile):
    return XM | (pr << 4) | ((2 << 8) if tile == 64 else (1 << 8))


SK_EXACT, SK_TABLE, SK_NOFRAG = SKINNY | (1 << 25), SKINNY | (1 << 26), SKINNY | (1 << 28)
# (name, kernel id, grid_split_k, leading words of plan_describe, token counts at a tile boundary +- 1, K, N, G); `mailbox`: K slices
# that meet through fp16 mailboxes (then each slice's partial has to stay exact in fp16)
FAMILIES = [
    ("auto-1", 0, 0, "", (1,), 1024, 512, 128),
    ("auto-mid", 0, 0, "", (15, 17, 33), 1024, 512, 128),
    ("auto-large", 0, 0, "", (63, 65, 129, 257), 1024, 512, 128),
    ("skinny-exact", SK_EXACT, 0, "skinny", (15, 17), 1024, 512, 128),
    ("skinny-exact-ks3", SK_EXACT, 3, "skinny", (1, 16), 1536, 512, 128),
    ("skinny-table", SK_TABLE, 0, "skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table", (1, 15), 1024, 512, 128),
    ("skinny-table-17", SK_TABLE, 0, "skinny", (17,), 1024, 512, 128),
    ("skinny-table-persist-flip", SK_TABLE | (1 << 21), 0, "skinny", (5,), 1024, 8320, 128),
    ("skinny-table-ks2", SK_TABLE, 2, "skinny", (16,), 1024, 512, 64),
    ("skinny-frag-ntw2", SKINNY | (1 << 26) | (1 << 12) | (2 << 4), 0, "skinny ntw=2", (9, 15, 17), 2048, 512, 128),
    ("skinny-frag-ntw4", SKINNY | (1 << 12) | (4 << 4) | (2 << 8), 0, "skinny ntw=4", (12, 16), 4096, 1024, 128),
    ("skinny-frag-ntw4-ks2", SKINNY | (1 << 12) | (4 << 4) | (2 << 8), 2, "skinny ntw=4", (16,), 4096, 1024, 128),
    ("frag8", SKINNY | (8 << 4), 0, "skinny ntw=8", (9, 16), 8192, 1024, 128),
    ("frag8-ks2", SKINNY | (8 << 4), 2, "skinny ntw=8", (13,), 8192, 1024, 128),
    ("frag7", SKINNY | (7 << 4), 0, "skinny ntw=7", (9, 16), 8192, 896, 128),
    ("tiled-8w", TILED, 0, "tiled", (15, 17, 65), 1024, 512, 128),
    ("tiled-16w", TILED | (4 << 8), 0, "tiled", (63, 129), 1024, 512, 128),
    ("tiled-ks3", TILED, 3, "tiled", (33,), 1536, 512, 128),
    ("tiled-64x256", TILED | (1 << 29), 0, "tiled", (63, 65, 129), 1024, 512, 128),
    ("tiled-128x256", TILED | (1 << 27), 0, "tiled", (127, 129), 1024, 512, 128),
    ("lean-1x8", _lean(1, 8), 0, "lean", (1, 15, 17), 1024, 256, 128),
    ("lean-2x16", _lean(2, 16), 0, "lean", (3, 16), 2048, 384, 128),
    ("lean-1x8-persist2", _lean(1, 8, 2), 0, "lean", (4, 16), 2048, 8448, 128),
    ("xm-32x1", _xm(1, 32), 0, "xm", (31, 33), 1024, 256, 128),
    ("xm-32x3", _xm(3, 32), 0, "xm", (17, 65), 1024, 384, 128),
    ("xm-64x2", _xm(2, 64), 0, "xm", (63, 65, 127), 2048, 512, 128),
    ("wide-ring", _wide(4, 2), 0, "wide", (127, 129), 1024, 512, 128),
    ("wide-noring", _wide(2, 1, 1 << 12), 0, "wide", (63, 65), 1024, 512, 128),
    ("wide-8waves", _wide(4, 1, 1 << 15), 0, "wide", (129,), 1024, 512, 128),
    ("wide-ks2", _wide(4, 2), 2, "wide", (100,), 1024, 512, 128),
    ("xk-64-s1", _xk(2, 1), 0, "xk", (63, 65), 1024, 512, 128),
    ("xk-64-s2", _xk(2, 2), 0, "xk", (65, 129), 1024, 512, 128),
    ("xk-128-s4", _xk(4, 4), 0, "xk", (127, 129), 1024, 512, 128),
    ("xk-128-s8", _xk(4, 8), 0, "xk", (129,), 2048, 256, 128),
    ("xw-128x256-s1", _xw(4, 2, 1), 0, "xw", (127, 129), 1024, 512, 128),
    ("xw-128x128-s2", _xw(4, 1, 2), 0, "xw", (129, 257), 1024, 512, 128),
    ("xw-64x128-s2", _xw(2, 1, 2), 0, "xw", (63, 65), 1024, 512, 128),
    ("xw-128x256-s4-giveup", _xw(4, 2, 4, poll_log2=1), 0, "xw", (129,), 1024, 512, 128),
    ("xw-256x256", _xw(8, 2, 1), 0, "xw", (255, 257), 1024, 512, 128),
    ("xk-128-s2-giveup", _xk(4, 2) | (1 << 22), 0, "xk", (127,), 1024, 512, 128),
]


@pytest.fixture(scope="module")
def K_(device):
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


def _slices(plan):
    return int(plan.split("slices=")[1].split()[0]) if "slices=" in plan else 1


def _exact_case(M, K, N, G, seed, nnz_tiles, imax):
    """Integers: x = i * 2^-3 at one column of each k tile in `nnz_tiles` (|i| <= imax; imax = 64: |x * w| <= 64 * 15 * 2^-6 < 2048
    units, a sum over one k tile is exact in fp16), weights (iw - z) * 2^-7 / 2^-6.  Every partial sum is exact in fp32."""
    rng = np.random.default_rng(seed)
    iw = rng.integers(0, 16, size=(K, N), dtype=np.uint8)
    z = rng.integers(0, 16, size=(K // G, N), dtype=np.uint8)
    s = (2.0 ** rng.integers(-7, -5, size=(K // G, N))).astype(np.float16)
    x = np.zeros((M, K), np.float64)
    for kt in nnz_tiles:
        col = kt * 128 + rng.integers(0, 128, size=M)
        x[np.arange(M), col] = rng.integers(-imax, imax + 1, size=M) * 0.125
    x = x.astype(np.float16)
    v = x.astype(np.float64) @ oracle.dequantize(iw, s, z, G).astype(np.float64)      # exact
    return x, iw, s, z, v


def _f16(a):
    return np.asarray(a, np.float64).astype(np.float16)


def _poisoned(M, ncol, device):
    """Output buffer for rows 1..M of an [M + 2, ncol] NaN-filled tensor: every element must be written and nothing next to it."""
    buf = torch.full((M + 2, ncol), float("nan"), dtype=torch.float16, device=device)
    return buf, buf[1:M + 1]


def _check_guard(buf, M):
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[M + 1]).all(), "wrote next to the output"
    assert not torch.isnan(buf[1:M + 1]).any(), "left output elements unwritten"


@pytest.mark.parametrize("name,kid,ks,word,Ms,K,N,G", FAMILIES, ids=[f[0] for f in FAMILIES])
def test_epilogue_rounding_points_bit_exact(K_, device, name, kid, ks, word, Ms, K, N, G):
    for M in Ms:
        plan = K_.plan_describe(M, K, N, G, kid, ks)
        assert plan.startswith(word), (name, M, plan)
        KT = K // 128
        # more than one K slice meeting through fp16 mailboxes: two nonzero k tiles, the first and the last (KT even: in different slices
        # whether the slices take contiguous or interleaved k tiles) -- every slice's partial is one tile's sum, exact in fp16; otherwise
        # six tiles with x up to 64 (sums up to ~2^17 units, where the product's fp16 rounding matters)
        mailbox = plan.startswith(("xk", "xw")) and _slices(plan) > 1
        assert KT % 2 == 0
        tiles = (0, KT - 1) if mailbox else tuple(sorted(set(np.linspace(0, KT - 1, 6).astype(int))))
        x, iw, s, z, v = _exact_case(M, K, N, G, seed=zlib.crc32(f"{name}/{M}".encode()), nnz_tiles=tiles, imax=64 if mailbox else 512)
        rng = np.random.default_rng(M + N)
        bias = ((2 * rng.integers(-50, 50, size=N) + 1) * 2.0 ** -11).astype(np.float16)      # half-unit offsets
        res = (rng.standard_normal((M, N)) * 2).astype(np.float16)
        qw, sc, qz = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in oracle.pack_mi355x(iw, s, z)]
        xd = torch.from_numpy(x).to(device)
        bd, rd = torch.from_numpy(bias).to(device), torch.from_numpy(res).to(device)
        assert np.abs(v).max() / UNIT > 2048, "the sums must reach where fp16 rounds them"

        def run(**kw):
            buf, out = _poisoned(M, N // 2 if kw.get("silu_mul") else N, device)
            y = K_.gemm_forward(xd, qw, sc, qz, kernel_id=kid, grid_split_k=ks, out=out, **kw)
            _check_guard(buf, M)
            return y.cpu().numpy()

        b64, r64 = bias.astype(np.float64), res.astype(np.float64)
        cases = {
            "plain": ({}, _f16(v), None),
            "bias": (dict(bias=bd), _f16(v + b64), None),
            "residual": (dict(residual=rd), _f16(_f16(v).astype(np.float64) + r64), _f16(v + r64)),
            "bias+residual": (dict(bias=bd, residual=rd), _f16(_f16(v + b64).astype(np.float64) + r64), _f16(v + b64 + r64)),
        }
        for case, (kw, want, wrong) in cases.items():
            y = run(**kw)
            bad = np.flatnonzero(y.view(np.uint16) != want.view(np.uint16))
            assert bad.size == 0, (name, M, case, plan, bad.size, y.flat[bad[0]], want.flat[bad[0]])
            # the inputs tell the two contracts apart (in the mailbox case the plain sums are exact in fp16 -- the partials have to be --
            # so only the bias's half units make the product's rounding matter)
            if wrong is not None and not (mailbox and case == "residual"):
                assert (wrong.view(np.uint16) != want.view(np.uint16)).sum() >= (1 if mailbox else max(8, want.size // 50)), (name, M, case)

        # the residual in place: out IS the residual tensor -- bit-equal to the out-of-place result
        y_oop = K_.gemm_forward(xd, qw, sc, qz, bias=bd, residual=rd, kernel_id=kid, grid_split_k=ks)
        inplace = rd.clone()
        y_in = K_.gemm_forward(xd, qw, sc, qz, bias=bd, residual=inplace, out=inplace, kernel_id=kid, grid_split_k=ks)
        assert y_in.data_ptr() == inplace.data_ptr() and torch.equal(y_in, y_oop), (name, M, plan)

        # SiLU * mul: bit-equal to quick_silu_mul_f16 on the same family's plain output; against torch's silu(gate) * up within 2 ulps
        # (the same rounding points, but __expf may put fp16(silu) one of its ulps away, which |up| scales to up to 2 ulps of the product)
        plain = K_.gemm_forward(xd, qw, sc, qz, kernel_id=kid, grid_split_k=ks)
        try:
            y_act = K_.gemm_forward(xd, qw, sc, qz, silu_mul=True, kernel_id=kid, grid_split_k=ks)
        except NotImplementedError:
            y_act = None     # (exchange launches whose waves do not finish whole token blocks: documented as unsupported)
            assert plan.startswith(("xk", "xw")), (name, M, plan)
        if y_act is not None:
            buf, out = _poisoned(M, N // 2, device)
            K_.gemm_forward(xd, qw, sc, qz, silu_mul=True, kernel_id=kid, grid_split_k=ks, out=out)
            _check_guard(buf, M)
            assert torch.equal(out, y_act) and torch.equal(y_act, K_.silu_mul(plain)), (name, M, plan)
            gu = plain.view(M, N // 16, 2, 8)
            ref = (torch.nn.functional.silu(gu[:, :, 0]) * gu[:, :, 1]).reshape(M, N // 2).float().cpu().numpy()    # torch, in fp16
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(ref), 2.0 ** -14))) - 10)     # (2^-24 below the normal range)
            assert (np.abs(y_act.float().cpu().numpy() - ref) <= 2 * ulp).all(), (name, M, plan)

        # the combinations the library refuses
        for kw in (dict(silu_mul=True, residual=rd), dict(silu_mul=True, bias=bd)):
            with pytest.raises(ValueError):
                K_.gemm_forward(xd, qw, sc, qz, kernel_id=kid, grid_split_k=ks, **kw)


# ------------------------------------------------------------------------------------------------
# RMSNorm prologue at the edges
# ------------------------------------------------------------------------------------------------
def _row_kind(m):
    """0 normal, 1 massive channels, 2 tiny, 3 all zero, 4 constant"""
    return (1, 2, 4, 3, 0)[m % 5]


def _edge_rows(M, K, rng, small_w=False):
    """Row kinds cycled over M rows (_row_kind): 1..6 massive channels (|x| 1e3 .. 3e4); tiny (rms ~ 1e-3); constant; all zero; normal --
    the edges first, so that launches of 1..4 tokens carry them too.  Norm
    weights 4 on the massive channels, elsewhere 0.5 .. 1.5 or (small_w) 0.02 .. 0.1."""
    x = np.zeros((M, K), np.float64)
    massive = np.zeros(K, bool)
    massive[rng.choice(K, 6, replace=False)] = True
    mcols = np.flatnonzero(massive)
    for m in range(M):
        kind = _row_kind(m)
        if kind == 0:
            x[m] = rng.standard_normal(K)
        elif kind == 1:
            x[m] = rng.standard_normal(K)
            n = 1 + m % 6
            x[m, mcols[:n]] = rng.choice([-1, 1], n) * np.geomspace(3e4, 1e3, n)
        elif kind == 2:
            x[m] = rng.standard_normal(K) * 1e-3
        elif kind == 4:
            x[m] = 0.75
    w = rng.uniform(0.02, 0.1, K) if small_w else rng.uniform(0.5, 1.5, K)
    w[massive] = 4.0
    return x.astype(np.float16), w.astype(np.float16), massive


def _rms_ref(x, w, eps):
    """torch's rounding points in float64: fp16(fp16(x * rstd) * w)."""
    xf = x.astype(np.float64)
    rstd = 1.0 / np.sqrt((xf * xf).mean(-1, keepdims=True) + eps)
    return _f16(_f16(xf * rstd).astype(np.float64) * w.astype(np.float64))


def _row_errs(y, ref):
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    return np.abs(y - ref).max(-1) / np.maximum(np.abs(ref).max(-1), 1e-30)


# (name, kernel id, token counts, K, N, G, leading words of plan_describe): every flavour that accepts rmsnorm_weight.  (AUTO entries: the
# words of the plan without the prologue -- a launch with one whose plan has none re-plans onto the fragment kernel)
FRAG = "skinny ntw={} waves=8 x=l2 dequant=deferred-zero-fragment"
PROLOGUES = [
    ("table", SK_TABLE, (1, 5, 16), 4096, 1024, 128, "skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table"),
    ("table-persist-flip", SK_TABLE | (1 << 21), (3,), 2048, 8320, 128, "skinny ntw=1 waves=8 x=lds dequant=deferred-zero-table"),
    ("fragment-ntw2", SKINNY | (1 << 26) | (1 << 12) | (2 << 4), (3, 5, 10, 16), 4096, 1024, 128, FRAG.format(2)),
    ("fragment-ntw4", SKINNY | (1 << 12) | (4 << 4) | (2 << 8), (9, 16), 4096, 2048, 128, FRAG.format(4)),
    ("lean-smr", _lean(1, 8), (1, 2, 3, 4), 4096, 512, 128, "lean ntw=1 waves=8"),
    ("lean-mr", _lean(2, 16), (5, 11, 16), 2048, 512, 128, "lean ntw=2 waves=16"),
    ("lean-persist", _lean(1, 8, 2), (2, 16), 2048, 8448, 128, "lean ntw=1 waves=8"),
    ("auto-decode", 0, (1, 4, 16), 4096, 12288, 128, "lean"),
    ("replan-from-xm", 0, (24,), 4096, 8192, 128, "xm"),
]


@pytest.mark.parametrize("small_w", [False, True], ids=["w0.5-1.5", "w0.02-0.1"])
@pytest.mark.parametrize("name,kid,Ms,K,N,G,word", PROLOGUES, ids=[p[0] for p in PROLOGUES])
def test_rmsnorm_prologue_edges_per_row(K_, device, name, kid, Ms, K, N, G, word, small_w):
    ks = 1 if kid & 15 == SKINNY else 0     # (a forced skinny id would split K across workgroups: the prologue needs whole rows)
    for M in Ms:
        plan = K_.plan_describe(M, K, N, G, kid, ks)
        assert plan.startswith(word) and "tiles_per_wave<=0" not in plan, (name, M, plan)
        rng = np.random.default_rng(M * 31 + K + N + small_w)
        x, w, _ = _edge_rows(M, K, rng, small_w)
        iw = rng.integers(0, 16, size=(K, N), dtype=np.uint8)
        z = rng.integers(0, 16, size=(K // G, N), dtype=np.uint8)
        s = rng.uniform(0.005, 0.025, size=(K // G, N)).astype(np.float16)
        packed = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in oracle.pack_mi355x(iw, s, z)]
        xd, wd = torch.from_numpy(x).to(device), torch.from_numpy(w).to(device)
        xn = _rms_ref(x, w, 1e-5)
        ref = xn.astype(np.float64) @ oracle.dequantize(iw, s, z, G).astype(np.float64)
        buf, out = _poisoned(M, N, device)
        y = K_.gemm_forward(xd, *packed, kernel_id=kid, grid_split_k=ks, rmsnorm_weight=wd, rmsnorm_eps=1e-5, out=out)
        _check_guard(buf, M)
        y = y.cpu().numpy()
        assert np.isfinite(ref).all() and np.isfinite(y).all(), (name, M, plan, np.flatnonzero(~np.isfinite(y).all(-1)))
        err = _row_errs(y, ref)
        assert err.max() <= 2e-3, (name, M, plan, int(err.argmax()), float(err.max()))
        # the two-launch path: quick_rmsnorm_f16, then the same kernel
        y2 = K_.gemm_forward(K_.rmsnorm(xd, wd, 1e-5), *packed, kernel_id=kid, grid_split_k=ks).cpu().numpy()
        err2 = _row_errs(y, y2)
        assert err2.max() <= 2e-3, (name, M, plan, int(err2.argmax()), float(err2.max()))
        if name.startswith("table"):
            # x held whole in LDS, normalised with quick_rmsnorm_f16's rounding points: bit-equal to the two launches wherever the sum
            # of squares is exact in any order (the all-zero and the constant rows); elsewhere the two sums, taken in different orders,
            # may round rstd differently, and with it an fp16(x * rstd) here and there
            exact_rows = [m for m in range(M) if _row_kind(m) in (3, 4)]
            assert np.array_equal(y[exact_rows].view(np.uint16), y2[exact_rows].view(np.uint16)), (name, M)


def test_rmsnorm_prologue_residual_and_silu_mul_on_massive_rows(K_, device):
    """The prologue with the decode layer's epilogues (residual in place, SiLU * mul) on the fragment and lean flavours."""
    K, N, G = 4096, 1024, 128
    for kid, ks, M in ((SKINNY | (1 << 12) | (4 << 4) | (2 << 8), 1, 16), (_lean(2, 16), 0, 7), (_lean(1, 8), 0, 2)):
        rng = np.random.default_rng(M)
        x, w, _ = _edge_rows(M, K, rng)
        iw = rng.integers(0, 16, size=(K, N), dtype=np.uint8)
        z = rng.integers(0, 16, size=(K // G, N), dtype=np.uint8)
        s = rng.uniform(0.005, 0.025, size=(K // G, N)).astype(np.float16)
        packed = [torch.from_numpy(np.ascontiguousarray(a)).to(device) for a in oracle.pack_mi355x(iw, s, z)]
        xd, wd = torch.from_numpy(x).to(device), torch.from_numpy(w).to(device)
        y = K_.gemm_forward(xd, *packed, kernel_id=kid, grid_split_k=ks, rmsnorm_weight=wd)
        res = torch.randn(M, N, device=device).half()
        inplace = res.clone()
        K_.gemm_forward(xd, *packed, kernel_id=kid, grid_split_k=ks, rmsnorm_weight=wd, residual=inplace, out=inplace)
        assert torch.equal(inplace, (y.float() + res.float()).half()), kid
        act = K_.gemm_forward(xd, *packed, kernel_id=kid, grid_split_k=ks, rmsnorm_weight=wd, silu_mul=True)
        assert torch.isfinite(act).all() and torch.equal(act, K_.silu_mul(y)), kid


@pytest.mark.parametrize("batch", [1, 5, 16, 64])
def test_decode_step_with_a_massive_residual_channel(K_, device, batch):
    """One Llama-2-7B layer with a massive activation (2e4) planted in one channel of the residual stream and norm weight 4 on that
    channel: the fused decode step (RMSNorm prologues, in-place residual epilogues) stays finite and within 1e-2 of the torch-op step."""
    import dataclasses

    from quick_amd.decoder import CONFIGS, SyntheticDecoder, decode_step_fused, torch_decode_hidden
    cfg = dataclasses.replace(CONFIGS["llama2-7b"], layers=1, vocab=512)
    ma = SyntheticDecoder(cfg, batch=batch, max_len=16, device=device, seed=9)
    mb = SyntheticDecoder(cfg, batch=batch, max_len=16, device=device, seed=9)
    c = 1234
    for m in (ma, mb):
        m.embed[:, c] = 2e4
        for l in m.layers:
            l["ln1"][c] = 4.0
            l["ln2"][c] = 4.0
    ctx = 8
    tokens = torch.randint(0, cfg.vocab, (batch, ctx), device=device)
    ma.forward(tokens, torch.arange(ctx, device=device), None)
    mb.forward(tokens, torch.arange(ctx, device=device), None)
    tok = torch.randint(0, cfg.vocab, (batch,), device=device)
    pos = torch.full((1,), ctx, dtype=torch.int64, device=device)
    mask = torch.full((1, 1, 1, 16), float("-inf"), dtype=torch.float16, device=device)
    mask[..., :ctx + 1] = 0
    _, hid_f = decode_step_fused(mb, tok.view(batch, 1), pos)
    x_ref = torch_decode_hidden(ma, tok.view(batch, 1), pos, mask)
    assert torch.isfinite(x_ref).all() and torch.isfinite(hid_f).all(), batch
    err = (hid_f.float() - x_ref.float()).abs().max() / x_ref.float().abs().max()
    assert err <= 1e-2, (batch, float(err))
