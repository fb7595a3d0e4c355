"""Sliding-window attention over a ring KV cache on the GPU (quick_*_win_f16): the ring write bit for bit against the linear write, the
fused decode step and the MFMA prefill against float64 banded attention (quick_amd.attention.window_attention_reference) within the fp16
kernels' error models restated for the window, exact probes at both edges of the window, the launches against each other, against a
never-wrapping cache and against the existing launches, per-sequence positions, reproducibility against the forcezero twin, and
QuantAttentionFused(sliding_window=...) stage by stage over more than two laps of its ring, a captured decode step included.

Every ring row that holds no position a launch may read is poisoned (NaN keys, +-Inf values) AFTER the fill; outputs land in NaN-poisoned
buffers with guard rows.  Shapes are the smallest at which the kernels can go wrong: rings of 80 .. 128 rows, windows of 1 .. 80."""
import math

import numpy as np
import pytest
import torch

import test_prefill_attention_gpu as PF
from conftest import rel_err
from oracle import w4a16
from quick_amd import QuantAttentionFused, quantize_linear
from quick_amd.attention import ring_rows, ring_slot, window_attention_reference
from test_decode_ops_gpu import _check_guard, _poisoned, _rope_model, _tables

pytestmark = pytest.mark.gpu

D = 128
NP = 1024                      # table_rows: the exclusive bound on positions
U = 2.0 ** -24
SCALE = D ** -0.5
LOG2E = math.log2(math.e)
KV_ROWS = 32                   # positions per tile of the prefill kernel
F32 = torch.float32
DEC_HEADS = [(4, 4), (4, 2), (8, 2), (8, 1)]           # groups 1, 2, 4, 8
# R = 80, W = 40: the first masked row (39 | 40 | 41), the first wrap (79 | 80 | 81), the wrap inside a 16-row chunk (95 | 96), many laps
DEC_P = (0, 15, 16, 39, 40, 41, 79, 80, 81, 95, 96, 159, 160, 1000)
PF_SHAPES = [(96, 32, 65), (128, 64, 65), (80, 40, 17), (80, 80, 1)]      # (R, W, T)
PF_P0 = (0, 31, 32, 90, 96, 500)


@pytest.fixture(scope="module")
def K_(device):
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def tables(device):
    cos_np, sin_np = _tables(NP, 1e4)
    return cos_np, sin_np, torch.from_numpy(cos_np).to(device), torch.from_numpy(sin_np).to(device)


def _i16(t):
    return t.contiguous().view(torch.int16)


def _pos(p, device):
    return torch.full((1,), p, dtype=torch.int64, device=device)


def poison_ring(B, nkv, R, device):
    """A ring nobody has written: NaN keys, +-Inf values."""
    k = torch.full((B, nkv, R, D), float("nan"), dtype=torch.float16, device=device)
    v = torch.full((B, nkv, R, D), float("inf"), dtype=torch.float16, device=device)
    v[:, :, 1::2] = float("-inf")
    return k, v


def fill_ring(k, v, lin_k, lin_v, lo, hi, b=None):
    """Positions lo .. hi (inclusive, fewer than R of them) of the linear streams [B, nkv, NP, D] into their ring rows; every other row of
    the ring keeps what it holds -- the poison."""
    R = k.shape[2]
    assert hi - lo < R
    if hi < lo:
        return
    span = torch.arange(lo, hi + 1, device=k.device)
    sel = slice(None) if b is None else slice(b, b + 1)
    k[sel, :, ring_slot(span, R)] = lin_k[sel, :, span]
    v[sel, :, ring_slot(span, R)] = lin_v[sel, :, span]


def stream(B, nkv, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randn(B, nkv, NP, D, generator=g, device=device).half(), torch.randn(B, nkv, NP, D, generator=g, device=device).half())


def reference_parts(q, k_ring, v_ring, p0, W):
    """What the bounds need, shaped like PF._reference's tuple but over the span max(0, p0 - W + 1) .. p0 + T - 1 gathered out of the ring:
    (qd [B, nkv, g, T, D], Kd, Vd [B, nkv, n, D], vis [T, n], s with -inf where masked, P, ref [B, nkv, g, T, D])."""
    B, nh, T, _ = q.shape
    nkv, R = k_ring.shape[1], k_ring.shape[2]
    lo = max(0, p0 - W + 1)
    span = torch.arange(lo, p0 + T, device=q.device)
    qd = q.double().view(B, nkv, nh // nkv, T, D)
    Kd, Vd = k_ring[:, :, ring_slot(span, R)].double(), v_ring[:, :, ring_slot(span, R)].double()
    qp = p0 + torch.arange(T, device=q.device)[:, None]
    vis = (span[None, :] <= qp) & (span[None, :] > qp - W)
    s = torch.einsum("bkgtd,bknd->bkgtn", qd, Kd) * SCALE
    s = torch.where(vis, s, torch.full_like(s, float("-inf")))
    P = torch.softmax(s, -1)
    ref = torch.einsum("bkgtn,bknd->bkgtd", P, Vd)
    return qd, Kd, Vd, vis, s, P, ref


def rows_to_heads(o, B, T, nkv, g):
    """The kernels' [B * T, nh * D] -> [B, nkv, g, T, D]."""
    return o.view(B, T, nkv, g, D).permute(0, 2, 3, 1, 4)


def prefill_bound_win(qd, Kd, Vd, vis, s, P, ref, p0, W):
    """PF._prefill_bound restated for the window (the kernel keeps that kernel's rounding points): the same terms with NT = the 32-position
    tiles a query's window touches -- the tiles of positions max(0, limit - W + 1) .. limit, limit = pos0 + t; tiles in front of them are
    skipped or pass the query as exact no-ops (max -inf, weights 0), tiles behind them too (rescale by exp2(0) = 1) -- and `seen` = the
    sum of |v| over the rows the query sees."""
    T, n = vis.shape
    lim = p0 + torch.arange(T, device=ref.device)
    NT = (lim // KV_ROWS - (lim - W + 1).clamp_min(0) // KV_ROWS + 1).double()[:, None]
    c = SCALE * LOG2E
    S_abs = torch.einsum("bkgtd,bknd->bkgtn", qd.abs(), Kd.abs()) * c
    s2 = torch.where(vis, s * LOG2E, torch.zeros_like(s))
    m = (s * LOG2E).amax(-1, keepdim=True)
    eta = math.log(2) * (64 * U * S_abs + (NT + 4) * 2 * U * (s2.abs() + m.abs())) + (NT + 2) * 2 * U
    pv = torch.einsum("bkgtn,bknd->bkgtd", P, Vd.abs())
    dev = torch.einsum("bkgtn,bknd->bkgtd", P * eta, Vd.abs()) + (P * eta).sum(-1, keepdim=True) * ref.abs()
    gamma = (43 * NT + 2) * U
    seen = torch.einsum("tn,bknd->bktd", vis.double(), Vd.abs())[:, :, None]
    return PF._ulp16(ref) + (gamma + 2.0 ** -11) * pv + 2.0 ** -25 * seen + dev


def decode_bound_win(qd, Kd, Vd, s, P, ref):
    """PF._decode_bound (= _attention_bound of tests/test_decode_ops_gpu.py) restated for the window: the decode kernel keeps the grouped
    MFMA sweep's rounding points, so the terms are the same with the row and trip counts taken over the n = min(p + 1, W) rows of the
    window (qd [B, nkv, g, D], Kd / Vd [B, nkv, n, D])."""
    return PF._decode_bound(qd, Kd, Vd, Kd.shape[2] - 1, s, P, ref)


def emulate_prefill_win(q, k_ring, v_ring, p0, W):
    """PF._emulate for the windowed kernel, on the CPU: tiles aligned to multiples of 32 LOGICAL positions, the first one the tile of the
    first query's window start; rows outside [that start, pos0 + T - 1] substituted by the nearest row inside, as the staging does (they
    are masked); scores masked on both diagonals by the position.  Returns [B, nkv, g, T, D] float64."""
    q, k_ring, v_ring = q.cpu(), k_ring.cpu(), v_ring.cpu()
    B, nh, T, _ = q.shape
    nkv, R = k_ring.shape[1], k_ring.shape[2]
    qd = q.double().view(B, nkv, nh // nkv, T, D)
    limit = (p0 + torch.arange(T))[:, None]
    lo, last = max(0, p0 - W + 1), p0 + T - 1
    m = torch.full((B, nkv, nh // nkv, T, 1), float("-inf"), dtype=F32)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, nkv, nh // nkv, T, D), dtype=F32)
    c32 = torch.tensor(SCALE, dtype=F32) * torch.tensor(1.44269504088896, dtype=F32)
    for tile0 in range(lo // KV_ROWS * KV_ROWS, last + 1, KV_ROWS):
        j = torch.arange(tile0, tile0 + KV_ROWS)
        rows = ring_slot(j.clamp(lo, last), R)
        x = torch.einsum("bkgtd,bknd->bkgtn", qd, k_ring[:, :, rows].double()).to(F32) * c32
        x = torch.where((j[None, :] <= limit) & (j[None, :] > limit - W), x, torch.full_like(x, float("-inf")))
        mb = torch.maximum(m, x.amax(-1, keepdim=True))
        mref = torch.where(torch.isinf(mb), torch.zeros_like(mb), mb)
        corr = torch.exp2(m - mref)
        e = torch.exp2(x - mref)
        l = l * corr + e.sum(-1, keepdim=True, dtype=F32)
        pv = torch.einsum("bkgtn,bknd->bkgtd", e.half().double(), v_ring[:, :, rows].double())
        acc = ((acc * corr).double() + pv).to(F32)
        m = mb
    return (acc / l).half().double()


def emulate_decode_win(q_rot, Kw, Vw):
    """The decode kernel's rounding points on the CPU over the n rows of the window (index n - 1 = this token), q_rot [B, nkv, g, D], Kw /
    Vw [B, nkv, n, D] fp16: wave w of four takes the 16-index chunks at 16 w + 64 k; in a chunk, row quarter r holds indices 4 r + i.
    Per (wave, quarter): the fp32 score (an fp32 sum of exact products, times scale * log2 e in fp32), the running max over the quarter's
    rows, exp2 and the sum in fp32, the accumulator rescaled once per chunk and P V added row by row in fp32.  Then the kernel's merges:
    the four quarters of a wave, the four waves, one division, one rounding to fp16.  Returns [B, nkv, g, D] float64."""
    q_rot, Kw, Vw = q_rot.cpu(), Kw.cpu(), Vw.cpu()
    n = Kw.shape[2]
    c32 = torch.tensor(SCALE, dtype=F32) * torch.tensor(1.44269504088896, dtype=F32)
    sc_all = torch.einsum("bkgd,bknd->bkgn", q_rot.double(), Kw.double()).to(F32) * c32          # [B, nkv, g, n]
    shape = sc_all.shape[:3]
    ninf = torch.full(shape, float("-inf"), dtype=F32)
    waves = []
    for w in range(4):
        quarters = []
        for r in range(4):
            m, l, acc = ninf.clone(), torch.zeros(shape, dtype=F32), torch.zeros(shape + (D,), dtype=F32)
            for base in range(16 * w, n, 64):
                idx = [base + 4 * r + i for i in range(4) if base + 4 * r + i < n]
                mb = m.clone()
                for i in idx:
                    mb = torch.maximum(mb, sc_all[..., i])
                mref = torch.where(torch.isinf(mb), torch.zeros_like(mb), mb)
                corr = torch.exp2(m - mref)
                l = l * corr
                e = [torch.exp2(sc_all[..., i] - mref) for i in idx]
                for ei in e:
                    l = l + ei
                m = mb
                acc = acc * corr[..., None]
                for ei, i in zip(e, idx):
                    acc = (acc.double() + ei.double()[..., None] * Vw[:, :, None, i].double()).to(F32)
            quarters.append((m, l, acc))
        mw = torch.maximum(torch.maximum(quarters[0][0], quarters[1][0]), torch.maximum(quarters[2][0], quarters[3][0]))
        mwr = torch.where(torch.isinf(mw), torch.zeros_like(mw), mw)
        f = [torch.exp2(qm - mwr) for qm, _, _ in quarters]
        lw = (quarters[0][1] * f[0] + quarters[1][1] * f[1]) + (quarters[2][1] * f[2] + quarters[3][1] * f[3])
        aw = (quarters[0][2] * f[0][..., None] + quarters[1][2] * f[1][..., None]) + (quarters[2][2] * f[2][..., None] + quarters[3][2] * f[3][..., None])
        waves.append((mw, lw, aw))
    M = torch.maximum(torch.maximum(waves[0][0], waves[1][0]), torch.maximum(waves[2][0], waves[3][0]))
    num, den = torch.zeros(shape + (D,), dtype=F32), torch.zeros(shape, dtype=F32)
    for mw, lw, aw in waves:
        f = torch.exp2(mw - M)
        num = (num.double() + aw.double() * f.double()[..., None]).to(F32)
        den = (den.double() + lw.double() * f.double()).to(F32)
    return (num / den[..., None]).half().double()


# ------------------------------------------------------------------------------------------------
# the write
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sequence", [False, True], ids=["shared", "per-sequence"])
@pytest.mark.parametrize("T", [1, 17, 65])
def test_ring_write_equals_the_linear_write_bit_for_bit(K_, device, tables, T, per_sequence):
    """R = 80, pos0 in {0, 70, 79, 80, 200} (a chunk wraps mid-way): the ring rows gathered by ring_slot and q_out equal what
    quick_rope_kv_write_f16 writes into a linear cache of table_rows rows, bit for bit; every other ring row keeps its poison.
    Per-sequence: mixed positions and one skipped slot, whose rows of the ring and of q_out keep their poison."""
    _, _, cos, sin = tables
    B, nh, nkv, R = 3, 8, 2, 80
    for pos0 in (0, 70, 79, 80, 200):
        g = torch.Generator(device=device).manual_seed(100 * pos0 + T)
        qkv = (torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device) * 2).half()
        starts = [pos0, (-1 if pos0 % 2 else NP - T + 1), (pos0 + 37) % (NP - T)] if per_sequence else [pos0] * B
        pos = torch.tensor(starts if per_sequence else starts[:1], dtype=torch.int64, device=device)
        kl = torch.zeros(B, nkv, NP, D, dtype=torch.float16, device=device)
        vl = torch.zeros_like(kl)
        ql = torch.full((B, nh, T, D), 7.0, dtype=torch.float16, device=device)
        K_.rope_kv_write(qkv, cos, sin, pos, ql, kl, vl, T, nh, nkv, D, per_sequence=per_sequence)
        kr, vr = poison_ring(B, nkv, R, device)
        k_want, v_want = kr.clone(), vr.clone()
        qbuf, qr = _poisoned(B, (nh, T, D), device, fill=7.0)
        K_.rope_kv_write(qkv, cos, sin, pos, qr, kr, vr, T, nh, nkv, D, per_sequence=per_sequence, window=40, table_rows=NP)
        torch.cuda.synchronize()
        assert bool((qbuf[0] == 7.0).all()) and bool((qbuf[B + 1] == 7.0).all()), "wrote next to q_out"
        assert PF._bits_equal(qr, ql), (pos0, T, "q_out differs from the linear launch")
        for b, s in enumerate(starts):
            if 0 <= s <= NP - T:
                fill_ring(k_want, v_want, kl, vl, s, s + T - 1, b=b)
            else:
                assert bool((qr[b] == 7.0).all()), "a skipped sequence's q_out was written"
        assert torch.equal(_i16(kr), _i16(k_want)), (pos0, T, per_sequence, "K rows")
        assert torch.equal(_i16(vr), _i16(v_want)), (pos0, T, per_sequence, "V rows")


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def decode_case(B, nh, nkv, R, W, p, seed, device, cos_np, sin_np):
    """qkv of one step at position p and the ring before it: positions max(0, p - W + 1) .. p - 1 of a random stream in their rows, every
    other row (row p % R included) poisoned.  Returns (qkv, k_ring, v_ring, q_rot [B, nh, D], k_rot [B, nkv, D])."""
    g = torch.Generator(device=device).manual_seed(seed)
    qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
    lin_k, lin_v = stream(B, nkv, seed + 1, device)
    kr, vr = poison_ring(B, nkv, R, device)
    fill_ring(kr, vr, lin_k, lin_v, max(0, p - W + 1), p - 1)
    x = qkv.cpu().numpy().reshape(B, nh + 2 * nkv, D)
    q_rot = torch.from_numpy(_rope_model(x[:, :nh], cos_np[p], sin_np[p])).to(device)
    k_rot = torch.from_numpy(_rope_model(x[:, nh:nh + nkv], cos_np[p], sin_np[p])).to(device)
    return qkv, kr, vr, q_rot, k_rot


def decode_check(qkv, kr, vr, kr0, vr0, out, p, W, nh, nkv, q_rot, k_rot, b=None):
    """The ring came back bit for bit except row p % R, which holds the RoPE model's K row and the token's V; out against
    window_attention_reference within decode_bound_win.  Returns max(err / bound)."""
    B, R = qkv.shape[0], kr.shape[2]
    k_want, v_want = kr0.clone(), vr0.clone()
    k_want[:, :, p % R] = k_rot
    v_want[:, :, p % R] = qkv.view(B, nh + 2 * nkv, D)[:, nh + nkv:]
    assert torch.equal(_i16(kr), _i16(k_want)) and torch.equal(_i16(vr), _i16(v_want)), (p, "row p % R / rows outside it")
    q4 = q_rot.view(B, nh, 1, D)
    qd, Kd, Vd, vis, s, P, ref = reference_parts(q4, kr, vr, p, W)
    assert Kd.shape[2] == min(p + 1, W)
    pub = window_attention_reference(q4, kr, vr, p, W).view(B, nkv, nh // nkv, D)
    assert float((pub - ref[:, :, :, 0]).abs().max()) < 1e-12
    bound = decode_bound_win(qd[:, :, :, 0], Kd, Vd, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])
    err = (out.double().view(B, nkv, nh // nkv, D) - pub).abs()
    assert not torch.isnan(err).any(), (p, "NaN in the output: a poisoned row was read")
    return float((err / bound).max())


@pytest.mark.parametrize("nh,nkv", DEC_HEADS, ids=[f"group{a // b}" for a, b in DEC_HEADS])
def test_decode_against_float64_over_the_window(K_, device, tables, nh, nkv):
    """B = 3, R = 80, W = 40, every p of DEC_P: every ring row outside the window (row p % R included) holds NaN keys and +-Inf values."""
    cos_np, sin_np, cos, sin = tables
    B, R, W = 3, 80, 40
    assert K_.window_attention_describe(B, 1, nh, nkv, D, R, W, NP).startswith(f"decode-win-mfma heads={nh // nkv} ")
    for p in DEC_P:
        qkv, kr, vr, q_rot, k_rot = decode_case(B, nh, nkv, R, W, p, 7 * p + nh, device, cos_np, sin_np)
        kr0, vr0 = kr.clone(), vr.clone()
        buf, out = _poisoned(B, (nh * D,), device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kr, vr, out, nh, nkv, D, window=W, table_rows=NP)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        ratio = decode_check(qkv, kr, vr, kr0, vr0, out, p, W, nh, nkv, q_rot, k_rot)
        print(f"[win-decode] {nh}/{nkv} p={p}: max err/bound {ratio:.3f}")
        assert ratio <= 1.0, (nh, nkv, p, ratio)


def test_decode_appends_the_row_the_write_launch_produces(K_, device, tables):
    cos_np, sin_np, cos, sin = tables
    B, nh, nkv, R, W = 3, 8, 2, 80, 40
    for p in (39, 80, 175):
        qkv, kr, vr, _, _ = decode_case(B, nh, nkv, R, W, p, p, device, cos_np, sin_np)
        kw, vw = poison_ring(B, nkv, R, device)
        K_.rope_kv_write(qkv, cos, sin, _pos(p, device), torch.empty(B, nh, 1, D, dtype=torch.float16, device=device), kw, vw, 1, nh, nkv, D,
                         window=W, table_rows=NP)
        out = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kr, vr, out, nh, nkv, D, window=W, table_rows=NP)
        torch.cuda.synchronize()
        assert torch.equal(_i16(kw[:, :, p % R]), _i16(kr[:, :, p % R])) and torch.equal(_i16(vw[:, :, p % R]), _i16(vr[:, :, p % R]))
        assert not torch.isnan(kr[:, :, p % R].float()).any()


# ------------------------------------------------------------------------------------------------
# prefill
# ------------------------------------------------------------------------------------------------
def prefill_case(B, nh, nkv, R, W, T, p0, variant, device):
    """N(0, 1) q and stream; "peaked": K halved and 24 rows per (sequence, KV head) inside the span replaced by beta x a query that sees
    them.  The ring holds positions max(0, p0 - W + 1) .. p0 + T - 1; every other row is poisoned."""
    g = torch.Generator(device=device).manual_seed(1000 * p0 + 10 * T + nh + R + (1 if variant == "peaked" else 0))
    q = torch.randn(B, nh, T, D, generator=g, device=device).half()
    lin_k = torch.randn(B, nkv, NP, D, generator=g, device=device).half()
    lin_v = torch.randn(B, nkv, NP, D, generator=g, device=device).half()
    lo = max(0, p0 - W + 1)
    if variant == "peaked":
        lin_k *= 0.5
        rng = np.random.default_rng(p0 + T + R)
        group = nh // nkv
        for b in range(B):
            for kv in range(nkv):
                for r in rng.choice(np.arange(lo, p0 + T), size=min(24, p0 + T - lo), replace=False):
                    users = [t for t in range(T) if p0 + t - W < r <= p0 + t]
                    t = int(rng.choice(users))
                    h = kv * group + int(rng.integers(0, group))
                    lin_k[b, kv, int(r)] = (q[b, h, t].float() * float(rng.uniform(1.0, 3.5))).half()
    kr, vr = poison_ring(B, nkv, R, device)
    fill_ring(kr, vr, lin_k, lin_v, lo, p0 + T - 1)
    return q, kr, vr


def prefill_launch(K_, q, kr, vr, p0, W, nh, nkv, lib=None, per_sequence=False, pos=None, table_rows=NP):
    """One launch into a poisoned output with guard rows; the ring must come back bit for bit.  Returns out [B * T, nh * D]."""
    B, T = q.shape[0], q.shape[2]
    kr0, vr0 = kr.clone(), vr.clone()
    buf, out = _poisoned(B * T, (nh * D,), q.device)
    pos = _pos(p0, q.device) if pos is None else pos
    if lib is None:
        K_.prefill_attention(q, kr, vr, pos, out, nh, nkv, D, per_sequence=per_sequence, window=W, table_rows=table_rows)
    else:
        rc = lib.quick_prefill_attention_win_f16(q.data_ptr(), kr.data_ptr(), vr.data_ptr(), pos.data_ptr(), out.data_ptr(), B, T, nh, nkv, D,
                                                 kr.shape[2], W, table_rows, SCALE, int(per_sequence), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    _check_guard(buf, B * T)
    assert torch.equal(_i16(kr), _i16(kr0)) and torch.equal(_i16(vr), _i16(vr0)), "the kernel wrote a cache"
    return out


def prefill_ratio(q, kr, vr, p0, W, out):
    """max(err / bound) of a prefill output against window_attention_reference, and the bound (as [B, nkv, g, T, D])."""
    B, nh, T, _ = q.shape
    nkv = kr.shape[1]
    qd, Kd, Vd, vis, s, P, ref = reference_parts(q, kr, vr, p0, W)
    pub = rows_to_heads(window_attention_reference(q, kr, vr, p0, W), B, T, nkv, nh // nkv)
    assert float((pub - ref).abs().max()) < 1e-12
    bound = prefill_bound_win(qd, Kd, Vd, vis, s, P, ref, p0, W)
    err = (rows_to_heads(out.double(), B, T, nkv, nh // nkv) - pub).abs()
    assert not torch.isnan(err).any(), (p0, "NaN in the output: a poisoned row was read")
    return float((err / bound).max()), bound, pub


@pytest.mark.parametrize("nh,nkv", PF.HEADS)
def test_prefill_against_float64_over_the_window(K_, device, nh, nkv):
    """B = 2, every (R, W, T) of PF_SHAPES at every pos0 of PF_P0, random and peaked: max(err / bound) <= 1 with prefill_bound_win; the
    float64 emulation of the rounding points stays inside the same bound."""
    B = 2
    for R, W, T in PF_SHAPES:
        word = "prefill-win-mfma q_rows=64 kv_rows=32 waves=4" if T > 1 else "decode-win-mfma"
        if T > 1 or nh // nkv in (1, 2, 4, 8):
            assert K_.window_attention_describe(B, T, nh, nkv, D, R, W, NP).startswith(word)
        for p0 in PF_P0:
            for variant in ("random", "peaked"):
                q, kr, vr = prefill_case(B, nh, nkv, R, W, T, p0, variant, device)
                out = prefill_launch(K_, q, kr, vr, p0, W, nh, nkv)
                ratio, bound, pub = prefill_ratio(q, kr, vr, p0, W, out)
                emu = float(((emulate_prefill_win(q, kr, vr, p0, W).to(device) - pub).abs() / bound).max())
                print(f"[win-prefill] {nh}/{nkv} R={R} W={W} T={T} pos0={p0} {variant}: max err/bound {ratio:.3f} (emulation {emu:.3f})")
                assert emu <= 1.0, ("the emulation of the rounding points leaves the bound", R, W, T, p0, variant, emu)
                assert ratio <= 1.0, (R, W, T, p0, variant, ratio)


# ------------------------------------------------------------------------------------------------
# exact probes
# ------------------------------------------------------------------------------------------------
def test_window_of_one_returns_each_tokens_own_v_row(K_, device, tables):
    """W = 1: the softmax has one row, its weight is exactly 1: decode returns the new token's V, prefill each token's own V row."""
    cos_np, sin_np, cos, sin = tables
    B, nh, nkv, R = 2, 8, 2, 80
    for p in (0, 79, 80, 333):
        qkv, kr, vr, _, _ = decode_case(B, nh, nkv, R, 1, p, p + 3, device, cos_np, sin_np)
        buf, out = _poisoned(B, (nh * D,), device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kr, vr, out, nh, nkv, D, window=1, table_rows=NP)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        want = qkv.view(B, nh + 2 * nkv, D)[:, nh + nkv:].repeat_interleave(nh // nkv, 1)
        assert PF._bits_equal(out.view(B, nh, D), want), ("decode", p)
    for p0, T in ((0, 65), (70, 17), (500, 65)):
        q, kr, vr = prefill_case(B, nh, nkv, R, 1, T, p0, "random", device)
        out = prefill_launch(K_, q, kr, vr, p0, 1, nh, nkv)
        rows = ring_slot(p0 + torch.arange(T, device=device), R)
        want = vr[:, :, rows].repeat_interleave(nh // nkv, 1).transpose(1, 2).reshape(B * T, nh * D)
        assert PF._bits_equal(out, want), ("prefill", p0, T)


def probe_stream(B, nkv, seed, device):
    """Zero keys, V rows of multiples of 2^-8 in [-1, 1]."""
    g = torch.Generator(device=device).manual_seed(seed)
    lin_k = torch.zeros(B, nkv, NP, D, dtype=torch.float16, device=device)
    lin_v = torch.randint(-256, 257, (B, nkv, NP, D), generator=g, device=device).half() / 256
    return lin_k, lin_v


@pytest.mark.parametrize("nh,nkv", DEC_HEADS, ids=[f"group{a // b}" for a, b in DEC_HEADS])
def test_decode_probes_exact(K_, device, tables, nh, nkv):
    """One-hot queries (512) and keys (4) in the manner of PF._probe_case: a hot score leads every other row by ~261 in the log2 domain,
    every other weight is exactly 0 in fp32.  Hot rows at lo and p (visible) and at lo - 1 -- a finite row still physically in the ring
    (R = 80, W = 40), which must contribute exactly nothing.  The output is the exact mean of the visible hot V rows."""
    _, _, cos, sin = tables
    B, R, W, group = 3, 80, 40, nh // nkv
    for p in DEC_P:
        lo = max(0, p - W + 1)
        lin_k, lin_v = probe_stream(B, nkv, p + nh, "cpu")                  # (built on the host, moved once)
        q = torch.zeros(B, nh, D, dtype=torch.float16)
        want = torch.zeros(B, nh, D, dtype=torch.float64)
        for b in range(B):
            for kv in range(nkv):
                dim = (5 * b + 3 * kv + p) % D
                hot = sorted({lo, p})
                for r in hot + ([lo - 1] if lo >= 1 else []):
                    lin_k[b, kv, r, dim] = 4.0
                q[b, kv * group:(kv + 1) * group, dim] = 512.0
                want[b, kv * group:(kv + 1) * group] = lin_v[b, kv, hot].double().mean(0)
        lin_k, lin_v, q, want = (t.to(device) for t in (lin_k, lin_v, q, want))
        vnew = lin_v[:, :, p].clone()
        kr, vr = poison_ring(B, nkv, R, device)
        fill_ring(kr, vr, lin_k, lin_v, max(0, p - R + 1), p - 1)          # everything still physically in the ring, lo - 1 included
        kr[:, :, p % R], vr[:, :, p % R] = float("nan"), float("nan")
        cos_p, sin_p = cos.clone(), sin.clone()
        cos_p[p], sin_p[p] = 1.0, 0.0                                     # the identity rotation at row p
        qkv = torch.cat([q.view(B, -1), lin_k[:, :, p].reshape(B, -1), vnew.reshape(B, -1)], -1).contiguous()
        buf, out = _poisoned(B, (nh * D,), device)
        K_.rope_attention(qkv, cos_p, sin_p, _pos(p, device), kr, vr, out, nh, nkv, D, window=W, table_rows=NP)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        assert torch.equal(want.half().double(), want)
        bad = (out.view(B, nh, D).double() != want).any(-1)
        assert not bool(bad.any()), (p, bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("nh,nkv", PF.HEADS)
def test_prefill_probes_exact(K_, device, nh, nkv):
    """As above, per query t of a chunk: hot rows at its lo and its own position (visible), at lo - 1 (for t >= 1 a row inside the
    workgroup's span, requested and masked by the lower diagonal) and at the position one behind the query (the causal decoy)."""
    B = 2
    group = nh // nkv
    for R, W, T in ((96, 32, 33), (80, 40, 17), (128, 64, 64)):
        for p0 in PF_P0:
            lin_k, lin_v = probe_stream(B, nkv, p0 + T + nh, "cpu")         # (built on the host, moved once)
            q = torch.zeros(B, nh, T, D, dtype=torch.float16)
            want = torch.zeros(B, T, nh, D, dtype=torch.float64)
            for b in range(B):
                for kv in range(nkv):
                    for t in range(T):
                        dim = (t + 7 * b + 3 * kv) % D          # (T <= 64 < D: one dimension per token of a KV head)
                        pt = p0 + t
                        lo = max(0, pt - W + 1)
                        hot = sorted({lo, pt})
                        cold = [r for r in (lo - 1, pt + 1) if max(0, p0 - W + 1) <= r <= p0 + T - 1]
                        for r in hot + cold:
                            lin_k[b, kv, r, dim] = 4.0
                        q[b, kv * group:(kv + 1) * group, t, dim] = 512.0
                        want[b, t, kv * group:(kv + 1) * group] = lin_v[b, kv, hot].double().mean(0)
            lin_k, lin_v, q, want = (t.to(device) for t in (lin_k, lin_v, q, want))
            kr, vr = poison_ring(B, nkv, R, device)
            fill_ring(kr, vr, lin_k, lin_v, max(0, p0 - W + 1), p0 + T - 1)
            ref = window_attention_reference(q, kr, vr, p0, W)
            assert torch.equal(ref.half().double(), want.view(B * T, nh * D)), "the probe's closed form is not softmax . V"
            out = prefill_launch(K_, q, kr, vr, p0, W, nh, nkv)
            bad = (out.double().view(B, T, nh, D) != want).any(-1)
            assert not bool(bad.any()), (R, W, T, p0, bad.nonzero()[:6].tolist())


# ------------------------------------------------------------------------------------------------
# cross-checks
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv", DEC_HEADS, ids=[f"group{a // b}" for a, b in DEC_HEADS])
def test_single_token_prefill_agrees_with_decode_on_the_same_ring(K_, device, tables, nh, nkv):
    """The decode step appends row p % R and attends its window; a T = 1 prefill of the same rotated query over the ring it left agrees
    within the sum of both bounds."""
    cos_np, sin_np, cos, sin = tables
    B, R, W = 3, 80, 40
    for p in (0, 39, 40, 79, 80, 96, 1000):
        qkv, kr, vr, q_rot, _ = decode_case(B, nh, nkv, R, W, p, 11 * p + nh, device, cos_np, sin_np)
        dec = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kr, vr, dec, nh, nkv, D, window=W, table_rows=NP)
        q = q_rot.view(B, nh, 1, D).contiguous()
        out = prefill_launch(K_, q, kr, vr, p, W, nh, nkv)
        qd, Kd, Vd, vis, s, P, ref = reference_parts(q, kr, vr, p, W)
        bound = prefill_bound_win(qd, Kd, Vd, vis, s, P, ref, p, W)[:, :, :, 0] + \
            decode_bound_win(qd[:, :, :, 0], Kd, Vd, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])
        diff = (out.double().view(B, nkv, nh // nkv, D) - dec.double().view(B, nkv, nh // nkv, D)).abs()
        assert float((diff / bound).max()) <= 1.0, (p, float((diff / bound).max()))


def test_ring_agrees_with_a_never_wrapping_cache(K_, device, tables):
    """The same token stream and the same W on a ring (R = 96) and on a cache that can never wrap (R = table_rows): prefill chunks and
    decode steps agree within twice the bound."""
    cos_np, sin_np, cos, sin = tables
    B, nh, nkv, R, W, T = 2, 8, 2, 96, 32, 65
    for p0 in (0, 90, 500):
        g = torch.Generator(device=device).manual_seed(p0)
        q = torch.randn(B, nh, T, D, generator=g, device=device).half()
        lin_k, lin_v = stream(B, nkv, p0 + 5, device)
        lo = max(0, p0 - W + 1)
        kr, vr = poison_ring(B, nkv, R, device)
        kn, vn = poison_ring(B, nkv, NP, device)
        fill_ring(kr, vr, lin_k, lin_v, lo, p0 + T - 1)
        fill_ring(kn, vn, lin_k, lin_v, lo, p0 + T - 1)
        a = prefill_launch(K_, q, kr, vr, p0, W, nh, nkv)
        b = prefill_launch(K_, q, kn, vn, p0, W, nh, nkv)
        _, bound, _ = prefill_ratio(q, kr, vr, p0, W, a)
        diff = (rows_to_heads(a.double(), B, T, nkv, nh // nkv) - rows_to_heads(b.double(), B, T, nkv, nh // nkv)).abs()
        assert float((diff / (2 * bound)).max()) <= 1.0, ("prefill", p0)
        # a decode step behind the chunk
        p = p0 + T
        qkv, kr, vr, q_rot, k_rot = decode_case(B, nh, nkv, R, W, p, p, device, cos_np, sin_np)
        lin_k, lin_v = stream(B, nkv, p + 1, device)                       # (decode_case's stream)
        kn, vn = poison_ring(B, nkv, NP, device)
        fill_ring(kn, vn, lin_k, lin_v, max(0, p - W + 1), p - 1)
        outs = []
        for kc, vc in ((kr, vr), (kn, vn)):
            o = torch.empty(B, nh * D, dtype=torch.float16, device=device)
            K_.rope_attention(qkv, cos, sin, _pos(p, device), kc, vc, o, nh, nkv, D, window=W, table_rows=NP)
            outs.append(o.double().view(B, nkv, nh // nkv, D))
        torch.cuda.synchronize()
        qd, Kd, Vd, vis, s, P, ref = reference_parts(q_rot.view(B, nh, 1, D), kr, vr, p, W)
        bound = decode_bound_win(qd[:, :, :, 0], Kd, Vd, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])
        assert float(((outs[0] - outs[1]).abs() / (2 * bound)).max()) <= 1.0, ("decode", p)


def test_a_window_that_covers_everything_agrees_with_the_existing_launches(K_, device, tables):
    """W >= p + 1 on a never-wrapping cache (R = table_rows = 512): the windowed launches agree with quick_prefill_attention_f16 and
    quick_decode_rope_attention_f16 on the same linear cache within the sum of the bounds."""
    cos_np, sin_np, cos, sin = tables
    B, nh, nkv, L, W = 2, 8, 2, 512, 256
    cos_l, sin_l = cos[:L].contiguous(), sin[:L].contiguous()
    for p0, T in ((0, 65), (100, 65), (190, 17)):
        q, kc, vc = PF._dense_case(B, nh, nkv, p0, T, "random", device)
        a = prefill_launch(K_, q, kc, vc, p0, W, nh, nkv, table_rows=L)
        b = PF._launch(K_, q, kc, vc, p0, nh, nkv)
        qd, Kd, Vd, vis, s, P, ref = PF._reference(q, kc, vc, p0)
        bound = PF._prefill_bound(qd, Kd, Vd, vis, s, P, ref, p0) + \
            prefill_bound_win(*reference_parts(q, kc, vc, p0, W), p0, W)
        diff = (rows_to_heads(a.double(), B, T, nkv, nh // nkv) - rows_to_heads(b.double(), B, T, nkv, nh // nkv)).abs()
        assert float((diff / bound).max()) <= 1.0, ("prefill", p0, T)
    for p in (0, 63, 64, 255):
        g = torch.Generator(device=device).manual_seed(p)
        qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
        kc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
        vc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
        PF._fill_behind(kc, vc, p)
        outs = []
        for kw in (dict(window=W, table_rows=L), {}):
            k1, v1 = kc.clone(), vc.clone()
            o = torch.empty(B, nh * D, dtype=torch.float16, device=device)
            K_.rope_attention(qkv, cos_l, sin_l, _pos(p, device), k1, v1, o, nh, nkv, D, **kw)
            outs.append((o.double().view(B, nkv, nh // nkv, D), k1, v1))
        torch.cuda.synchronize()
        assert torch.equal(_i16(outs[0][1]), _i16(outs[1][1])) and torch.equal(_i16(outs[0][2]), _i16(outs[1][2])), (p, "the caches differ")
        q_rot = torch.from_numpy(_rope_model(qkv.cpu().numpy().reshape(B, nh + 2 * nkv, D)[:, :nh], cos_np[p], sin_np[p])).to(device)
        qd, Kd, Vd, vis, s, P, ref = reference_parts(q_rot.view(B, nh, 1, D), outs[0][1], outs[0][2], p, W)
        bound = 2 * decode_bound_win(qd[:, :, :, 0], Kd, Vd, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])
        assert float(((outs[0][0] - outs[1][0]).abs() / bound).max()) <= 1.0, ("decode", p)


# ------------------------------------------------------------------------------------------------
# per-sequence positions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nh,nkv", [(4, 2), (8, 1)], ids=["group2", "group8"])
def test_per_sequence_launches_equal_the_shared_launch_and_skip(K_, device, tables, nh, nkv):
    """Mixed positions on both sides of the wrap and one sequence out of range: a skipped sequence's rows of out and of the ring keep their
    poison; every other sequence's results equal the shared launch at its position bit for bit."""
    cos_np, sin_np, cos, sin = tables
    R, W = 80, 40
    for positions in ((79, -1, 80), (NP, 15, 1000), (41, 160, NP - 1)):
        B = len(positions)
        qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=torch.Generator(device=device).manual_seed(sum(positions)), device=device).half()
        kr, vr = poison_ring(B, nkv, R, device)
        for b, p in enumerate(positions):
            if 0 <= p < NP:
                lin_k, lin_v = stream(B, nkv, p, device)
                fill_ring(kr, vr, lin_k, lin_v, max(0, p - W + 1), p - 1, b=b)
        kr0, vr0 = kr.clone(), vr.clone()
        out = torch.full((B, nh * D), 7.0, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, torch.tensor(positions, dtype=torch.int64, device=device), kr, vr, out, nh, nkv, D,
                          per_sequence=True, window=W, table_rows=NP)
        torch.cuda.synchronize()
        for b, p in enumerate(positions):
            if not 0 <= p < NP:
                assert bool((out[b] == 7.0).all()), "a skipped sequence's out was written"
                assert torch.equal(_i16(kr[b]), _i16(kr0[b])) and torch.equal(_i16(vr[b]), _i16(vr0[b])), "a skipped sequence's ring changed"
                continue
            k1, v1 = kr0[b:b + 1].clone(), vr0[b:b + 1].clone()
            one = torch.empty(1, nh * D, dtype=torch.float16, device=device)
            K_.rope_attention(qkv[b:b + 1].contiguous(), cos, sin, _pos(p, device), k1, v1, one, nh, nkv, D, window=W, table_rows=NP)
            torch.cuda.synchronize()
            assert PF._bits_equal(out[b:b + 1], one), ("decode", p)
            assert torch.equal(_i16(kr[b:b + 1]), _i16(k1)) and torch.equal(_i16(vr[b:b + 1]), _i16(v1)), ("decode ring", p)
    T = 17
    for starts in ((70, NP - T + 1, 200), (-1, 0, 64)):
        B = len(starts)
        q = torch.randn(B, nh, T, D, generator=torch.Generator(device=device).manual_seed(sum(starts) + 9), device=device).half()
        kr, vr = poison_ring(B, nkv, R, device)
        for b, s in enumerate(starts):
            if 0 <= s <= NP - T:
                lin_k, lin_v = stream(B, nkv, s + 1, device)
                fill_ring(kr, vr, lin_k, lin_v, max(0, s - W + 1), s + T - 1, b=b)
        kr0, vr0 = kr.clone(), vr.clone()
        out = torch.full((B * T, nh * D), 7.0, dtype=torch.float16, device=device)
        K_.prefill_attention(q, kr, vr, torch.tensor(starts, dtype=torch.int64, device=device), out, nh, nkv, D, per_sequence=True,
                             window=W, table_rows=NP)
        torch.cuda.synchronize()
        assert torch.equal(_i16(kr), _i16(kr0)) and torch.equal(_i16(vr), _i16(vr0)), "the kernel wrote a cache"
        for b, s in enumerate(starts):
            if not 0 <= s <= NP - T:
                assert bool((out[b * T:(b + 1) * T] == 7.0).all()), "a skipped sequence's rows were written"
                continue
            one = prefill_launch(K_, q[b:b + 1].contiguous(), kr[b:b + 1].contiguous(), vr[b:b + 1].contiguous(), s, W, nh, nkv)
            assert PF._bits_equal(out[b * T:(b + 1) * T], one), ("prefill", s)


# ------------------------------------------------------------------------------------------------
# reproducibility
# ------------------------------------------------------------------------------------------------
def test_window_launches_are_reproducible_and_equal_their_forcezero_build(K_, device, tables):
    """Write, decode (every group) and prefill: two launches give bit-equal results, and so does the -amdgpu-waitcnt-forcezero build."""
    from quick_amd import _lib
    from quick_amd.build import FORCEZERO_LIB
    other = _lib.load_other(FORCEZERO_LIB)
    cos_np, sin_np, cos, sin = tables
    st = torch.cuda.current_stream().cuda_stream
    R, W = 80, 40
    for nh, nkv in DEC_HEADS:
        B, p = 2, 175
        qkv, kr, vr, _, _ = decode_case(B, nh, nkv, R, W, p, nh + nkv, device, cos_np, sin_np)
        pos = _pos(p, device)
        got = []
        for lib in (_lib.load(), _lib.load(), other):
            k1, v1 = kr.clone(), vr.clone()
            out = torch.empty(B, nh * D, dtype=torch.float16, device=device)
            rc = lib.quick_decode_rope_attention_win_f16(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), k1.data_ptr(),
                                                         v1.data_ptr(), out.data_ptr(), B, nh, nkv, D, R, W, NP, SCALE, 0, st)
            assert rc == 0, rc
            torch.cuda.synchronize()
            got.append((out, k1, v1))
        for run in got[1:]:
            for a, b in zip(got[0], run):
                assert torch.equal(_i16(a), _i16(b)), (nh, nkv, "decode: launches / forcezero build differ")
    B, nh, nkv, T = 2, 8, 2, 17
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=torch.Generator(device=device).manual_seed(3), device=device).half()
    pos = _pos(70, device)
    got = []
    for lib in (_lib.load(), _lib.load(), other):
        k1, v1 = poison_ring(B, nkv, R, device)
        q1 = torch.empty(B, nh, T, D, dtype=torch.float16, device=device)
        rc = lib.quick_rope_kv_write_win_f16(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), q1.data_ptr(), k1.data_ptr(),
                                             v1.data_ptr(), B, T, nh, nkv, D, R, NP, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        got.append((q1, k1, v1))
    for run in got[1:]:
        for a, b in zip(got[0], run):
            assert torch.equal(_i16(a), _i16(b)), "write: launches / forcezero build differ"
    for (nh, nkv), (R, W, T), p0 in zip(PF.HEADS, PF_SHAPES[:3], (90, 500, 70)):
        q, kr, vr = prefill_case(2, nh, nkv, R, W, T, p0, "random", device)
        a = prefill_launch(K_, q, kr, vr, p0, W, nh, nkv)
        b = prefill_launch(K_, q, kr, vr, p0, W, nh, nkv)
        z = prefill_launch(K_, q, kr, vr, p0, W, nh, nkv, lib=other)
        assert PF._bits_equal(a, b), (nh, nkv, p0, T, "two launches differ")
        assert PF._bits_equal(a, z), (nh, nkv, p0, T, "the forcezero build differs")


# ------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------
TOL = 2e-3      # the existing module tests' o_proj tolerance (tests/test_attention_module_gpu.py)
MAXLEN, WIN, CHUNK = 256, 40, 24
RING = 63       # ring_rows(40, 24, 256)
# a 24-token chunk, then single steps and chunks: 188 tokens = two laps of the ring and 62 -- the next two steps cross the third wrap
CALLS = (24, 1, 1, 24, 1, 17, 24, 1, 24, 5, 1, 24, 24, 17)
RAGGED = {24: [24, 20], 17: [9, 17], 5: [5, 3]}


def _module(hidden, nh, nkv, device, per_sequence, monkeypatch, **kw):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "2")
    g = torch.Generator().manual_seed(hidden + nkv)
    lin = lambda n_out: torch.nn.Linear(hidden, n_out, bias=False, dtype=torch.float16)
    qkv_lin, o_lin = lin((nh + 2 * nkv) * D), lin(hidden)
    qkv_lin.weight.data = (torch.randn(qkv_lin.weight.shape, generator=g) * 0.06).half()
    o_lin.weight.data = (torch.randn(o_lin.weight.shape, generator=g) * 0.04).half()
    qkv, o = quantize_linear(qkv_lin, 4, 128).to(device), quantize_linear(o_lin, 4, 128).to(device)
    o_logical = w4a16.unpack_mi355x(*[t.cpu().numpy() for t in (o.qweight, o.scales, o.qzeros)])
    m = QuantAttentionFused(hidden, nh, nkv, qkv, o, device, MAXLEN, per_sequence=per_sequence, **kw)
    x = torch.randn(2, sum(CALLS) + 19, hidden, generator=g).half().to(device)
    return m, o_logical, x


class _Model:
    """The torch model of the windowed module: per sequence its position and the rows of every position it has written (a linear record,
    [B, nkv, MAXLEN + CHUNK, D]) from the RoPE model of the module's own qkv output."""

    def __init__(self, m, B):
        self.m, self.pos = m, [0] * B
        self.k = torch.zeros(B, m.n_kv_heads, MAXLEN + CHUNK, D, dtype=torch.float16, device=m.k_cache.device)
        self.v = torch.zeros_like(self.k)

    def step(self, qkv, counts, attention_weight, attn_output, o_logical):
        m, dev = self.m, qkv.device
        nh, nkv = m.n_heads, m.n_kv_heads
        B, T = len(counts), qkv.shape[0] // len(counts)
        qkv = qkv.view(B, T, nh + 2 * nkv, D)
        worst = 0.0
        for b in range(B):
            p0, n = self.pos[b], counts[b]
            c, s = (t[p0:p0 + T].cpu().numpy()[:, None] for t in (m.cos, m.sin))
            rows = qkv[b].cpu().numpy()
            q_rot = torch.from_numpy(_rope_model(rows[:, :nh], c, s)).to(dev).transpose(0, 1).contiguous()[None]          # [1, nh, T, D]
            self.k[b, :, p0:p0 + T] = torch.from_numpy(_rope_model(rows[:, nh:nh + nkv], c, s)).to(dev).transpose(0, 1)
            self.v[b, :, p0:p0 + T] = qkv[b, :, nh + nkv:].transpose(0, 1)
            # the module's ring: every position a query of this call attends, and the padding behind them, in its row
            span = torch.arange(max(0, p0 - WIN + 1), p0 + T, device=dev)
            assert torch.equal(_i16(m.k_cache[b][:, ring_slot(span, RING)]), _i16(self.k[b][:, span])), (b, p0, T, "K rows")
            assert torch.equal(_i16(m.v_cache[b][:, ring_slot(span, RING)]), _i16(self.v[b][:, span])), (b, p0, T, "V rows")
            if n:
                q1, k1, v1 = q_rot[:, :, :n].contiguous(), m.k_cache[b:b + 1], m.v_cache[b:b + 1]
                ref = rows_to_heads(window_attention_reference(q1, k1, v1, p0, WIN), 1, n, nkv, nh // nkv)
                qd, Kd, Vd, vis, sc, P, ref2 = reference_parts(q1, k1, v1, p0, WIN)
                if T > 1:
                    bound = prefill_bound_win(qd, Kd, Vd, vis, sc, P, ref2, p0, WIN)
                else:
                    bound = decode_bound_win(qd[:, :, :, 0], Kd, Vd, sc[:, :, :, 0], P[:, :, :, 0], ref2[:, :, :, 0])[:, :, :, None]
                got = rows_to_heads(attention_weight[b, :n].double().reshape(n, nh * D), 1, n, nkv, nh // nkv)
                worst = max(worst, float(((got - ref).abs() / bound).max()))
                want = attention_weight[b, :n].double().cpu().numpy() @ w4a16.dequantize(*o_logical, 128).astype(np.float64)
                err = rel_err(attn_output[b, :n].float().cpu().numpy(), want)
                assert err <= TOL, (b, p0, T, err)
            self.pos[b] += n
        return worst


@pytest.mark.parametrize("per_sequence", [False, True], ids=["shared", "per-sequence"])
@pytest.mark.parametrize("hidden,nh,nkv", [(512, 4, 4), (512, 4, 2)], ids=["group1", "group2"])
def test_module_with_a_sliding_window_stage_by_stage(device, monkeypatch, hidden, nh, nkv, per_sequence):
    """sliding_window = 40, prefill_chunk = 24, max_seq_len = 256: a ring of 63 rows.  A 24-token chunk, then single steps and chunks to
    beyond two laps (per_sequence: ragged new_tokens, the sequences on different laps).  Every call: the ring rows of every attended
    position equal the RoPE model's rows of the module's own qkv output, the attention in front of o_proj is within the kernels' bounds
    of window_attention_reference over the module's ring, o_proj within 2e-3 of the oracle's GEMM.  Then one decode step captured in a
    graph and replayed twice, across the wrap of the ring, against eager steps.  A 25-token chunk and position 256 raise."""
    m, o_logical, x = _module(hidden, nh, nkv, device, per_sequence, monkeypatch, sliding_window=WIN, prefill_chunk=CHUNK)
    assert ring_rows(WIN, CHUNK, MAXLEN) == RING and tuple(m.k_cache.shape) == (2, nkv, RING, D) == tuple(m.v_cache.shape)
    assert m.cos.shape[0] == MAXLEN
    B = 2
    model = _Model(m, B)
    with pytest.raises(ValueError, match="prefill_chunk"):
        m(x[:, :CHUNK + 1])
    at = bound_pos = 0
    # (per_sequence: a last chunk that sequence 0 alone takes -- sequence 1 idles on its own lap -- brings it to position 188 too)
    for T, counts in [(T, RAGGED.get(T, [T] * B) if per_sequence else [T] * B) for T in CALLS] + ([(16, [16, 0])] if per_sequence else []):
        seen = []
        hook = m.qkv_proj.register_forward_hook(lambda mod, inp, out: seen.append(out))
        try:
            kw = dict(new_tokens=counts) if per_sequence else {}
            attn_output, attention_weight, past = m(x[:, at:at + T], **kw)
        finally:
            hook.remove()
        torch.cuda.synchronize()
        ratio = model.step(seen[0], counts, attention_weight, attn_output, o_logical)
        print(f"[win-module] {nh}/{nkv} per_sequence={per_sequence} T={T} at {model.pos}: attention err/bound {ratio:.3f}")
        assert ratio <= 1.0, (T, ratio)
        assert m.pos.tolist() == (model.pos if per_sequence else model.pos[:1])
        bound_pos += max(counts)
        assert tuple(past[0].shape) == (1, 1, m.start_pos, 1) and m.start_pos == bound_pos
        at += T
    assert model.pos[0] == 188 and model.pos[0] % RING == RING - 1        # the next step writes the last row of the ring, the one after row 0
    # a captured decode step, replayed twice; the same module runs the same two steps eagerly from the same state
    xs = x[:, at - 1:at + 2].contiguous()
    static = xs[:, :1].clone()
    state = (m.pos.clone(), m.k_cache.clone(), m.v_cache.clone(), m.start_pos)

    def restore():
        m.pos.copy_(state[0])
        m.k_cache.copy_(state[1])
        m.v_cache.copy_(state[2])
        m.start_pos = state[3]
    eager = []
    for i in (1, 2):
        eager.append(m(xs[:, i:i + 1].contiguous())[0].clone())
    k_eager, v_eager, pos_eager = m.k_cache.clone(), m.v_cache.clone(), m.pos.clone()
    restore()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m(static)                                          # warm-up outside the capture (workspaces)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_static = m(static)[0]
    restore()                                              # (capture executes nothing, but advances the host-side bound)
    torch.cuda.synchronize()
    for i in (1, 2):
        static.copy_(xs[:, i:i + 1])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_i16(out_static), _i16(eager[i - 1])), ("replay", i)
    assert torch.equal(m.pos, pos_eager) and torch.equal(_i16(m.k_cache), _i16(k_eager)) and torch.equal(_i16(m.v_cache), _i16(v_eager))
    # the position bound is max_seq_len, as without a window
    m.start_pos = MAXLEN
    with pytest.raises(ValueError, match="max_seq_len"):
        m(x[:, :1])


def test_a_default_module_issues_the_existing_launches(device, monkeypatch):
    """sliding_window=None: the module calls the kernels entry points with the arguments it always passed (no window, no table_rows) on
    caches of max_seq_len rows, and returns what a second default module returns, bit for bit."""
    from quick_amd import kernels
    m, _, x = _module(512, 4, 2, device, False, monkeypatch)
    m2, _, _ = _module(512, 4, 2, device, False, monkeypatch)
    assert m.sliding_window is None and tuple(m.k_cache.shape) == (2, 2, MAXLEN, D)
    want = [m2(x[:, :19])[0], m2(x[:, 19:20])[0]]
    calls = []
    for name in ("rope_attention", "rope_kv_write", "prefill_attention"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, (lambda real, name: lambda *a, **kw: (calls.append((name, len(a), dict(kw))), real(*a, **kw))[1])(real, name))
    got = [m(x[:, :19])[0], m(x[:, 19:20])[0]]
    torch.cuda.synchronize()
    assert calls == [("rope_kv_write", 11, {}), ("prefill_attention", 8, {}), ("rope_attention", 10, {})], calls
    for a, b in zip(got, want):
        assert torch.equal(_i16(a), _i16(b))
