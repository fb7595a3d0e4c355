"""quick_prefill_attention_f16 (causal attention of T new tokens over the KV cache) against exact and float64 models.  Needs an MI355X.

Probes: one-hot queries (512) and keys (4) make every score one exact product (2048 or 0); the hot rows lead every other row by ~261 in
the log2 domain, so every other weight is exp2 of less than -149: exactly 0 in fp32, and a hot weight is exactly 1 (also as fp16).  With V
rows of multiples of 2^-8 and 1, 2 or 4 visible hot rows per query the output is exactly their mean.  Dense: N(0, 1) and peaked data
against float64 causal softmax . V within the error model stated at _prefill_bound, which a float64 emulation of the kernel's rounding
points (_emulate) must meet as well.  Rows at or behind pos0 + T hold NaN keys and +-Inf values; outputs land in NaN-poisoned buffers
with guard rows; the caches must come back bit for bit.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
L = 512
U = 2.0 ** -24     # fp32 unit roundoff
SCALE = D ** -0.5
LOG2E = math.log2(math.e)
KV_ROWS = 32       # cache rows per tile of the kernel
WAVE_ROWS = 16     # query rows per wave
WG_ROWS = 64       # query rows per workgroup
WORD = "prefill-mfma q_rows=64 kv_rows=32 waves=4"
HEADS = [(4, 4), (8, 2), (8, 1)]


@pytest.fixture(scope="module")
def K_(device):
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


def _poisoned(rows, tail, device, fill=float("nan"), dtype=torch.float16):
    """Output buffer for rows 1..rows of a [rows + 2, *tail] tensor filled with `fill`: every element must be written and nothing next to it."""
    buf = torch.full((rows + 2,) + tuple(tail), fill, dtype=dtype, device=device)
    return buf, buf[1:rows + 1]


def _check_guard(buf, rows):
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[rows + 1]).all(), "wrote next to the output"
    assert not torch.isnan(buf[1:rows + 1]).any(), "left output elements unwritten"


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _ulp16(a):
    """Spacing of fp16 at |a| (float64 tensor): 2^(e - 10) in the normal range, 2^-24 below it."""
    e = torch.floor(torch.log2(a.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _fill_behind(kc, vc, n):
    """Rows n.. of a real cache are unwritten: NaN keys, +-Inf values."""
    kc[:, :, n:] = float("nan")
    vc[:, :, n:] = float("inf")
    vc[:, :, n + 1::2] = float("-inf")


def _launch(K_, q, kc, vc, p0, nh, nkv, lib=None):
    """One launch into a poisoned output with guard rows; the caches must come back bit for bit.  Returns out [B * T, nh * D]."""
    B, T = q.shape[0], q.shape[2]
    kc0, vc0 = kc.clone(), vc.clone()
    buf, out = _poisoned(B * T, (nh * D,), q.device)
    pos = torch.full((1,), p0, dtype=torch.int64, device=q.device)
    if lib is None:
        K_.prefill_attention(q, kc, vc, pos, out, nh, nkv, D)
    else:
        rc = lib.quick_prefill_attention_f16(q.data_ptr(), kc.data_ptr(), vc.data_ptr(), pos.data_ptr(), out.data_ptr(), B, T, nh, nkv, D,
                                             kc.shape[2], SCALE, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    _check_guard(buf, B * T)
    assert _bits_equal(kc, kc0) and _bits_equal(vc, vc0), "the kernel wrote a cache"
    return out


def _reference(q, kc, vc, p0):
    """float64 causal softmax . V of fp16 inputs: q [B, nh, T, D], caches [B, nkv, >= p0 + T, D].  Returns (qd [B, nkv, g, T, D], Kd, Vd
    [B, nkv, n, D], vis [T, n], s [B, nkv, g, T, n] in nats with -inf where masked, P, ref [B, nkv, g, T, D])."""
    B, nh, T, _ = q.shape
    nkv, n = kc.shape[1], p0 + T
    qd = q.double().view(B, nkv, nh // nkv, T, D)
    Kd, Vd = kc[:, :, :n].double(), vc[:, :, :n].double()
    vis = torch.arange(n, device=q.device)[None, :] <= (p0 + torch.arange(T, device=q.device))[:, None]
    s = torch.einsum("bkgtd,bknd->bkgtn", qd, Kd) * SCALE
    s = torch.where(vis, s, torch.full_like(s, float("-inf")))
    P = torch.softmax(s, -1)
    ref = torch.einsum("bkgtn,bknd->bkgtd", P, Vd)
    return qd, Kd, Vd, vis, s, P, ref


def _rows_out(o, B, T, nh):
    """[B, nkv, g, T, D] (or [B, nh, T, D]) -> the kernel's [B * T, nh * D]."""
    return o.reshape(B, nh, T, D).transpose(1, 2).reshape(B * T, nh * D)


# ------------------------------------------------------------------------------------------------
# exact probes
# ------------------------------------------------------------------------------------------------
def _probe_case(B, nh, nkv, p0, T, seed):
    """One-hot queries, (multi-)hot keys.  Within a (sequence, KV head), the queries of the heads h with h % nsets == s share a family of
    dimensions; dimension number i of the family is the query dimension of tokens t = i, i + n3, i + 2 n3 (n3 = ceil(T / 3)), which see 1, 2
    and 4 hot rows: a base row among the rows the kernel can get wrong (row 0, both sides of every 32-row K/V tile, of every 16-row wave
    and 64-row workgroup boundary of the chunk, pos0 + t - 1, pos0 + t); then the DECOY of the first token, row pos0 + t + 1 -- hot in its
    dimension, inside the chunk, finite, invisible to it and visible to the second; then the second's decoy and one row more (the third
    token's own row or the one before).  Every query with t + 1 < T has its decoy.  Returns fp16 q [B, nh, T, D], caches [B, nkv, L, D] with
    NaN keys and +-Inf values from row pos0 + T on, and the exact expectation [B * T, nh * D] in float64."""
    rng = np.random.default_rng(seed)
    group = nh // nkv
    nsets = min(group, 2)
    nd = D // nsets
    n3 = -(-T // 3)
    assert n3 <= nd and (n3 > 2 or T <= 2)
    q = np.zeros((B, nh, T, D), np.float16)
    kc = np.zeros((B, nkv, L, D), np.float16)
    vc = (rng.integers(-256, 257, (B, nkv, L, D)) / 256).astype(np.float16)
    want = np.zeros((B, T, nh, D), np.float64)
    edges = {0, p0 - 1, p0}
    edges |= {r + e for r in range(KV_ROWS, p0 + T, KV_ROWS) for e in (-1, 0)}
    edges |= {p0 + r + e for r in range(WAVE_ROWS, T, WAVE_ROWS) for e in (-1, 0)}
    for b in range(B):
        for kv in range(nkv):
            v64 = vc[b, kv].astype(np.float64)
            for s in range(nsets):
                heads = [kv * group + g for g in range(group) if g % nsets == s]
                for i in range(n3):
                    dim = s * nd + (5 * i + b + 3 * kv) % nd
                    users = [t for t in (i, i + n3, i + 2 * n3) if t < T]
                    t0 = users[0]
                    cands = sorted(r for r in edges | {p0 + t0 - 1, p0 + t0} if 0 <= r <= p0 + t0)
                    rows = [cands[(i + 2 * b + kv + 3 * s) % len(cands)]]
                    for c, t in enumerate(users):
                        if c == 2:
                            extra = p0 + t - (i % 2)                 # the third token's own row, or the one before
                            assert extra > rows[-1]
                            rows.append(extra)
                        assert len(rows) in (1, 2, 4) and max(rows) <= p0 + t
                        want[b, t, heads] = v64[rows].mean(0)
                        q[b, heads, t, dim] = 512.0
                        if t + 1 < T:
                            rows.append(p0 + t + 1)                  # the decoy
                    kc[b, kv, rows, dim] = 4.0
    n = p0 + T
    kc[:, :, n:] = np.nan
    vc[:, :, n:] = np.inf
    vc[:, :, n + 1::2] = -np.inf
    return q, kc, vc, want.reshape(B * T, nh * D)


def _check_probe_on_cpu(q, kc, vc, want, p0):
    """The construction against float64 softmax . V: equal after rounding to fp16, and within 1e-50 before it (the weight of a cold row is
    e^-181)."""
    B, nh, T, _ = q.shape
    *_, ref = _reference(torch.from_numpy(q), torch.from_numpy(kc), torch.from_numpy(vc), p0)
    ref = _rows_out(ref, B, T, nh).numpy()
    assert np.array_equal(ref.astype(np.float16).astype(np.float64), want), "the probe's closed form is not softmax . V"
    assert np.abs(ref - want).max() < 1e-50


PROBE_P0 = (0, 1, 63, 64, 65, 200)
PROBE_T = (1, 2, 15, 16, 17, 63, 64, 65, 130)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("nh,nkv", HEADS)
def test_prefill_attention_probes_exact(K_, device, nh, nkv, B):
    """Every (pos0, T) of PROBE_P0 x PROBE_T: each (b, h, t) output must equal the exact mean of its 1, 2 or 4 visible hot V rows
    (_probe_case: row 0, both sides of every tile and wave boundary, pos0 + t - 1, pos0 + t among them; a decoy at pos0 + t + 1; NaN keys
    and +-Inf values from pos0 + T on).  The construction is checked on the CPU against float64 softmax . V first."""
    for p0 in PROBE_P0:
        for T in PROBE_T:
            if p0 + T > L:
                continue
            q, kc, vc, want = _probe_case(B, nh, nkv, p0, T, 1000 * p0 + 10 * T + B + nh)
            _check_probe_on_cpu(q, kc, vc, want, p0)
            assert K_.prefill_attention_describe(B, T, nh, nkv, D, L).startswith(WORD)
            out = _launch(K_, torch.from_numpy(q).to(device), torch.from_numpy(kc).to(device), torch.from_numpy(vc).to(device), p0, nh, nkv)
            o = out.double().cpu().numpy()
            bad = np.argwhere((o != want).reshape(B, T, nh, D).any(-1))
            assert len(bad) == 0, (p0, T, "first wrong (b, t, h):", bad[:6].tolist())


# ------------------------------------------------------------------------------------------------
# dense data
# ------------------------------------------------------------------------------------------------
def _prefill_bound(qd, Kd, Vd, vis, s, P, ref, p0):
    """Per-element bound on |o - ref| for quick_prefill_attention_f16, in float64 (shapes as _reference returns them), from the roundings
    the kernel performs.  Query t sees n_t = pos0 + t + 1 rows in NT = ceil(n_t / 32) tiles.

    A row's weight is exp2(s_t - m) with s_t = c q . k_t, c = scale * log2 e.  Its errors, in the log2 domain:
      * the dot product: 128 exact fp16 x fp16 products summed in fp32 by four 32-product MFMAs, <= 64 u c sum_j |q_j k_tj| (c applied to
        the fp32 score: one rounding more, inside the 64);
      * the subtraction of the running maximum and the rescalings exp2(m_old - m_new), one per tile: at most NT + 4 roundings of values
        <= |s_t| + |m|: (NT + 4) 2u (|s_t| + |m|);
    and exp2 itself, one ulp (2u relative) per call, at most NT + 2 calls on a weight.  So the relative weight error is
      eta_t = ln2 [64 u c sum_j |q_j k_tj| + (NT + 4) 2u (|s_t| + |m|)] + (NT + 2) 2u,
    and o = sum w v / sum w moves by at most sum_t p_t eta_t (|v_t| + |o|) (first order).
    P is rounded to fp16 as the operand of the second product (the denominator adds the unrounded weights): 2^-11 relative on a weight in
    fp16's normal range, 2^-11 sum_t p_t |v_t| on the quotient; a weight below 2^-14 (relative to the running maximum of its tile, which
    the final one only exceeds, and to a denominator >= 1 in those units) is off by at most 2^-25 absolute: 2^-25 sum_t |v_t| over the
    visible rows covers them.
    The fp32 accumulations: a term of the numerator passes, per tile after (and including) its own, one rescale and one MFMA of 32 products
    and the accumulator (<= 33 roundings): 34 NT u relative; a term of the denominator one rescale and 8 adds per tile, and 2 adds when the
    four lanes of a query merge: (9 NT + 2) u.  Together gamma = (43 NT + 2) u on sum_t p_t |v_t|.
    Last, the division and the rounding to fp16: one fp16 ulp of |ref| covers both."""
    T, n = vis.shape
    NT = torch.ceil((p0 + torch.arange(T, device=ref.device, dtype=torch.float64) + 1) / KV_ROWS)[:, None]     # [T, 1]
    c = SCALE * LOG2E
    S_abs = torch.einsum("bkgtd,bknd->bkgtn", qd.abs(), Kd.abs()) * c
    s2 = torch.where(vis, s * LOG2E, torch.zeros_like(s))
    m = (s * LOG2E).amax(-1, keepdim=True)
    eta = math.log(2) * (64 * U * S_abs + (NT + 4) * 2 * U * (s2.abs() + m.abs())) + (NT + 2) * 2 * U
    pv = torch.einsum("bkgtn,bknd->bkgtd", P, Vd.abs())
    dev = torch.einsum("bkgtn,bknd->bkgtd", P * eta, Vd.abs()) + (P * eta).sum(-1, keepdim=True) * ref.abs()
    gamma = (43 * NT + 2) * U
    seen = torch.cumsum(Vd.abs(), 2)[:, :, p0:p0 + T][:, :, None]                                           # [B, nkv, 1, T, D]
    return _ulp16(ref) + (gamma + 2.0 ** -11) * pv + 2.0 ** -25 * seen + dev


def _emulate(q, kc, vc, p0):
    """The kernel's stated rounding points in torch on the CPU (float64 where the kernel is exact, rounded where it rounds): per 32-row tile
    the scores as fp32 (dot, then times c), the running max, exp2 in fp32, the sum l in fp32 from the unrounded weights, P rounded to fp16,
    the tile's P V as one fp32 sum onto the rescaled accumulator, one fp32 division at the end and one rounding to fp16.  Rows behind
    pos0 + T are substituted by the last written row, as the kernel's staging does.  Returns [B, nkv, g, T, D] float64."""
    q, kc, vc = q.cpu(), kc.cpu(), vc.cpu()
    B, nh, T, _ = q.shape
    nkv = kc.shape[1]
    f32 = torch.float32
    qd = q.double().view(B, nkv, nh // nkv, T, D)
    limit = (p0 + torch.arange(T))[:, None]
    m = torch.full((B, nkv, nh // nkv, T, 1), float("-inf"), dtype=f32)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, nkv, nh // nkv, T, D), dtype=f32)
    c32 = torch.tensor(SCALE, dtype=f32) * torch.tensor(1.44269504088896, dtype=f32)
    for tile0 in range(0, p0 + T, KV_ROWS):
        rows = torch.arange(tile0, tile0 + KV_ROWS).clamp_max(p0 + T - 1)
        x = torch.einsum("bkgtd,bknd->bkgtn", qd, kc[:, :, rows].double()).to(f32) * c32
        x = torch.where(torch.arange(tile0, tile0 + KV_ROWS)[None, :] <= limit, x, torch.full_like(x, float("-inf")))
        mb = torch.maximum(m, x.amax(-1, keepdim=True))
        mref = torch.where(torch.isinf(mb), torch.zeros_like(mb), mb)
        corr = torch.exp2(m - mref)
        e = torch.exp2(x - mref)
        l = l * corr + e.sum(-1, keepdim=True, dtype=f32)
        pv = torch.einsum("bkgtn,bknd->bkgtd", e.half().double(), vc[:, :, rows].double())
        acc = ((acc * corr).double() + pv).to(f32)
        m = mb
    return (acc / l).half().double()


DENSE = [(0, 130), (65, 63), (200, 17), (381, 130)]


def _dense_case(B, nh, nkv, p0, T, variant, device):
    """N(0, 1) q, K, V in fp16; "peaked": K halved and, per (sequence, KV head), 24 rows replaced by beta (1 .. 3.5) times a query that
    sees them, which then leads its other rows by tens of nats.  NaN keys and +-Inf values from pos0 + T on."""
    g = torch.Generator(device=device).manual_seed(1000 * p0 + T + nh + (1 if variant == "peaked" else 0))
    group = nh // nkv
    q = torch.randn(B, nh, T, D, generator=g, device=device).half()
    kc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
    vc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
    if variant == "peaked":
        kc *= 0.5
        rng = np.random.default_rng(p0 + T)
        for b in range(B):
            for kv in range(nkv):
                for r in rng.choice(p0 + T, size=min(24, p0 + T), replace=False):
                    t = int(rng.integers(max(r - p0, 0), T))
                    h = kv * group + int(rng.integers(0, group))
                    kc[b, kv, r] = (q[b, h, t].float() * float(rng.uniform(1.0, 3.5))).half()
    _fill_behind(kc, vc, p0 + T)
    return q, kc, vc


@pytest.mark.parametrize("nh,nkv", HEADS)
def test_prefill_attention_dense_against_float64(K_, device, nh, nkv):
    """N(0, 1) data and a peaked variant at (pos0, T) of DENSE against float64 causal softmax . V of the kernel's own fp16 inputs:
    max(err / bound) <= 1 with _prefill_bound, printed with the largest bound.  The float64 emulation of the kernel's rounding points
    (_emulate) on the same inputs must stay within the same bound: its largest err / bound over these cases is 0.57 (random) and
    0.67 (peaked) -- the bound is not loose by more than a factor of two, and the rounding of P to fp16 is what fills it."""
    B = 2
    for p0, T in DENSE:
        for variant in ("random", "peaked"):
            q, kc, vc = _dense_case(B, nh, nkv, p0, T, variant, device)
            out = _launch(K_, q, kc, vc, p0, nh, nkv)
            qd, Kd, Vd, vis, s, P, ref = _reference(q, kc, vc, p0)
            bound = _prefill_bound(qd, Kd, Vd, vis, s, P, ref, p0)
            emu = ((_emulate(q, kc, vc, p0).to(device) - ref).abs() / bound).max()
            o = out.double().view(B, T, nkv, nh // nkv, D).permute(0, 2, 3, 1, 4)
            err = (o - ref).abs()
            ratio = float((err / bound).max())
            print(f"[prefill-dense] {nh}/{nkv} pos0={p0} T={T} {variant}: max err/bound {ratio:.3f} (emulation {float(emu):.3f}), "
                  f"max err {float(err.max()):.3g}, max bound {float(bound.max()):.3g}")
            assert float(emu) <= 1.0, ("the emulation of the kernel's rounding points leaves the bound", p0, T, variant, float(emu))
            assert ratio <= 1.0, (p0, T, variant, ratio, [int(i) for i in np.unravel_index(int((err / bound).argmax()), err.shape)])


# ------------------------------------------------------------------------------------------------
# T = 1 against the two-pass decode kernel
# ------------------------------------------------------------------------------------------------
def _decode_bound(q, Kc, Vc, p, s_ref, P, ref):
    """_attention_bound of tests/test_decode_ops_gpu.py: the fp32 single-query kernels' bound (q [B, nkv, g, D], Kc / Vc [B, nkv, p + 1, D])."""
    T = math.ceil((p + 1) / 64)
    R = math.ceil((p + 1) / 16)
    c = SCALE * LOG2E
    S_abs = torch.einsum("bkgd,bktd->bkgt", q.abs(), Kc.abs()) * c
    s2 = s_ref * LOG2E
    m = s2.amax(-1, keepdim=True)
    eta = math.log(2) * (64 * U * S_abs + (T + 4) * 2 * U * (s2.abs() + m.abs())) + (T + 2) * 2 * U
    dev = torch.einsum("bkgt,bkgt,bktd->bkgd", P, eta, Vc.abs()) + torch.einsum("bkgt,bkgt->bkg", P, eta)[..., None] * ref.abs()
    gamma = (R + T + 16) * U
    return _ulp16(ref) + 2 * gamma * torch.einsum("bkgt,bktd->bkgd", P, Vc.abs()) + dev


@pytest.mark.parametrize("nh,nkv", HEADS)
def test_prefill_attention_single_token_agrees_with_decode_attention(K_, device, nh, nkv):
    """T = 1 on the same cache: within the sum of both kernels' bounds of quick_decode_attention_f16 (the two-pass kernel)."""
    B = 3
    for p0 in (0, 31, 32, 200, L - 1):
        q, kc, vc = _dense_case(B, nh, nkv, p0, 1, "random", device)
        out = _launch(K_, q, kc, vc, p0, nh, nkv)
        buf, dec = _poisoned(B, (nh * D,), device)
        K_.decode_attention(q.view(B, nh, D), kc, vc, torch.full((1,), p0, dtype=torch.int64, device=device), dec, nh, nkv, D)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        qd, Kd, Vd, vis, s, P, ref = _reference(q, kc, vc, p0)
        bound = _prefill_bound(qd, Kd, Vd, vis, s, P, ref, p0)[:, :, :, 0] + \
            _decode_bound(qd[:, :, :, 0], Kd, Vd, p0, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])
        diff = (out.double().view(B, nkv, nh // nkv, D) - dec.double().view(B, nkv, nh // nkv, D)).abs()
        assert float((diff / bound).max()) <= 1.0, (p0, float((diff / bound).max()))


# ------------------------------------------------------------------------------------------------
# reproducibility
# ------------------------------------------------------------------------------------------------
def test_prefill_attention_is_reproducible_and_equals_its_forcezero_build(K_, device):
    """Two launches give bit-equal output, and so does the -amdgpu-waitcnt-forcezero build of the same sources, on three dense shapes."""
    from quick_amd import _lib
    from quick_amd.build import FORCEZERO_LIB
    other = _lib.load_other(FORCEZERO_LIB)
    for (nh, nkv), (p0, T) in zip(HEADS, DENSE[:3]):
        q, kc, vc = _dense_case(2, nh, nkv, p0, T, "random", device)
        a = _launch(K_, q, kc, vc, p0, nh, nkv)
        b = _launch(K_, q, kc, vc, p0, nh, nkv)
        z = _launch(K_, q, kc, vc, p0, nh, nkv, lib=other)
        assert _bits_equal(a, b), (nh, nkv, p0, T, "two launches differ")
        assert _bits_equal(a, z), (nh, nkv, p0, T, "the forcezero build differs")
