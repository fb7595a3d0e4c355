"""The decode-step kernels of decode_ops.hip against exact and float64 models.  Needs an MI355X.

Attention, probes: one-hot queries and keys make every score one exact product (2048 or 0) in every kernel and summation order, and the
hot rows lead every other row by ~261 in the log2 domain (181 nats in the two-pass kernel), so every other weight is exp2 of less than
-149: exactly 0 in fp32.  With V rows of multiples of 2^-8 the output is then exactly the hot V row, or the exact mean of 2 or 4 of them.
Every probe asserts which launch branch ran (quick_decode_rope_attention_describe), rows behind the position hold NaN keys and +-Inf
values, and outputs land in NaN-poisoned buffers with guard rows.

Attention, dense: random and peaked data at long contexts against float64 softmax . V, within an error model stated at _attention_bound.

RoPE bit for bit against the rounding points the kernels claim; RMSNorm bracketed by its only freedom (the last bits of rstd); SiLU * mul
against f16(silu64) and its fp16 neighbours; the lm_head arg-max at ties, signed zeros, block tails and against a float64 bound.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
U = 2.0 ** -24     # fp32 unit roundoff
SCALE = D ** -0.5


@pytest.fixture(scope="module")
def K_(device):
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


def _f16(a):
    return np.asarray(a, np.float64).astype(np.float16)


def _poisoned(rows, tail, device, fill=float("nan"), dtype=torch.float16):
    """Output buffer for rows 1..rows of a [rows + 2, *tail] tensor filled with `fill`: every element must be written and nothing next to it."""
    buf = torch.full((rows + 2,) + tuple(tail), fill, dtype=dtype, device=device)
    return buf, buf[1:rows + 1]


def _check_guard(buf, rows):
    assert torch.isnan(buf[0]).all() and torch.isnan(buf[rows + 1]).all(), "wrote next to the output"
    assert not torch.isnan(buf[1:rows + 1]).any(), "left output elements unwritten"


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def _tables(L, theta, dim=D):
    """fp16 RoPE tables [L, dim] (HF rotate-half: both halves carry the same angles)."""
    ang = np.outer(np.arange(L, dtype=np.float64), 1.0 / theta ** (np.arange(0, dim, 2) / dim))
    return _f16(np.concatenate([np.cos(ang)] * 2, -1)), _f16(np.concatenate([np.sin(ang)] * 2, -1))


def _rope_model(x, c, s):
    """The kernels' rounding points: f16(f32(f16(x0 c0)) + f32(f16(-x1 s0))) and f16(f32(f16(x1 c1)) + f32(f16(x0 s1))); numpy float32
    adds (every fp16 x fp16 product is exact in fp32, so the first rounding is the cast to fp16)."""
    f32, f16 = np.float32, np.float16
    h = x.shape[-1] // 2
    x0, x1 = x[..., :h].astype(f32), x[..., h:].astype(f32)
    c0, c1, s0, s1 = c[..., :h].astype(f32), c[..., h:].astype(f32), s[..., :h].astype(f32), s[..., h:].astype(f32)
    r0 = ((x0 * c0).astype(f16).astype(f32) + (-x1 * s0).astype(f16).astype(f32)).astype(f16)
    r1 = ((x1 * c1).astype(f16).astype(f32) + (x0 * s1).astype(f16).astype(f32)).astype(f16)
    return np.concatenate([r0, r1], -1)


def _ulp16(a):
    """Spacing of fp16 at |a| (float64 tensor): 2^(e - 10) in the normal range, 2^-24 below it."""
    e = torch.floor(torch.log2(a.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


# ------------------------------------------------------------------------------------------------
# attention: the launch branches
# ------------------------------------------------------------------------------------------------
# (name, B, nh, nkv, L, leading words of attention_describe)
BRANCHES = [
    ("gqa-mfma-8", 32, 64, 8, 4096, "gqa-mfma heads=8 gsplit=1 waves=4 set_rows=64"),
    ("gqa-mfma-4x2", 16, 64, 8, 4096, "gqa-mfma heads=4 gsplit=2 waves=4 set_rows=64"),
    ("gqa-mfma-4", 32, 32, 8, 4096, "gqa-mfma heads=4 gsplit=1 waves=4 set_rows=64"),
    ("gqa-2x2", 16, 32, 8, 4096, "gqa heads=2 gsplit=2 waves=4 set_rows=64"),
    ("gqa-2", 32, 16, 8, 4096, "gqa heads=2 gsplit=1 waves=4 set_rows=64"),
    ("flash-8", 4, 32, 8, 4096, "flash heads=1 gsplit=1 waves=8 set_rows=128"),
    ("flash-4", 3, 48, 16, 4096, "flash heads=1 gsplit=1 waves=4 set_rows=64"),   # (group 3: no grouped-query kernel)
    ("two-pass", 4, 32, 8, 4096, None),                                             # quick_decode_attention_f16
    ("two-pass-15872", 2, 16, 4, 15872, None),                                      # its LDS limit
]
PROBE_P = (0, 1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 4095)
# hot-row candidates: the first rows, the wave boundaries (4 rows per slot: 3 / 4; a 16-row MFMA chunk: 15 / 16), the register set and
# trip boundaries (64 and 128 rows per set, sets alternating), and p - 2 .. p (the last cache rows and this token)
HOT = (0, 1, 2, 3, 4, 15, 16, 17, 31, 32, 63, 64, 65, 127, 128, 129, 191, 192, 255, 256, 257, 383, 384, 511, 512)


def _run_attention(K_, name, B, nh, nkv, L, word, qkv, q_rot, kc, vc, p, cos, sin, device):
    """One launch of the branch into a poisoned output; returns the output [B, nh * D]."""
    buf, out = _poisoned(B, (nh * D,), device)
    pos = torch.full((1,), p, dtype=torch.int64, device=device)
    if word is None:
        K_.decode_attention(q_rot, kc, vc, pos, out, nh, nkv, D)
    else:
        assert K_.attention_describe(B, nh, nkv, D, L).startswith(word), (name, K_.attention_describe(B, nh, nkv, D, L))
        K_.rope_attention(qkv, cos, sin, pos, kc, vc, out, nh, nkv, D)
    torch.cuda.synchronize()
    _check_guard(buf, B)
    return out


def _fill_behind(kc, vc, p):
    """Rows p + 1.. of a real cache are unwritten: NaN keys, +-Inf values (a value row behind the position that leaks into a sum shows)."""
    kc[:, :, p + 1:] = float("nan")
    vc[:, :, p + 1:] = float("inf")
    vc[:, :, p + 2::2] = float("-inf")


@pytest.mark.parametrize("name,B,nh,nkv,L,word", BRANCHES, ids=[b[0] for b in BRANCHES])
def test_attention_position_probes_exact(K_, device, name, B, nh, nkv, L, word):
    """Every branch, every position of PROBE_P: each (sequence, query head) has its own one-hot query dimension and 1, 2 or 4 hot rows
    (identical keys) among HOT, p - 2, p - 1 and p; out[b, h] must be exactly the mean of their V rows (row p: the new token's v).  Row p
    of both caches must be written bit for bit and every other cache byte left alone."""
    group = nh // nkv
    span = D // group
    cos, sin = (torch.from_numpy(t).to(device) for t in _tables(L, 1e4))
    ps = PROBE_P + ((8191, L - 1) if L > 4096 else ())
    for p in ps:
        rng = np.random.default_rng(1000 * p + B)
        cand = sorted({t for t in HOT + (p - 2, p - 1, p) if 0 <= t <= p})
        nc = len(cand)
        hot = np.zeros((B, nh, 4), np.int64)
        wgt = np.zeros((B, nh, 4))
        dim = np.zeros((B, nh), np.int64)
        for b in range(B):
            for h in range(nh):
                i = b * nh + h
                n = (1, 2, 4)[i % 3]
                while n > nc:
                    n //= 2
                k = i // 3 + b
                rows = [cand[(k + j * (nc // n)) % nc] for j in range(n)]
                hot[b, h, :n] = rows
                hot[b, h, n:] = rows[0]
                wgt[b, h, :n] = 1.0 / n
                dim[b, h] = (h % group) * span + (b + h // group) % span     # distinct within a KV group: keys are shared
        bi, hi = np.meshgrid(np.arange(B), np.arange(nh), indexing="ij")
        kvi = hi // group
        # keys: 4 at the head's dimension in its hot rows, 0 elsewhere; the new token's key likewise where p is hot
        kc = torch.zeros(B, nkv, L, D, dtype=torch.float16, device=device)
        knew = torch.zeros(B, nkv, D, dtype=torch.float16, device=device)
        sel = wgt > 0
        bb, hh, jj = np.nonzero(sel)
        rows = hot[bb, hh, jj]
        in_cache = rows < p
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
        kc[t(bb[in_cache]), t(kvi[bb, hh][in_cache]), t(rows[in_cache]), t(dim[bb, hh][in_cache])] = 4.0
        knew[t(bb[~in_cache]), t(kvi[bb, hh][~in_cache]), t(dim[bb, hh][~in_cache])] = 4.0
        q = torch.zeros(B, nh, D, dtype=torch.float16, device=device)
        q[t(bi.ravel()), t(hi.ravel()), t(dim.ravel())] = 512.0
        g = torch.Generator(device=device).manual_seed(p + 7 * B)
        vc = (torch.randint(-256, 257, (B, nkv, L, D), generator=g, device=device).half() / 256)
        vnew = (torch.randint(-256, 257, (B, nkv, D), generator=g, device=device).half() / 256)
        _fill_behind(kc, vc, p)
        kc[:, :, p], vc[:, :, p] = float("nan"), float("nan")
        # the identity rotation at row p
        cos_p, sin_p = cos.clone(), sin.clone()
        cos_p[p], sin_p[p] = 1.0, 0.0
        vfull = vc.clone()
        vfull[:, :, p] = vnew
        gathered = vfull[t(bi)[..., None], t(kvi)[..., None], t(hot)].double()        # [B, nh, 4, D]
        want = (gathered * t(wgt)[..., None]).sum(2)
        assert torch.equal(want.half().double(), want)                                 # (exact in fp16)
        kc_want, vc_want = kc.clone(), vc.clone()
        kc_want[:, :, p], vc_want[:, :, p] = knew, vnew
        if word is None:                         # the two-pass kernel reads row p from the cache: the caller appended it
            kc[:, :, p], vc[:, :, p] = knew, vnew
        qkv = torch.cat([q.view(B, -1), knew.view(B, -1), vnew.view(B, -1)], -1).contiguous()
        out = _run_attention(K_, name, B, nh, nkv, L, word, qkv, q, kc, vc, p, cos_p, sin_p, device)
        o = out.view(B, nh, D).double()
        bad = (o != want).any(-1)
        assert not bool(bad.any()), (name, p, [(int(b), int(h), hot[b, h].tolist(), float(wgt[b, h, 0])) for b, h in bad.nonzero()[:4].tolist()])
        assert _bits_equal(kc, kc_want) and _bits_equal(vc, vc_want), (name, p, "cache rows other than p changed, or row p wrong")


def _attention_bound(q, Kc, Vc, p, s_ref, P, ref):
    """Per-element bound |o - ref| for the fp32 single-query kernels, in float64 (q [B, nkv, g, D], Kc / Vc [B, nkv, p + 1, D]).

    A row's weight is exp2(s_t - m) with s_t = c q . k_t, c = scale * log2 e.  Its errors, in the log2 domain:
      * the dot product: 128 exact fp16 x fp16 products summed in fp32 by at most 12 roundings (8 per lane, 4 across lanes) or, on the
        matrix core, by four 32-product MFMAs; both <= 64 u * c * sum_j |q_j k_tj| (c applied to q or to the score: one rounding more);
      * the subtraction of the running maximum, the constant c and the rescalings exp2(m_old - m_new), at most T + 4 roundings of values
        <= |s_t| + |m|: (T + 4) 2u (|s_t| + |m|);
    and exp2 itself, one ulp (2u relative) per call, at most T + 2 calls on a weight.  So the relative weight error is
      eta_t = ln2 * [64 u c sum_j |q_j k_tj| + (T + 4) 2u (|s_t| + |m|)] + (T + 2) 2u,
    and o = sum w v / sum w moves by at most sum_t p_t |v_t - o| eta_t (first order).  The fp32 accumulations of numerator and denominator
    run over R <= ceil((p + 1) / 16) rows per accumulator (16 row slots, or 4 waves x 4 row quarters, per workgroup), rescaled at most
    T = ceil((p + 1) / 64) times and merged in <= 16 more operations: gamma = (R + T + 16) u relative on each, so 2 gamma sum_t p_t |v_t|
    on the quotient.  Last, the division and the rounding to fp16: one fp16 ulp of |ref| covers both."""
    T = math.ceil((p + 1) / 64)
    R = math.ceil((p + 1) / 16)
    c = SCALE * math.log2(math.e)
    S_abs = torch.einsum("bkgd,bktd->bkgt", q.abs(), Kc.abs()) * c
    s2 = s_ref * math.log2(math.e)
    m = s2.amax(-1, keepdim=True)
    eta = math.log(2) * (64 * U * S_abs + (T + 4) * 2 * U * (s2.abs() + m.abs())) + (T + 2) * 2 * U
    dev = torch.einsum("bkgt,bkgt,bktd->bkgd", P, eta, Vc.abs()) + torch.einsum("bkgt,bkgt->bkg", P, eta)[..., None] * ref.abs()
    gamma = (R + T + 16) * U
    return _ulp16(ref) + 2 * gamma * torch.einsum("bkgt,bktd->bkgd", P, Vc.abs()) + dev


@pytest.mark.parametrize("name,B,nh,nkv,L,word", BRANCHES[:-1], ids=[b[0] for b in BRANCHES[:-1]])
def test_attention_dense_long_context_against_float64(K_, device, name, B, nh, nkv, L, word):
    """Random N(0, 1) data and a peaked variant (each head's top row leads by ~11..40 nats) at p = 511, 2047, 4095 against float64
    softmax . V of the kernel's own fp16 inputs (q and the new k through _rope_model), within _attention_bound.  Prints max(err / bound)."""
    group = nh // nkv
    for p, theta in ((511, 1e4), (2047, 1e4), (4095, 1e6)):
        cos_np, sin_np = _tables(L, theta)
        cos, sin = torch.from_numpy(cos_np).to(device), torch.from_numpy(sin_np).to(device)
        for variant in ("random", "peaked"):
            g = torch.Generator(device=device).manual_seed(p + B + (1 if variant == "peaked" else 0))
            qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
            qkv_np = qkv.cpu().numpy()
            q_np = qkv_np[:, :nh * D].reshape(B, nh, D)
            k_np = qkv_np[:, nh * D:(nh + nkv) * D].reshape(B, nkv, D)
            q_rot = _rope_model(q_np, cos_np[p], sin_np[p])
            k_rot = torch.from_numpy(_rope_model(k_np, cos_np[p], sin_np[p])).to(device)
            vnew = qkv[:, (nh + nkv) * D:].view(B, nkv, D)
            kc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
            vc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
            if variant == "peaked":
                kc *= 0.5
                rng = np.random.default_rng(p)
                for kv in range(nkv):        # each query head of the group gets its own peak row: beta * its rotated query
                    rows = rng.choice(p, size=(B, group), replace=False) if B * group <= p else rng.integers(0, p, (B, group))
                    beta = torch.from_numpy(rng.uniform(1.0, 3.5, (B, group))).to(device)
                    qh = torch.from_numpy(q_rot[:, kv * group:(kv + 1) * group].astype(np.float32)).to(device)
                    kc[torch.arange(B, device=device)[:, None], kv, torch.from_numpy(rows).to(device)] = (qh * beta[..., None]).half()
            _fill_behind(kc, vc, p)
            kc[:, :, p], vc[:, :, p] = float("nan"), float("nan")
            kc_want, vc_want = kc.clone(), vc.clone()
            kc_want[:, :, p], vc_want[:, :, p] = k_rot, vnew
            q_rot_t = torch.from_numpy(q_rot).to(device)
            if word is None:
                kc[:, :, p], vc[:, :, p] = k_rot, vnew
            out = _run_attention(K_, name, B, nh, nkv, L, word, qkv, q_rot_t, kc, vc, p, cos, sin, device)
            assert _bits_equal(kc, kc_want) and _bits_equal(vc, vc_want), (name, p, variant, "cache row p is not the RoPE model's")
            # float64 reference
            qd = q_rot_t.double().view(B, nkv, group, D)
            Kd, Vd = kc_want[:, :, :p + 1].double(), vc_want[:, :, :p + 1].double()
            s = torch.einsum("bkgd,bktd->bkgt", qd, Kd) * SCALE
            P = torch.softmax(s, -1)
            ref = torch.einsum("bkgt,bktd->bkgd", P, Vd)
            bound = _attention_bound(qd, Kd, Vd, p, s, P, ref)
            err = (out.view(B, nkv, group, D).double() - ref).abs()
            ratio = float((err / bound).max())
            if variant == "peaked":
                top2 = s.topk(2, -1).values
                lead = (top2[..., 0] - top2[..., 1]).median()
                assert float(lead) >= 5, (name, p, float(lead))
            print(f"[attention-dense] {name} p={p} {variant}: max err/bound {ratio:.3f}, max err {float(err.max()):.3g}")
            assert ratio <= 1.0, (name, p, variant, ratio, [int(i) for i in np.unravel_index(int((err / bound).argmax()), err.shape)])


# ------------------------------------------------------------------------------------------------
# RoPE
# ------------------------------------------------------------------------------------------------
def _random_qkv(rows, width, seed, device):
    """N(0, 1) with some large (|x| ~ 1e3) and tiny (subnormal-product) entries mixed in."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, width))
    m = rng.random((rows, width))
    x[m < 0.05] *= 1000
    x[m > 0.95] *= 1e-4
    return torch.from_numpy(_f16(x)).to(device)


@pytest.mark.parametrize("Dh", [64, 128])
def test_rope_kv_append_bit_exact(K_, device, Dh):
    B, nh, nkv, L = 3, 8, 2, 64
    cos_np, sin_np = _tables(L, 1e4, Dh)
    cos, sin = torch.from_numpy(cos_np).to(device), torch.from_numpy(sin_np).to(device)
    for p in (0, 1, 37, L - 1):
        qkv = _random_qkv(B, (nh + 2 * nkv) * Dh, p + Dh, device)
        x = qkv.cpu().numpy()
        g = torch.Generator(device=device).manual_seed(p)
        kc = torch.randint(-2 ** 15, 2 ** 15, (B, nkv, L, Dh), generator=g, device=device, dtype=torch.int16).view(torch.float16)
        vc = torch.randint(-2 ** 15, 2 ** 15, (B, nkv, L, Dh), generator=g, device=device, dtype=torch.int16).view(torch.float16)
        kc_want, vc_want = kc.clone(), vc.clone()
        q_want = _rope_model(x[:, :nh * Dh].reshape(B, nh, Dh), cos_np[p], sin_np[p])
        kc_want[:, :, p] = torch.from_numpy(_rope_model(x[:, nh * Dh:(nh + nkv) * Dh].reshape(B, nkv, Dh), cos_np[p], sin_np[p])).to(device)
        vc_want[:, :, p] = qkv[:, (nh + nkv) * Dh:].view(B, nkv, Dh)
        buf, q_out = _poisoned(B, (nh, Dh), device)
        K_.rope_kv_append(qkv, cos, sin, torch.full((1,), p, dtype=torch.int64, device=device), q_out, kc, vc, nh, nkv, Dh)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        assert np.array_equal(q_out.cpu().numpy().view(np.uint16), q_want.view(np.uint16)), (Dh, p)
        assert _bits_equal(kc, kc_want) and _bits_equal(vc, vc_want), (Dh, p)


@pytest.mark.parametrize("Dh", [64, 128])
def test_rope_kv_write_bit_exact(K_, device, Dh):
    B, nh, nkv, L = 2, 8, 4, 96
    cos_np, sin_np = _tables(L, 1e4, Dh)
    cos, sin = torch.from_numpy(cos_np).to(device), torch.from_numpy(sin_np).to(device)
    for T, p0 in ((1, 0), (1, L - 1), (5, 3), (37, 0), (37, L - 37), (L, 0)):
        qkv = _random_qkv(B * T, (nh + 2 * nkv) * Dh, T + p0 + Dh, device)
        x = qkv.cpu().numpy().reshape(B, T, -1)
        g = torch.Generator(device=device).manual_seed(T + p0)
        kc = torch.randint(-2 ** 15, 2 ** 15, (B, nkv, L, Dh), generator=g, device=device, dtype=torch.int16).view(torch.float16)
        vc = torch.randint(-2 ** 15, 2 ** 15, (B, nkv, L, Dh), generator=g, device=device, dtype=torch.int16).view(torch.float16)
        c, s = cos_np[p0:p0 + T][None, :, None], sin_np[p0:p0 + T][None, :, None]      # [1, T, 1, Dh]
        q_want = _rope_model(x[..., :nh * Dh].reshape(B, T, nh, Dh), c, s).transpose(0, 2, 1, 3)
        k_want = _rope_model(x[..., nh * Dh:(nh + nkv) * Dh].reshape(B, T, nkv, Dh), c, s).transpose(0, 2, 1, 3)
        kc_want, vc_want = kc.clone(), vc.clone()
        kc_want[:, :, p0:p0 + T] = torch.from_numpy(np.ascontiguousarray(k_want)).to(device)
        vc_want[:, :, p0:p0 + T] = qkv.view(B, T, -1)[..., (nh + nkv) * Dh:].reshape(B, T, nkv, Dh).transpose(1, 2)
        buf, q_out = _poisoned(B, (nh, T, Dh), device)
        K_.rope_kv_write(qkv, cos, sin, torch.full((1,), p0, dtype=torch.int64, device=device), q_out, kc, vc, T, nh, nkv, Dh)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        assert np.array_equal(q_out.cpu().numpy().view(np.uint16), np.ascontiguousarray(q_want).view(np.uint16)), (Dh, T, p0)
        assert _bits_equal(kc, kc_want) and _bits_equal(vc, vc_want), (Dh, T, p0)


# ------------------------------------------------------------------------------------------------
# RMSNorm
# ------------------------------------------------------------------------------------------------
def _row_kind(m):
    """0 normal, 1 massive channels, 2 tiny, 3 all zero, 4 constant"""
    return (1, 2, 4, 3, 0)[m % 5]


def _edge_rows(M, K, rng, small_w=False):
    """Row kinds cycled over M rows (_row_kind): 1..6 massive channels (|x| 1e3 .. 3e4); tiny (rms ~ 1e-3); constant; all zero; normal --
    the edges first.  Norm weights 4 on the massive channels, elsewhere 0.5 .. 1.5 or (small_w) 0.02 .. 0.1.  (As in test_fusion_gpu.)"""
    x = np.zeros((M, K), np.float64)
    massive = np.zeros(K, bool)
    massive[rng.choice(K, min(6, K), replace=False)] = True
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


def _rmsnorm_eps(H):
    """Relative bound on the kernel's rstd against the exact one.  Squares of fp16 values are exact in fp32; each reaches the total through
    at most n = 8 ceil(H / 2048) sequential adds in its thread, 6 in the wave butterfly and 3 across the four wave sums, so the sum of
    these positive terms is off by at most gamma_n = n u / (1 - n u) relative; / H and + eps round once more each (2u); the square root
    halves the relative error; rsqrtf adds at most 2 ulp (2^-22)."""
    n = 8 * math.ceil(H / 2048) + 6 + 3
    gamma = n * U / (1 - n * U)
    return (gamma + 2 * U) / 2 * (1 + 1e-6) + 2.0 ** -22


def _rms_bracket(x, w, eps, rel):
    """f16(f16(f32(x r)) w) at r = rstd64 (1 -+ rel): monotone in r, so the kernel's y lies between the two ends."""
    xf = x.astype(np.float64)
    rstd = 1.0 / np.sqrt((xf * xf).mean(-1, keepdims=True) + float(np.float32(eps)))
    ends = []
    for r in (rstd * (1 - rel), rstd * (1 + rel)):
        ends.append(_f16(_f16((xf * r).astype(np.float32)).astype(np.float64) * w.astype(np.float64)).astype(np.float64))
    return np.minimum(*ends), np.maximum(*ends)


@pytest.mark.parametrize("H", [8, 512, 2048, 2056, 4096, 5120, 8192, 8200, 11008, 16384])
def test_rmsnorm_bracketed_by_rstd_rounding(K_, device, H):
    """Every instantiation (NIT = 1 / 2 / 4 and the generic loop) and its partial last chunk, on massive, tiny, zero and constant rows:
    each y between the ends of _rms_bracket at eps = _rmsnorm_eps(H); zero and constant rows (sums exact in fp32) bit for bit."""
    M, eps = 10, 1e-5
    x, w, _ = _edge_rows(M, H, np.random.default_rng(H))
    xd, wd = torch.from_numpy(x).to(device), torch.from_numpy(w).to(device)
    buf, out = _poisoned(M, (H,), device)
    K_.rmsnorm(xd, wd, eps, out=out)
    torch.cuda.synchronize()
    _check_guard(buf, M)
    y = out.cpu().numpy().astype(np.float64)
    lo, hi = _rms_bracket(x, w, eps, _rmsnorm_eps(H))
    outside = (y < lo) | (y > hi)
    assert not outside.any(), (H, [(int(m), int(j), y[m, j], lo[m, j], hi[m, j]) for m, j in zip(*np.nonzero(outside))][:5])
    exact = [m for m in range(M) if _row_kind(m) in (3, 4)]
    assert np.array_equal(lo[exact], hi[exact]) and np.array_equal(y[exact], lo[exact]), H
    assert np.all(y[[m for m in range(M) if _row_kind(m) == 3]] == 0)


@pytest.mark.parametrize("H", [512, 2048, 4096, 5120, 8192, 16384])
def test_lm_head_hidden_equals_rmsnorm_on_edge_rows(K_, device, H):
    """The lm_head normalises in its own launch with quick_rmsnorm_f16's order of the sum of squares: hidden_out bit-equal to it."""
    M, B = 10, min(4, 36864 // H)
    x, w, _ = _edge_rows(M, H, np.random.default_rng(H + 1))
    xd, wd = torch.from_numpy(x).to(device), torch.from_numpy(w).to(device)
    W = (torch.randn(64, H, device=device) * 0.02).half()
    y = K_.rmsnorm(xd, wd, 1e-5)
    for m0 in range(0, M, B):
        rows = slice(m0, min(m0 + B, M))
        _, hid, _ = _lm_head(xd[rows].contiguous(), W, wd)
        assert _bits_equal(hid, y[rows]), (H, m0)


# ------------------------------------------------------------------------------------------------
# SiLU * mul
# ------------------------------------------------------------------------------------------------
SILU_EXACT_G = (0.0, 16.0, 20.0, 100.0, 1000.0, 65504.0, -20.0, -30.0, -100.0, -1000.0, -65504.0)


def _silu64(g):
    with np.errstate(over="ignore"):
        return g / (1.0 + np.exp(-g))


@pytest.mark.parametrize("I", [8, 1024, 11008, 14336, 28672])
def test_silu_mul_against_float64(K_, device, I):
    """y = f16(s * u) with s = f16(silu64(g)) or one of its fp16 neighbours (__expf is not exact); exact at g = 0 and far out on both
    sides.  Gate and up interleaved in blocks of 8; rows * I / 8 not a multiple of the 256-thread workgroup."""
    for rows in (1, 3, 64, 257):
        rng = np.random.default_rng(I + rows)
        g = rng.standard_normal((rows, I)) * 4
        special = rng.random((rows, I)) < 0.1
        g[special] = rng.choice(SILU_EXACT_G, int(special.sum()))
        g = _f16(g)
        u = _f16(rng.standard_normal((rows, I)) * 2)
        gu = np.stack([g.reshape(rows, I // 8, 8), u.reshape(rows, I // 8, 8)], 2).reshape(rows, 2 * I)
        buf, out = _poisoned(rows, (I,), device)
        K_.silu_mul(torch.from_numpy(np.ascontiguousarray(gu)).to(device), out=out)
        torch.cuda.synchronize()
        _check_guard(buf, rows)
        y = out.cpu().numpy()
        s0 = _f16(_silu64(g.astype(np.float64)))
        with np.errstate(over="ignore"):
            cands = [_f16(s.astype(np.float64) * u.astype(np.float64)) for s in (np.nextafter(s0, np.float16(-np.inf)), s0,
                                                                                np.nextafter(s0, np.float16(np.inf)))]
        ok = (y == cands[0]) | (y == cands[1]) | (y == cands[2])
        assert ok.all(), (I, rows, [(float(g[i]), float(u[i]), float(y[i]), float(cands[1][i])) for i in zip(*np.nonzero(~ok))][:4])
        assert np.array_equal(y[special].view(np.uint16), cands[1][special].view(np.uint16)), (I, rows)


# ------------------------------------------------------------------------------------------------
# lm_head arg-max
# ------------------------------------------------------------------------------------------------
def _lm_head(x, w, nw, eps=1e-5):
    """quick_lm_head_argmax_f16 into poisoned hidden / logits / token buffers with guard rows."""
    from quick_amd import _lib
    lib = _lib.load()
    (B, H), V, dev = x.shape, w.shape[0], x.device
    ws = torch.empty(lib.quick_lm_head_workspace_bytes(B), dtype=torch.uint8, device=dev)
    hb, hid = _poisoned(B, (H,), dev)
    lb, lg = _poisoned(B, (V,), dev)
    tb = torch.full((B + 2,), -7, dtype=torch.int64, device=dev)
    rc = lib.quick_lm_head_argmax_f16(x.data_ptr(), nw.data_ptr() if nw is not None else None, eps, w.data_ptr(), hid.data_ptr(),
                                      lg.data_ptr(), tb[1:B + 1].data_ptr(), ws.data_ptr(), ws.numel(), B, V, H,
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    _check_guard(hb, B)
    _check_guard(lb, B)
    assert int(tb[0]) == -7 and int(tb[B + 1]) == -7
    return tb[1:B + 1], hid, lg


def _check_logits(hid, w, lg, tok):
    """Logits within fp16 rounding of a float64 dot product plus the fp32 error of the fdot2 chain (<= 2 H / 64 roundings per lane, 8
    across lanes); the token the lowest index among the largest fp16 logits."""
    H = hid.shape[1]
    ref = hid.double() @ w.double().t()
    absdot = hid.double().abs() @ w.double().abs().t()
    bound = _ulp16(ref) + (2 * H / 64 + 8) * U * absdot
    err = (lg.double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    for b in range(hid.shape[0]):
        top = lg[b].max()
        first = int((lg[b] == top).nonzero()[0])
        assert int(tok[b]) == first, (b, int(tok[b]), first)
    return ref


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_lm_head_argmax_ties_tails_and_signs(K_, device, B):
    g = torch.Generator(device=device).manual_seed(B)
    # duplicated maximum rows in four different workgroups (row r: block r // 4, workgroup (r // 32) % 512): the lowest index wins
    V, H = 32000, 4096
    x = torch.randn(B, H, generator=g, device=device).half()
    nw = (1 + 0.1 * torch.randn(H, generator=g, device=device)).half()
    w = (torch.randn(V, H, generator=g, device=device) * 0.02).half()
    h = K_.rmsnorm(x, nw)
    dups = [[37 + b, 4093 + 7 * b, 17001 + b, 31999 - b] for b in range(B)]
    for b in range(B):
        w[dups[b]] = (torch.sign(h[b].float()) * 0.05).half()
    tok, hid, lg = _lm_head(x, w, nw)
    assert torch.equal(hid, h)
    _check_logits(hid, w, lg, tok)
    for b in range(B):
        assert int(tok[b]) == 37 + b and bool((lg[b, dups[b]] == lg[b].max()).all()), (b, int(tok[b]))
    # the maximum at V - 1 (V % 4 != 0: the last block is partial) and at index 0; all-negative logits
    V, H = 32003, 1024
    x = (torch.rand(B, H, generator=g, device=device) + 0.1).half()
    nw = (torch.rand(H, generator=g, device=device) + 0.5).half()
    for where in (V - 1, 0, None):
        w = (torch.randn(V, H, generator=g, device=device) * 0.02).half()
        if where is None:
            w = -(w.abs() + 2.0 ** -10)
        else:
            w[where] = 0.05
        tok, hid, lg = _lm_head(x, w, nw)
        _check_logits(hid, w, lg, tok)
        if where is None:
            assert bool((lg < 0).all())
        else:
            assert bool((tok == where).all()), (where, tok.tolist())


@pytest.mark.parametrize("B", [1, 2, 3, 4])
def test_lm_head_argmax_signed_zero_tie(K_, device, B):
    """The largest logit is zero, -0 at index 0 (-2^-28 rounds to -0) and +0 at index 1: they compare equal, the lowest index wins."""
    H, V = 512, 1000
    x = torch.zeros(B, H, dtype=torch.float16, device=device)
    x[:, 0] = 2.0 ** -14
    w = torch.zeros(V, H, dtype=torch.float16, device=device)
    w[0, 0] = -2.0 ** -14
    w[2:, 0] = -1.0
    tok, hid, lg = _lm_head(x, w, None)
    assert torch.equal(hid, x)
    assert bool((lg[:, 0].view(torch.int16) == -0x8000).all()) and bool((lg[:, 1].view(torch.int16) == 0).all())
    assert tok.tolist() == [0] * B, tok.tolist()
