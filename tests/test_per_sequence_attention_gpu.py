"""The per-sequence launches (quick_decode_rope_attention_seq_f16, quick_rope_kv_write_seq_f16, quick_prefill_attention_seq_f16) on an
MI355X: sequence b works at pos[b].

A workgroup's arithmetic depends on its own sequence and that sequence's position only, so every comparison with the shared launches is
BIT FOR BIT: for each distinct position v the shared entry runs on copies of the same inputs with pos = [v], and the sequences that sit at
v must give the same output rows and the same cache rows; every other cache element keeps its initial bits (NaNs included).  Rows at or
behind a sequence's position hold NaN keys and +-Inf values.  Two decode shapes and two prefill lengths are also held against float64
softmax . V within the kernels' stated bounds (restated from tests/test_prefill_attention_gpu.py), and positions outside a launch's range
are skipped: nothing written, outputs left as they were.

The float64 references take q and the new k through the kernels' stated RoPE rounding points (_rope_model, as tests/test_decode_ops_gpu.py
does -- the bounds are bounds on the attention, and the appended k row is compared bit for bit here anyway) and everything behind them in
float64.

Run as a program (``python tests/test_per_sequence_attention_gpu.py child``) the file repeats the decode comparisons on the two shapes that
reach decode_rope_attention_gqa_kernel<4> -- only with QUICK_AMD_ATTN_MFMA=0, which the library reads once per process.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
D = 128
U = 2.0 ** -24     # fp32 unit roundoff
SCALE = D ** -0.5
LOG2E = math.log2(math.e)
KV_ROWS = 32       # cache rows per tile of the prefill kernel
SENTINEL = 1234.0  # what an output row nobody may write holds

L_DEC = 320
POSITIONS = (0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 319)
# (nh, nkv, B), the leading words of attention_describe
DECODE_SHAPES = [
    ((4, 4, 5), "flash heads=1 gsplit=1 waves=8"),
    ((4, 4, 40), "flash heads=1 gsplit=1 waves=4"),
    ((2, 1, 256), "gqa heads=2 gsplit=1"),
    ((4, 1, 128), "gqa heads=2 gsplit=2"),
    ((4, 1, 256), "gqa-mfma heads=4 gsplit=1"),
    ((8, 1, 128), "gqa-mfma heads=4 gsplit=2"),
    ((8, 1, 256), "gqa-mfma heads=8 gsplit=1"),
]
FLOAT64_SHAPES = {(4, 4, 5), (8, 1, 128)}
CHILD_SHAPES = [((8, 1, 128), "gqa heads=4 gsplit=2"), ((4, 1, 256), "gqa heads=4 gsplit=1")]   # with QUICK_AMD_ATTN_MFMA=0

L_PRE = 192
PREFILL_HEADS = [(4, 4), (8, 2)]
PREFILL_POS0 = (0, 5, 31, 32, 100)
PREFILL_T = (2, 17, 64, 65, 80)      # both sides of the 16-row wave, the 32-row tile and the 64-row workgroup
FLOAT64_T = {17, 65}


def _kernels():
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def K_(device):
    return _kernels()


def _bits(a):
    return a.contiguous().view(torch.int16)


def _bits_equal(a, b):
    return torch.equal(_bits(a), _bits(b))


def _tables(L, device, theta=1e4):
    """fp16 RoPE tables [L, D] (HF rotate-half: both halves carry the same angles)."""
    ang = np.outer(np.arange(L, dtype=np.float64), 1.0 / theta ** (np.arange(0, D, 2) / D))
    cos, sin = (np.concatenate([f(ang)] * 2, -1).astype(np.float16) for f in (np.cos, np.sin))
    return torch.from_numpy(cos).to(device), torch.from_numpy(sin).to(device)


def _rope_model(x, c, s):
    """The kernels' rounding points: f16(f32(f16(x0 c0)) + f32(f16(-x1 s0))) and f16(f32(f16(x1 c1)) + f32(f16(x0 s1))), every fp16 x fp16
    product being exact in fp32 (torch tensors, fp16 in, fp16 out)."""
    h = x.shape[-1] // 2
    x0, x1, c0, c1, s0, s1 = (t.float() for t in (x[..., :h], x[..., h:], c[..., :h], c[..., h:], s[..., :h], s[..., h:]))
    r0 = ((x0 * c0).half().float() + (-x1 * s0).half().float()).half()
    r1 = ((x1 * c1).half().float() + (x0 * s1).half().float()).half()
    return torch.cat([r0, r1], -1)


def _ulp16(a):
    """Spacing of fp16 at |a| (float64 tensor): 2^(e - 10) in the normal range, 2^-24 below it."""
    e = torch.floor(torch.log2(a.abs().clamp_min(2.0 ** -14)))
    return torch.exp2(e - 10)


def _poison_behind(kc, vc, first):
    """Rows first[b].. of sequence b are unwritten: NaN keys, +-Inf values."""
    for b, n in enumerate(first):
        n = max(int(n), 0)
        kc[b, :, n:] = float("nan")
        vc[b, :, n:] = float("inf")
        vc[b, :, n + 1::2] = float("-inf")


def _decode_bound(q, Kc, Vc, p, s_ref, P, ref):
    """_decode_bound of tests/test_prefill_attention_gpu.py (_attention_bound of tests/test_decode_ops_gpu.py), restated: the per-element
    bound on |o - ref| for the fp32 single-query kernels, in float64 (q [B, nkv, g, D], Kc / Vc [B, nkv, p + 1, D]).  A weight
    exp2(s_t - m) carries eta_t = ln2 [64 u c sum_j |q_j k_tj| + (T + 4) 2u (|s_t| + |m|)] + (T + 2) 2u relative (the fp32 dot product,
    the T = ceil((p + 1) / 64) rescalings, exp2); numerator and denominator gamma = (R + T + 16) u each, R = ceil((p + 1) / 16) rows per
    accumulator; one fp16 ulp of |ref| for the division and the final rounding."""
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


def _prefill_reference(q, kc, vc, p0):
    """_reference of tests/test_prefill_attention_gpu.py, restated: float64 causal softmax . V of fp16 inputs, q [B, nh, T, D], caches
    [B, nkv, >= p0 + T, D] -> (qd [B, nkv, g, T, D], Kd, Vd [B, nkv, n, D], vis [T, n], s in nats with -inf where masked, P, ref)."""
    B, nh, T, _ = q.shape
    nkv, n = kc.shape[1], p0 + T
    qd = q.double().view(B, nkv, nh // nkv, T, D)
    Kd, Vd = kc[:, :, :n].double(), vc[:, :, :n].double()
    vis = torch.arange(n, device=q.device)[None, :] <= (p0 + torch.arange(T, device=q.device))[:, None]
    s = torch.einsum("bkgtd,bknd->bkgtn", qd, Kd) * SCALE
    s = torch.where(vis, s, torch.full_like(s, float("-inf")))
    P = torch.softmax(s, -1)
    return qd, Kd, Vd, vis, s, P, torch.einsum("bkgtn,bknd->bkgtd", P, Vd)


def _prefill_bound(qd, Kd, Vd, vis, s, P, ref, p0):
    """_prefill_bound of tests/test_prefill_attention_gpu.py, restated (its derivation is there): query t sees pos0 + t + 1 rows in
    NT = ceil of that / 32 tiles; a weight carries eta_t = ln2 [64 u c sum_j |q_j k_tj| + (NT + 4) 2u (|s_t| + |m|)] + (NT + 2) 2u; P is
    rounded to fp16 for the second product (2^-11 sum p |v|, and 2^-25 sum |v| for weights below fp16's normal range); the fp32
    accumulations gamma = (43 NT + 2) u; one fp16 ulp of |ref| for the division and the final rounding."""
    T, n = vis.shape
    NT = torch.ceil((p0 + torch.arange(T, device=ref.device, dtype=torch.float64) + 1) / KV_ROWS)[:, None]
    c = SCALE * LOG2E
    S_abs = torch.einsum("bkgtd,bknd->bkgtn", qd.abs(), Kd.abs()) * c
    s2 = torch.where(vis, s * LOG2E, torch.zeros_like(s))
    m = (s * LOG2E).amax(-1, keepdim=True)
    eta = math.log(2) * (64 * U * S_abs + (NT + 4) * 2 * U * (s2.abs() + m.abs())) + (NT + 2) * 2 * U
    pv = torch.einsum("bkgtn,bknd->bkgtd", P, Vd.abs())
    dev = torch.einsum("bkgtn,bknd->bkgtd", P * eta, Vd.abs()) + (P * eta).sum(-1, keepdim=True) * ref.abs()
    gamma = (43 * NT + 2) * U
    seen = torch.cumsum(Vd.abs(), 2)[:, :, p0:p0 + T][:, :, None]
    return _ulp16(ref) + (gamma + 2.0 ** -11) * pv + 2.0 ** -25 * seen + dev


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def _decode_inputs(nh, nkv, B, pos, L, device, seed):
    g = torch.Generator(device=device).manual_seed(seed)
    qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
    kc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
    vc = torch.randn(B, nkv, L, D, generator=g, device=device).half()
    _poison_behind(kc, vc, pos)        # row pos[b] itself as well: the launch appends it
    return qkv, kc, vc


def _decode_against_shared(K_, device, nh, nkv, B, pos, L, word, float64=False, seed=0):
    """The per-sequence launch at `pos` (a list of B, values outside 0 .. L - 1 are to be skipped) against the shared launch at every distinct
    valid value; returns the number of sequences compared."""
    assert K_.attention_describe(B, nh, nkv, D, L).startswith(word), (word, K_.attention_describe(B, nh, nkv, D, L))
    cos, sin = _tables(L, device)
    qkv, kc0, vc0 = _decode_inputs(nh, nkv, B, pos, L, device, seed)
    pos_t = torch.tensor(pos, dtype=torch.int64, device=device)
    kc, vc = kc0.clone(), vc0.clone()
    out = torch.full((B, nh * D), SENTINEL, dtype=torch.float16, device=device)
    K_.rope_attention(qkv, cos, sin, pos_t, kc, vc, out, nh, nkv, D, per_sequence=True)
    torch.cuda.synchronize()
    kc_want, vc_want, out_want = kc0.clone(), vc0.clone(), torch.full_like(out, SENTINEL)
    compared = 0
    for v in sorted(set(p for p in pos if 0 <= p < L)):
        kcs, vcs = kc0.clone(), vc0.clone()
        outs = torch.full_like(out, SENTINEL)
        K_.rope_attention(qkv, cos, sin, torch.tensor([v], dtype=torch.int64, device=device), kcs, vcs, outs, nh, nkv, D)
        torch.cuda.synchronize()
        rows = [b for b in range(B) if pos[b] == v]
        compared += len(rows)
        out_want[rows] = outs[rows]
        kc_want[rows, :, v] = kcs[rows, :, v]
        vc_want[rows, :, v] = vcs[rows, :, v]
        assert torch.isfinite(outs[rows]).all(), (word, v, "the shared launch itself is not finite")
    assert _bits_equal(out, out_want), (word, "output rows", (_bits(out) != _bits(out_want)).any(-1).nonzero().flatten()[:8].tolist())
    assert _bits_equal(kc, kc_want), (word, "k cache", (_bits(kc) != _bits(kc_want)).flatten(1).any(-1).nonzero().flatten()[:8].tolist())
    assert _bits_equal(vc, vc_want), (word, "v cache", (_bits(vc) != _bits(vc_want)).flatten(1).any(-1).nonzero().flatten()[:8].tolist())
    if float64:
        group = nh // nkv
        worst = 0.0
        for v in sorted(set(pos)):
            rows = [b for b in range(B) if pos[b] == v]
            x = qkv[rows].view(len(rows), nh + 2 * nkv, D)
            q_rot = _rope_model(x[:, :nh], cos[v], sin[v])
            k_rot = _rope_model(x[:, nh:nh + nkv], cos[v], sin[v])
            assert _bits_equal(kc[rows, :, v], k_rot) and _bits_equal(vc[rows, :, v], x[:, nh + nkv:]), (word, v, "appended rows")
            qd = q_rot.double().view(len(rows), nkv, group, D)
            Kd, Vd = kc[rows, :, :v + 1].double(), vc[rows, :, :v + 1].double()
            s = torch.einsum("bkgd,bktd->bkgt", qd, Kd) * SCALE
            P = torch.softmax(s, -1)
            ref = torch.einsum("bkgt,bktd->bkgd", P, Vd)
            assert torch.isfinite(ref).all(), (word, v, "the float64 reference is not finite")
            bound = _decode_bound(qd, Kd, Vd, v, s, P, ref)
            err = (out[rows].view(len(rows), nkv, group, D).double() - ref).abs()
            worst = max(worst, float((err / bound).max()))
        print(f"[per-sequence decode] {nh}/{nkv} B={B} {word}: max err/bound {worst:.3f}")
        assert worst <= 1.0, (word, worst)
        assert torch.isfinite(out).all()
    return compared


@pytest.mark.parametrize("shape,word", DECODE_SHAPES, ids=[w.replace(" ", "_") for _, w in DECODE_SHAPES])
def test_decode_per_sequence_equals_the_shared_launch_bit_for_bit(K_, device, shape, word):
    """Each family at L = 320, the positions 0, 1, 63 .. 65, 127 .. 129, 255, 256, 319 assigned cyclically: output rows and appended cache rows
    bit-equal to the shared launch at that position, every other cache element untouched; (4, 4, 5) and (8, 1, 128) also within
    _decode_bound of float64 attention, all outputs finite."""
    nh, nkv, B = shape
    pos = [POSITIONS[b % len(POSITIONS)] for b in range(B)]
    assert _decode_against_shared(K_, device, nh, nkv, B, pos, L_DEC, word, float64=shape in FLOAT64_SHAPES, seed=B + nh) == B


def test_decode_vector_alu_group_of_four_in_a_fresh_process(device):
    """decode_rope_attention_gqa_kernel<4> is reached only with QUICK_AMD_ATTN_MFMA=0, read once per process: a child runs (8, 1, 128) and
    (4, 1, 256) through the same comparisons (checking the pick first) and exits non-zero on a mismatch."""
    env = dict(os.environ, QUICK_AMD_ATTN_MFMA="0")
    env.pop("QUICK_AMD_ATTN_WAVES", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "child"]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert "per-sequence child: 2 shapes equal" in r.stdout, r.stdout[-2000:]


def test_decode_skips_positions_outside_the_cache(K_, device):
    """pos = [-1, 0, L, L - 1, 7] on the flash kernel: sequences 0 and 2 leave their caches bit-unchanged and their output rows at the
    sentinel (_decode_against_shared expects exactly that of every position outside 0 .. L - 1); the other three match the shared launch."""
    L = L_DEC
    assert _decode_against_shared(K_, device, 4, 4, 5, [-1, 0, L, L - 1, 7], L, "flash heads=1 gsplit=1 waves=8", seed=77) == 3


# ------------------------------------------------------------------------------------------------
# rope_kv_write and prefill attention
# ------------------------------------------------------------------------------------------------
def _prefill_against_shared(K_, device, nh, nkv, pos0, T, L, float64=False, seed=0):
    """rope_kv_write and prefill_attention per sequence at `pos0` (values outside 0 .. L - T are to be skipped) against the shared pair at
    every valid value; returns the number of sequences compared."""
    B = len(pos0)
    cos, sin = _tables(L, device)
    g = torch.Generator(device=device).manual_seed(seed)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device).half()
    kc0 = torch.randn(B, nkv, L, D, generator=g, device=device).half()
    vc0 = torch.randn(B, nkv, L, D, generator=g, device=device).half()
    _poison_behind(kc0, vc0, pos0)     # the rows the launch writes as well: what stays behind pos0[b] + T - 1 is poison when attention runs
    pos_t = torch.tensor(pos0, dtype=torch.int64, device=device)
    kc, vc = kc0.clone(), vc0.clone()
    q = torch.full((B, nh, T, D), SENTINEL, dtype=torch.float16, device=device)
    att = torch.full((B * T, nh * D), SENTINEL, dtype=torch.float16, device=device)
    K_.rope_kv_write(qkv, cos, sin, pos_t, q, kc, vc, T, nh, nkv, D, per_sequence=True)
    torch.cuda.synchronize()
    kc_written, vc_written = kc.clone(), vc.clone()
    K_.prefill_attention(q, kc, vc, pos_t, att, nh, nkv, D, per_sequence=True)
    torch.cuda.synchronize()
    assert _bits_equal(kc, kc_written) and _bits_equal(vc, vc_written), "prefill attention wrote a cache"
    kc_want, vc_want, q_want, att_want = kc0.clone(), vc0.clone(), torch.full_like(q, SENTINEL), torch.full_like(att, SENTINEL)
    compared, worst = 0, 0.0
    for v in sorted(set(p for p in pos0 if 0 <= p <= L - T)):
        kcs, vcs = kc0.clone(), vc0.clone()
        qs, atts = torch.full_like(q, SENTINEL), torch.full_like(att, SENTINEL)
        one = torch.tensor([v], dtype=torch.int64, device=device)
        K_.rope_kv_write(qkv, cos, sin, one, qs, kcs, vcs, T, nh, nkv, D)
        K_.prefill_attention(qs, kcs, vcs, one, atts, nh, nkv, D)
        torch.cuda.synchronize()
        for b in (b for b in range(B) if pos0[b] == v):
            compared += 1
            q_want[b] = qs[b]
            att_want[b * T:(b + 1) * T] = atts[b * T:(b + 1) * T]
            kc_want[b, :, v:v + T] = kcs[b, :, v:v + T]
            vc_want[b, :, v:v + T] = vcs[b, :, v:v + T]
            assert torch.isfinite(atts[b * T:(b + 1) * T]).all(), (v, "the shared launch itself is not finite")
            if float64:
                qd, Kd, Vd, vis, s, P, ref = _prefill_reference(q[b:b + 1], kc[b:b + 1], vc[b:b + 1], v)
                assert torch.isfinite(ref).all(), (v, "the float64 reference is not finite")
                bound = _prefill_bound(qd, Kd, Vd, vis, s, P, ref, v)
                o = att[b * T:(b + 1) * T].double().view(1, T, nkv, nh // nkv, D).permute(0, 2, 3, 1, 4)
                worst = max(worst, float(((o - ref).abs() / bound).max()))
    for got, want, what in ((q, q_want, "q_out"), (kc, kc_want, "k cache"), (vc, vc_want, "v cache"), (att, att_want, "attention rows")):
        assert _bits_equal(got, want), (nh, nkv, T, what, (_bits(got) != _bits(want)).flatten(1).any(-1).nonzero().flatten()[:8].tolist())
    if float64:
        print(f"[per-sequence prefill] {nh}/{nkv} T={T}: max err/bound {worst:.3f}")
        assert worst <= 1.0, (nh, nkv, T, worst)
    return compared


@pytest.mark.parametrize("T", PREFILL_T)
@pytest.mark.parametrize("nh,nkv", PREFILL_HEADS)
def test_write_and_prefill_per_sequence_equal_the_shared_launches_bit_for_bit(K_, device, nh, nkv, T):
    """L = 192, pos0 = [0, 5, 31, 32, 100]: per sequence q_out, the written cache rows and the attention rows are the shared launches' at
    pos0 = [pos0[b]], untouched cache elements keep their bits; at T = 17 and 65 the attention rows also lie within _prefill_bound of
    float64 causal softmax . V."""
    n = _prefill_against_shared(K_, device, nh, nkv, list(PREFILL_POS0), T, L_PRE, float64=T in FLOAT64_T, seed=10 * T + nh)
    assert n == len(PREFILL_POS0)


@pytest.mark.parametrize("T", [17, 65])
def test_write_and_prefill_skip_positions_outside_the_cache(K_, device, T):
    """pos0 = [-1, L - T + 1, 0, L - T, 3]: sequences 0 and 1 keep q_out and attention rows at the sentinel and their caches bit for bit
    (_prefill_against_shared expects that of every start outside 0 .. L - T); the other three match the shared launches."""
    L = L_PRE
    assert _prefill_against_shared(K_, device, 4, 4, [-1, L - T + 1, 0, L - T, 3], T, L, seed=T) == 3


if __name__ == "__main__" and sys.argv[1:] == ["child"]:
    sys.path.insert(0, ROOT)
    dev = torch.device("cuda:0")
    kernels_ = _kernels()
    for (nh_, nkv_, B_), word_ in CHILD_SHAPES:
        pos_ = [POSITIONS[b % len(POSITIONS)] for b in range(B_)]
        assert _decode_against_shared(kernels_, dev, nh_, nkv_, B_, pos_, L_DEC, word_, float64=(nh_, nkv_, B_) in FLOAT64_SHAPES,
                                      seed=B_ + nh_) == B_
    print(f"per-sequence child: {len(CHILD_SHAPES)} shapes equal")
