"""The one-byte (OCP e4m3fn) KV cache on the GPU: the write bit for bit against quantize_kv of the fp16 launch's rows, the fused decode
step and the MFMA prefill against float64 attention over the DEQUANTISED bytes read back from the device within the fp16 kernels' error
models, T = 1 prefill against decode, reproducibility against the forcezero twin, and QuantAttentionFused(kv_cache_dtype="fp8_e4m3")
stage by stage, a captured decode step included.

Shapes are small: L = 512, B = 2..3, head_dim 128, groups of 1, 2, 4 and 8 query heads per KV head."""
import math

import numpy as np
import pytest
import torch

import test_prefill_attention_gpu as PF
from conftest import rel_err
from oracle import w4a16
from quick_amd import QuantAttentionFused, quantize_linear
from quick_amd.attention import dequantize_kv, quantize_kv
from test_decode_ops_gpu import _attention_bound, _check_guard, _poisoned, _rope_model, _tables

pytestmark = pytest.mark.gpu

D, L = 128, 512
U = 2.0 ** -24
SCALE = D ** -0.5
F8, U8 = torch.float8_e4m3fn, torch.uint8
GUARD = 0xA5
HEADS = [(4, 4), (8, 4), (8, 2), (8, 1)]                     # groups 1, 2, 4, 8 (the existing attention tests' pairs plus group 2)
SCALES = [(1.0, 1.0), (0.37, 2.0 ** -3)]                     # (k_scale, v_scale)
# The decode kernel: wave w of a workgroup takes the 16-row chunks that start at 16 w + 64 k, so a wave's trip count changes wherever p
# crosses a multiple of 16 (p = 15 | 16, 31 | 32, 47 | 48: waves 1, 2, 3 join; 63 | 64: wave 0's second trip, the first request of the
# second register set; 79 | 80, 95 | 96, 111 | 112: the second trips of waves 1, 2, 3; 127 | 128: wave 0's third trip, the first set again;
# 191 | 192 and 255 | 256: the sets alternating -- from there on every further multiple of 16 repeats one of these paths with a larger trip
# count, and L - 1 runs the longest).  One build per group.
DECODE_P = (0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 127, 128, 191, 192, 255, 256, L - 1)


@pytest.fixture(scope="module")
def K_(device):
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def tables(device):
    cos_np, sin_np = _tables(L, 1e4)
    return cos_np, sin_np, torch.from_numpy(cos_np).to(device), torch.from_numpy(sin_np).to(device)


def _u8(t):
    return t.contiguous().view(U8)


def _poison_behind(kb, vb, n):
    """Rows n.. of a byte cache hold what nobody may read: the NaN codes and +-448."""
    for i, code in enumerate((0x7F, 0xFF, 0x7E, 0xFE)):
        kb[:, :, n + i::4] = code
        vb[:, :, n + (i + 1) % 4::4] = code


def _edge_values(scale):
    """fp16 values around every decision of the quantiser at a power-of-two scale: the exact midpoints between neighbouring codes, values
    beyond 448 * scale, the subnormal range around the smallest code's midpoint, and zeros -- both signs of everything."""
    codes = torch.arange(0, 0x7E, dtype=U8)
    lo, hi = dequantize_kv(codes, 1.0), dequantize_kv(codes + 1, 1.0)
    tiny = 2.0 ** -10 * torch.tensor([0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0])
    v = torch.cat([(lo + hi) / 2, torch.tensor([448.0, 449.0, 480.0, 1000.0, 60000.0]), tiny, torch.zeros(1)]) * scale
    v = torch.cat([v, -v, torch.tensor([65504.0, -65504.0])])
    assert torch.equal(v.half().float(), v)          # (exactly representable in fp16)
    return v.half()


# ------------------------------------------------------------------------------------------------
# the write
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sequence", [False, True], ids=["shared", "per-sequence"])
@pytest.mark.parametrize("T", [1, 17, 130])
def test_write_is_quantize_kv_of_the_fp16_launch_bit_for_bit(K_, device, tables, T, per_sequence):
    """fp16 and fp8 rope_kv_write on the same inputs: the bytes equal quantize_kv of the fp16 launch's cache rows, q_out is bit-identical,
    every byte outside the written rows keeps its guard pattern (a skipped sequence: all of its bytes, and its q_out rows).  V (copied) and
    the K of position 0 (the identity rotation) carry the exact midpoints, saturating values, subnormals and zeros of _edge_values."""
    _, _, cos, sin = tables
    B, nh, nkv = 3, 8, 2
    ks, vs = 2.0 ** -3, 2.0 ** -5
    g = torch.Generator(device=device).manual_seed(100 + T)
    qkv = (torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device) * 3).half()
    ev_k, ev_v = _edge_values(ks).to(device), _edge_values(vs).to(device)
    n = ev_k.numel()
    assert n <= nkv * D + D
    flat_k = qkv[:, nh * D:(nh + nkv) * D]
    flat_v = qkv[:, (nh + nkv) * D:]
    for r in range(0, B * T, T):                          # token 0 of every sequence (position 0 where the start is 0)
        flat_k[r, :min(n, nkv * D)] = ev_k[:nkv * D]
        flat_v[r, :min(n, nkv * D)] = ev_v[:nkv * D]
    flat_v[T - 1, -(n - nkv * D):] = ev_v[nkv * D:]      # the tail of the list, elsewhere
    flat_k[0, -(n - nkv * D):] = ev_k[nkv * D:]
    if per_sequence:
        starts = [0, -1, L - T] if T < 130 else [0, L - T + 1, L - T]        # (one skipped sequence: before the cache / past its end)
        pos0 = torch.tensor(starts, dtype=torch.int64, device=device)
    else:
        starts = [0] * B if T != 17 else [199] * B                            # (position 0: the identity rotation, K keeps the edge values)
        pos0 = torch.tensor(starts[:1], dtype=torch.int64, device=device)
    kh = torch.zeros(B, nkv, L, D, dtype=torch.float16, device=device)
    vh = torch.zeros_like(kh)
    qh = torch.full((B, nh, T, D), 7.0, dtype=torch.float16, device=device)
    K_.rope_kv_write(qkv, cos, sin, pos0, qh, kh, vh, T, nh, nkv, D, per_sequence=per_sequence)
    kb = torch.full((B, nkv, L, D), GUARD, dtype=U8, device=device)
    vb = kb.clone()
    q8 = torch.full((B, nh, T, D), 7.0, dtype=torch.float16, device=device)
    K_.rope_kv_write(qkv, cos, sin, pos0, q8, kb.view(F8) if T != 17 else kb, vb.view(F8) if T != 17 else vb, T, nh, nkv, D,
                     per_sequence=per_sequence, k_scale=ks, v_scale=vs)     # (T = 17: the uint8 view is accepted as it is)
    torch.cuda.synchronize()
    assert torch.equal(qh.view(torch.int16), q8.view(torch.int16)), "q_out differs from the fp16 launch"
    k_want = torch.full_like(kb, GUARD)
    v_want = torch.full_like(vb, GUARD)
    for b, s in enumerate(starts):
        if 0 <= s <= L - T:
            k_want[b, :, s:s + T] = _u8(quantize_kv(kh[b, :, s:s + T], ks))
            v_want[b, :, s:s + T] = _u8(quantize_kv(vh[b, :, s:s + T], vs))
        else:
            assert bool((q8[b] == 7.0).all()), "a skipped sequence's q_out was written"
    assert torch.equal(kb, k_want), ("K bytes", T, per_sequence, int((kb != k_want).sum()))
    assert torch.equal(vb, v_want), ("V bytes", T, per_sequence, int((vb != v_want).sum()))
    seen = set(vb[0].flatten().tolist())
    assert {0x00, 0x80, 0x7E, 0xFE, 0x01, 0x81} <= seen, "the edge values did not reach the cache"


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def _decode_case(B, nh, nkv, ks, vs, seed, device):
    g = torch.Generator(device=device).manual_seed(seed)
    qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
    kb = _u8(quantize_kv(torch.randn(B, nkv, L, D, generator=g, device=device).half(), ks))
    vb = _u8(quantize_kv(torch.randn(B, nkv, L, D, generator=g, device=device).half(), vs))
    return qkv, kb, vb


def _decode_check(qkv, kb, vb, kb0, vb0, out, pos, nh, nkv, ks, vs, cos_np, sin_np, tag):
    """Per sequence b at position pos[b] (outside 0 .. L - 1: skipped -- out and caches untouched): the appended rows are quantize_kv of
    the RoPE model's rows, every other byte is as it was, and out is within _attention_bound (+ one fp32 rounding for the v_scale multiply)
    of float64 softmax(q K^T) V over the dequantised bytes read back from the device.  Returns max(err / bound)."""
    B, group, worst = qkv.shape[0], nh // nkv, 0.0
    qkv_np = qkv.cpu().numpy().reshape(B, nh + 2 * nkv, D)
    for b in range(B):
        p = int(pos[b])
        if p < 0 or p >= L:
            assert torch.equal(kb[b], kb0[b]) and torch.equal(vb[b], vb0[b]), (tag, b, "a skipped sequence's caches changed")
            assert bool((out[b] == 7.0).all()), (tag, b, "a skipped sequence's out was written")
            continue
        q_rot = torch.from_numpy(_rope_model(qkv_np[b, :nh], cos_np[p], sin_np[p])).to(qkv.device)
        k_rot = torch.from_numpy(_rope_model(qkv_np[b, nh:nh + nkv], cos_np[p], sin_np[p])).to(qkv.device)
        k_want, v_want = kb0[b].clone(), vb0[b].clone()
        k_want[:, p] = _u8(quantize_kv(k_rot, ks))
        v_want[:, p] = _u8(quantize_kv(qkv[b].view(nh + 2 * nkv, D)[nh + nkv:], vs))
        assert torch.equal(kb[b], k_want) and torch.equal(vb[b], v_want), (tag, b, p, "appended rows / bytes outside row p")
        Kd = dequantize_kv(kb[b:b + 1, :, :p + 1], ks).double()
        Vd = dequantize_kv(vb[b:b + 1, :, :p + 1], vs).double()
        qd = q_rot.double().view(1, nkv, group, D)
        s = torch.einsum("bkgd,bktd->bkgt", qd, Kd) * SCALE
        P = torch.softmax(s, -1)
        ref = torch.einsum("bkgt,bktd->bkgd", P, Vd)
        bound = _attention_bound(qd, Kd, Vd, p, s, P, ref) + U * ref.abs()
        err = (out[b].double().view(1, nkv, group, D) - ref).abs()
        assert not torch.isnan(err).any(), (tag, b, p, "NaN in the output: a poisoned row was read")
        worst = max(worst, float((err / bound).max()))
    return worst


@pytest.mark.parametrize("nh,nkv", HEADS, ids=[f"group{a // b}" for a, b in HEADS])
def test_decode_against_float64_over_the_dequantised_cache(K_, device, tables, nh, nkv):
    """Shared position, every p of DECODE_P, both scale pairs alternating; rows behind p hold NaN codes and +-448, row p a NaN code."""
    cos_np, sin_np, cos, sin = tables
    B = 2
    assert K_.attention_describe(B, nh, nkv, D, L, kv_cache_dtype="fp8_e4m3").startswith(f"gqa-mfma-fp8 heads={nh // nkv} gsplit=1")
    for i, p in enumerate(DECODE_P):
        ks, vs = SCALES[i % 2]
        qkv, kb, vb = _decode_case(B, nh, nkv, ks, vs, 7 * p + nh, device)
        _poison_behind(kb, vb, p)
        kb0, vb0 = kb.clone(), vb.clone()
        buf, out = _poisoned(B, (nh * D,), device)
        pos = torch.full((1,), p, dtype=torch.int64, device=device)
        K_.rope_attention(qkv, cos, sin, pos, kb.view(F8), vb.view(F8), out, nh, nkv, D, k_scale=ks, v_scale=vs)
        torch.cuda.synchronize()
        _check_guard(buf, B)
        ratio = _decode_check(qkv, kb, vb, kb0, vb0, out, [p] * B, nh, nkv, ks, vs, cos_np, sin_np, (nh, nkv, p))
        print(f"[fp8-decode] {nh}/{nkv} p={p} scales=({ks}, {vs}): max err/bound {ratio:.3f}")
        assert ratio <= 1.0, (nh, nkv, p, ratio)


@pytest.mark.parametrize("nh,nkv", HEADS, ids=[f"group{a // b}" for a, b in HEADS])
def test_decode_per_sequence_mixed_positions_and_skipped_slots(K_, device, tables, nh, nkv):
    """One launch, one position per sequence: mixed lengths, a sequence at -1 and one at L that leave out and both caches untouched."""
    cos_np, sin_np, cos, sin = tables
    for positions, (ks, vs) in (((-1, 130, L), SCALES[1]), ((L - 1, 0, 63), SCALES[0]), ((64, L, 17), SCALES[1])):
        B = len(positions)
        qkv, kb, vb = _decode_case(B, nh, nkv, ks, vs, sum(positions) + nh, device)
        for b, p in enumerate(positions):
            _poison_behind(kb[b:b + 1], vb[b:b + 1], max(min(p, L), 0))
        kb0, vb0 = kb.clone(), vb.clone()
        out = torch.full((B, nh * D), 7.0, dtype=torch.float16, device=device)
        pos = torch.tensor(positions, dtype=torch.int64, device=device)
        K_.rope_attention(qkv, cos, sin, pos, kb.view(F8), vb.view(F8), out, nh, nkv, D, per_sequence=True, k_scale=ks, v_scale=vs)
        torch.cuda.synchronize()
        ratio = _decode_check(qkv, kb, vb, kb0, vb0, out, positions, nh, nkv, ks, vs, cos_np, sin_np, (nh, nkv, positions))
        print(f"[fp8-decode-seq] {nh}/{nkv} pos={positions}: max err/bound {ratio:.3f}")
        assert ratio <= 1.0, (nh, nkv, positions, ratio)


def test_decode_appends_the_rows_the_write_launch_produces(K_, device, tables):
    """The same token at the same position through rope_kv_write (T = 1) and through the fused decode step: the same bytes in row p."""
    _, _, cos, sin = tables
    B, nh, nkv, p, ks, vs = 3, 8, 2, 77, 0.37, 2.0 ** -3
    qkv, _, _ = _decode_case(B, nh, nkv, ks, vs, 5, device)
    pos = torch.full((1,), p, dtype=torch.int64, device=device)
    caches = [torch.full((B, nkv, L, D), GUARD, dtype=U8, device=device) for _ in range(4)]
    K_.rope_kv_write(qkv, cos, sin, pos, torch.empty(B, nh, 1, D, dtype=torch.float16, device=device), caches[0].view(F8), caches[1].view(F8),
                     1, nh, nkv, D, k_scale=ks, v_scale=vs)
    for c in caches[2:]:
        c[:, :, :p] = 0x30
    out = torch.empty(B, nh * D, dtype=torch.float16, device=device)
    K_.rope_attention(qkv, cos, sin, pos, caches[2].view(F8), caches[3].view(F8), out, nh, nkv, D, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert torch.equal(caches[0][:, :, p], caches[2][:, :, p]) and torch.equal(caches[1][:, :, p], caches[3][:, :, p])
    assert bool((caches[0][:, :, p] != GUARD).any())


# ------------------------------------------------------------------------------------------------
# prefill
# ------------------------------------------------------------------------------------------------
def _prefill_case(B, nh, nkv, p0, T, variant, ks, vs, device):
    """The fp16 dense case of tests/test_prefill_attention_gpu.py, quantised: the peaked rows are beta x a query BEFORE quantisation and the
    reference is built on the dequantised K, so the peak that is checked is the one that survived.  Rows from pos0 + T on: NaN codes, +-448."""
    q, kc, vc = PF._dense_case(B, nh, nkv, p0, T, variant, device)
    n = p0 + T
    kb = torch.zeros(kc.shape, dtype=U8, device=device)
    vb = torch.zeros_like(kb)
    kb[:, :, :n] = _u8(quantize_kv(kc[:, :, :n], ks))
    vb[:, :, :n] = _u8(quantize_kv(vc[:, :, :n], vs))
    _poison_behind(kb, vb, n)
    return q, kb, vb


def _prefill_launch(K_, q, kb, vb, p0, nh, nkv, ks, vs, lib=None, per_sequence=False, pos=None):
    B, T = q.shape[0], q.shape[2]
    kb0, vb0 = kb.clone(), vb.clone()
    buf, out = _poisoned(B * T, (nh * D,), q.device)
    pos = torch.full((1,), p0, dtype=torch.int64, device=q.device) if pos is None else pos
    if lib is None:
        K_.prefill_attention(q, kb.view(F8), vb.view(F8), pos, out, nh, nkv, D, per_sequence=per_sequence, k_scale=ks, v_scale=vs)
    else:
        rc = lib.quick_prefill_attention_fp8(q.data_ptr(), kb.data_ptr(), vb.data_ptr(), pos.data_ptr(), out.data_ptr(), B, T, nh, nkv, D,
                                             kb.shape[2], SCALE, ks, vs, int(per_sequence), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    _check_guard(buf, B * T)
    assert torch.equal(kb, kb0) and torch.equal(vb, vb0), "the kernel wrote a cache"
    return out


def emulate_fp8_prefill(q, kb, vb, p0, ks, vs):
    """The fp8 prefill kernel's rounding points in torch on the CPU (PF._emulate with the byte cache): scores are fp32 sums of exact
    fp16 x byte products times the fp32 factor scale * log2 e * k_scale; max, exp2 and l in fp32; P rounded to fp16; P V per tile as one
    fp32 sum of exact products with the BYTE values onto the rescaled accumulator; one fp32 division, one fp32 multiply by v_scale, one
    rounding to fp16.  Returns [B, nkv, g, T, D] float64."""
    q, kb, vb = q.cpu(), kb.cpu(), vb.cpu()
    B, nh, T, _ = q.shape
    nkv = kb.shape[1]
    f32 = torch.float32
    kv, vv = dequantize_kv(kb, 1.0).double(), dequantize_kv(vb, 1.0).double()
    qd = q.double().view(B, nkv, nh // nkv, T, D)
    limit = (p0 + torch.arange(T))[:, None]
    m = torch.full((B, nkv, nh // nkv, T, 1), float("-inf"), dtype=f32)
    l = torch.zeros_like(m)
    acc = torch.zeros((B, nkv, nh // nkv, T, D), dtype=f32)
    c32 = torch.tensor(SCALE, dtype=f32) * torch.tensor(1.44269504088896, dtype=f32) * torch.tensor(ks, dtype=f32)
    for tile0 in range(0, p0 + T, PF.KV_ROWS):
        rows = torch.arange(tile0, tile0 + PF.KV_ROWS).clamp_max(p0 + T - 1)
        x = torch.einsum("bkgtd,bknd->bkgtn", qd, kv[:, :, rows]).to(f32) * c32
        x = torch.where(torch.arange(tile0, tile0 + PF.KV_ROWS)[None, :] <= limit, x, torch.full_like(x, float("-inf")))
        mb = torch.maximum(m, x.amax(-1, keepdim=True))
        mref = torch.where(torch.isinf(mb), torch.zeros_like(mb), mb)
        corr = torch.exp2(m - mref)
        e = torch.exp2(x - mref)
        l = l * corr + e.sum(-1, keepdim=True, dtype=f32)
        pv = torch.einsum("bkgtn,bknd->bkgtd", e.half().double(), vv[:, :, rows])
        acc = ((acc * corr).double() + pv).to(f32)
        m = mb
    return ((acc / l) * torch.tensor(vs, dtype=f32)).half().double()


def prefill_reference_and_bound(q, kb, vb, p0, ks, vs):
    """float64 causal softmax . V over the dequantised bytes and PF._prefill_bound applied to them."""
    qd, Kd, Vd, vis, s, P, ref = PF._reference(q, dequantize_kv(kb, ks).double(), dequantize_kv(vb, vs).double(), p0)
    return ref, PF._prefill_bound(qd, Kd, Vd, vis, s, P, ref, p0)


@pytest.mark.parametrize("nh,nkv", PF.HEADS)
def test_prefill_dense_against_float64_over_the_dequantised_cache(K_, device, nh, nkv):
    """The DENSE (pos0, T) cases, random and peaked, scale pairs alternating: max(err / bound) <= 1 with _prefill_bound on the dequantised
    cache; the emulation of the rounding points stays inside the same bound (its largest err / bound over these cases, all three head
    pairs: 0.63 random, 0.66 peaked -- the kernel's own figures agree with it to three digits)."""
    B = 2
    for i, (p0, T) in enumerate(PF.DENSE):
        for variant in ("random", "peaked"):
            ks, vs = SCALES[i % 2]
            q, kb, vb = _prefill_case(B, nh, nkv, p0, T, variant, ks, vs, device)
            out = _prefill_launch(K_, q, kb, vb, p0, nh, nkv, ks, vs)
            ref, bound = prefill_reference_and_bound(q, kb, vb, p0, ks, vs)
            emu = float(((emulate_fp8_prefill(q, kb, vb, p0, ks, vs).to(device) - ref).abs() / bound).max())
            err = (out.double().view(B, T, nkv, nh // nkv, D).permute(0, 2, 3, 1, 4) - ref).abs()
            ratio = float((err / bound).max())
            print(f"[fp8-prefill] {nh}/{nkv} pos0={p0} T={T} {variant} scales=({ks}, {vs}): max err/bound {ratio:.3f} (emulation {emu:.3f})")
            assert emu <= 1.0, ("the emulation of the rounding points leaves the bound", p0, T, variant, emu)
            assert ratio <= 1.0, (p0, T, variant, ratio)


def test_prefill_per_sequence_equals_the_shared_launch_and_skips(K_, device):
    """pos0 per sequence: each sequence's rows are bit for bit the shared launch's at its own start; a start outside 0 .. L - T is skipped."""
    nh, nkv, T, ks, vs = 8, 2, 17, 0.37, 2.0 ** -3
    starts = (200, L - T + 1, 65)
    q, kb, vb = _prefill_case(3, nh, nkv, 0, L, "random", ks, vs, device)
    q = q[:, :, :T].contiguous()
    for b, s in enumerate(starts):
        _poison_behind(kb[b:b + 1], vb[b:b + 1], min(s + T, L))
    out = torch.full((3 * T, nh * D), 7.0, dtype=torch.float16, device=device)
    K_.prefill_attention(q, kb.view(F8), vb.view(F8), torch.tensor(starts, dtype=torch.int64, device=device), out, nh, nkv, D,
                         per_sequence=True, k_scale=ks, v_scale=vs)
    torch.cuda.synchronize()
    assert bool((out[T:2 * T] == 7.0).all()), "a skipped sequence's rows were written"
    for b in (0, 2):
        one = _prefill_launch(K_, q[b:b + 1].contiguous(), kb[b:b + 1].contiguous(), vb[b:b + 1].contiguous(), starts[b], nh, nkv, ks, vs)
        assert PF._bits_equal(out[b * T:(b + 1) * T], one), b


@pytest.mark.parametrize("nh,nkv", HEADS, ids=[f"group{a // b}" for a, b in HEADS])
def test_single_token_prefill_agrees_with_decode_on_the_same_bytes(K_, device, tables, nh, nkv):
    """The decode step appends row p and attends rows 0 .. p; a T = 1 prefill of the same rotated query over the cache it left agrees
    within the sum of both bounds."""
    cos_np, sin_np, cos, sin = tables
    B, (ks, vs) = 3, SCALES[1]
    for p in (0, 31, 32, 200, L - 1):
        qkv, kb, vb = _decode_case(B, nh, nkv, ks, vs, 11 * p + nh, device)
        _poison_behind(kb, vb, p)
        pos = torch.full((1,), p, dtype=torch.int64, device=device)
        dec = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, pos, kb.view(F8), vb.view(F8), dec, nh, nkv, D, k_scale=ks, v_scale=vs)
        q_rot = torch.from_numpy(_rope_model(qkv.cpu().numpy().reshape(B, nh + 2 * nkv, D)[:, :nh], cos_np[p], sin_np[p])).to(device)
        q = q_rot.view(B, nh, 1, D).contiguous()
        out = _prefill_launch(K_, q, kb, vb, p, nh, nkv, ks, vs)
        ref, bound = prefill_reference_and_bound(q, kb, vb, p, ks, vs)
        qd, Kd, Vd, vis, s, P, _ = PF._reference(q, dequantize_kv(kb, ks).double(), dequantize_kv(vb, vs).double(), p)
        bound = bound[:, :, :, 0] + _attention_bound(qd[:, :, :, 0], Kd, Vd, p, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0]) + \
            U * ref[:, :, :, 0].abs()
        diff = (out.double().view(B, nkv, nh // nkv, D) - dec.double().view(B, nkv, nh // nkv, D)).abs()
        assert float((diff / bound).max()) <= 1.0, (p, float((diff / bound).max()))


# ------------------------------------------------------------------------------------------------
# reproducibility
# ------------------------------------------------------------------------------------------------
def test_fp8_launches_are_reproducible_and_equal_their_forcezero_build(K_, device, tables):
    """Write, decode (every group) and prefill: two launches give bit-equal results, and so does the -amdgpu-waitcnt-forcezero build."""
    from quick_amd import _lib
    from quick_amd.build import FORCEZERO_LIB
    other = _lib.load_other(FORCEZERO_LIB)
    _, _, cos, sin = tables
    st = torch.cuda.current_stream().cuda_stream
    ks, vs = SCALES[1]
    for nh, nkv in HEADS:
        B, p = 2, 200
        qkv, kb, vb = _decode_case(B, nh, nkv, ks, vs, nh + nkv, device)
        pos = torch.full((1,), p, dtype=torch.int64, device=device)
        got = []
        for lib in (_lib.load(), _lib.load(), other):
            k1, v1 = kb.clone(), vb.clone()
            out = torch.empty(B, nh * D, dtype=torch.float16, device=device)
            rc = lib.quick_decode_rope_attention_fp8(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), k1.data_ptr(), v1.data_ptr(),
                                                     out.data_ptr(), B, nh, nkv, D, L, SCALE, ks, vs, 0, st)
            assert rc == 0, rc
            torch.cuda.synchronize()
            got.append((out, k1, v1))
        for a, b in zip(got[0], got[1]):
            assert torch.equal(a.view(U8), b.view(U8)), (nh, nkv, "two decode launches differ")
        for a, z in zip(got[0], got[2]):
            assert torch.equal(a.view(U8), z.view(U8)), (nh, nkv, "decode: the forcezero build differs")
    # write, T = 17 at 65
    B, nh, nkv, T = 2, 8, 2, 17
    g = torch.Generator(device=device).manual_seed(3)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device).half()
    pos = torch.full((1,), 65, dtype=torch.int64, device=device)
    got = []
    for lib in (_lib.load(), _lib.load(), other):
        k1 = torch.full((B, nkv, L, D), GUARD, dtype=U8, device=device)
        v1, q1 = k1.clone(), torch.empty(B, nh, T, D, dtype=torch.float16, device=device)
        rc = lib.quick_rope_kv_write_fp8(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), q1.data_ptr(), k1.data_ptr(),
                                         v1.data_ptr(), B, T, nh, nkv, D, L, ks, vs, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        got.append((q1, k1, v1))
    for other_run in got[1:]:
        for a, b in zip(got[0], other_run):
            assert torch.equal(a.view(U8), b.view(U8)), "write: launches / forcezero build differ"
    # prefill
    for (nh, nkv), (p0, T) in zip(PF.HEADS, PF.DENSE[:3]):
        q, kb, vb = _prefill_case(2, nh, nkv, p0, T, "random", ks, vs, device)
        a = _prefill_launch(K_, q, kb, vb, p0, nh, nkv, ks, vs)
        b = _prefill_launch(K_, q, kb, vb, p0, nh, nkv, ks, vs)
        z = _prefill_launch(K_, q, kb, vb, p0, nh, nkv, ks, vs, lib=other)
        assert PF._bits_equal(a, b), (nh, nkv, p0, T, "two launches differ")
        assert PF._bits_equal(a, z), (nh, nkv, p0, T, "the forcezero build differs")


# ------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------
TOL = 2e-3      # the existing module tests' o_proj tolerance (tests/test_attention_module_gpu.py)
MAXLEN = 64
CALLS = (19, 1, 1, 1, 5)      # a 19-token prefill, three decode steps, a 5-token chunk


def _module(hidden, nh, nkv, device, per_sequence, ks, vs, monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "2")
    g = torch.Generator().manual_seed(hidden + nkv)
    lin = lambda n_out: torch.nn.Linear(hidden, n_out, bias=False, dtype=torch.float16)
    qkv_lin, o_lin = lin((nh + 2 * nkv) * D), lin(hidden)
    qkv_lin.weight.data = (torch.randn(qkv_lin.weight.shape, generator=g) * 0.06).half()
    o_lin.weight.data = (torch.randn(o_lin.weight.shape, generator=g) * 0.04).half()
    qkv, o = quantize_linear(qkv_lin, 4, 128).to(device), quantize_linear(o_lin, 4, 128).to(device)
    o_logical = w4a16.unpack_mi355x(*[t.cpu().numpy() for t in (o.qweight, o.scales, o.qzeros)])
    m = QuantAttentionFused(hidden, nh, nkv, qkv, o, device, MAXLEN, per_sequence=per_sequence, kv_cache_dtype="fp8_e4m3", k_scale=ks, v_scale=vs)
    assert m.k_cache.dtype == F8 and m.k_cache.numel() * m.k_cache.element_size() == 2 * nkv * MAXLEN * D
    x = torch.randn(2, sum(CALLS), hidden, generator=g).half().to(device)
    return m, o_logical, x


class _Model:
    """The torch model of the module: per sequence its position and its cache rows as quantize_kv of the RoPE model's rows; attention in
    float64 over the dequantised rows."""

    def __init__(self, m, B):
        self.m, self.pos = m, [0] * B
        self.kb = torch.zeros(B, m.n_kv_heads, MAXLEN, D, dtype=U8, device=m.k_cache.device)
        self.vb = torch.zeros_like(self.kb)

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
            self.kb[b, :, p0:p0 + T] = _u8(quantize_kv(torch.from_numpy(_rope_model(rows[:, nh:nh + nkv], c, s)).to(dev).transpose(0, 1), m.k_scale))
            self.vb[b, :, p0:p0 + T] = _u8(quantize_kv(qkv[b, :, nh + nkv:].transpose(0, 1), m.v_scale))
            # the module's bytes: rows 0 .. p0 + T - 1 (all T rows of a padded chunk are written)
            assert torch.equal(_u8(m.k_cache)[b, :, :p0 + T], self.kb[b, :, :p0 + T]), (b, p0, T, "K bytes")
            assert torch.equal(_u8(m.v_cache)[b, :, :p0 + T], self.vb[b, :, :p0 + T]), (b, p0, T, "V bytes")
            if n:
                q1, k1, v1 = q_rot[:, :, :n].contiguous(), self.kb[b:b + 1], self.vb[b:b + 1]
                qd, Kd, Vd, vis, sc, P, ref = PF._reference(q1, dequantize_kv(k1, m.k_scale).double(), dequantize_kv(v1, m.v_scale).double(), p0)
                if T > 1:
                    bound = PF._prefill_bound(qd, Kd, Vd, vis, sc, P, ref, p0)
                else:
                    bound = (_attention_bound(qd[:, :, :, 0], Kd, Vd, p0, sc[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0]) +
                             U * ref[:, :, :, 0].abs())[:, :, :, None]
                got = attention_weight[b, :n].double().view(1, n, nkv, nh // nkv, D).permute(0, 2, 3, 1, 4)
                worst = max(worst, float(((got - ref).abs() / bound).max()))
                want = attention_weight[b, :n].double().cpu().numpy() @ w4a16.dequantize(*o_logical, 128).astype(np.float64)
                err = rel_err(attn_output[b, :n].float().cpu().numpy(), want)
                assert err <= TOL, (b, p0, T, err)
            self.pos[b] += n
        return worst


@pytest.mark.parametrize("per_sequence", [False, True], ids=["shared", "per-sequence"])
@pytest.mark.parametrize("hidden,nh,nkv", [(512, 4, 4), (512, 4, 2)], ids=["group1", "group2"])
def test_module_with_a_byte_cache_stage_by_stage(device, monkeypatch, hidden, nh, nkv, per_sequence):
    """A 19-token prefill, three decode steps, a 5-token chunk (per_sequence: ragged new_tokens) on quantize_linear-made projections.
    Every call: the cache bytes equal quantize_kv of the RoPE model's rows of the module's own qkv output (the rows of this single
    forward, where the qkv GEMM outputs agree trivially), the attention in front of o_proj is within the kernels' bounds of float64
    attention over the dequantised bytes, o_proj within 2e-3 of the oracle's GEMM.  Then one decode step captured in a graph and replayed
    twice with the positions advancing on the device: the replays append the bytes and return the outputs of eager steps."""
    ks, vs = SCALES[1]
    m, o_logical, x = _module(hidden, nh, nkv, device, per_sequence, ks, vs, monkeypatch)
    B = 2
    model = _Model(m, B)
    ragged = {19: [19, 12], 5: [3, 5]}
    at = bound_pos = 0
    for T in CALLS:
        counts = ragged.get(T, [T] * B) if per_sequence else [T] * B
        seen = []
        hook = m.qkv_proj.register_forward_hook(lambda mod, inp, out: seen.append(out))
        try:
            kw = dict(new_tokens=counts) if per_sequence else {}
            attn_output, attention_weight, past = m(x[:, at:at + T], **kw)
        finally:
            hook.remove()
        torch.cuda.synchronize()
        ratio = model.step(seen[0], counts, attention_weight, attn_output, o_logical)
        print(f"[fp8-module] {nh}/{nkv} per_sequence={per_sequence} T={T}: attention err/bound {ratio:.3f}")
        assert ratio <= 1.0, (T, ratio)
        assert m.pos.tolist() == (model.pos if per_sequence else model.pos[:1])
        bound_pos += max(counts)
        assert tuple(past[0].shape) == (1, 1, m.start_pos, 1) and m.start_pos == bound_pos
        at += T
    # a captured decode step, replayed twice; an identical module runs the same two steps eagerly from the same state
    xs = x[:, :3].contiguous()
    static = xs[:, :1].clone()
    state = (m.pos.clone(), _u8(m.k_cache).clone(), _u8(m.v_cache).clone(), m.start_pos)

    def restore():
        m.pos.copy_(state[0])
        _u8(m.k_cache).copy_(state[1])
        _u8(m.v_cache).copy_(state[2])
        m.start_pos = state[3]
    eager = []
    for i in (1, 2):
        eager.append(m(xs[:, i:i + 1].contiguous())[0].clone())
    k_eager, v_eager, pos_eager = _u8(m.k_cache).clone(), _u8(m.v_cache).clone(), m.pos.clone()
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
        assert torch.equal(out_static.view(torch.int16), eager[i - 1].view(torch.int16)), ("replay", i)
    assert torch.equal(m.pos, pos_eager) and torch.equal(_u8(m.k_cache), k_eager) and torch.equal(_u8(m.v_cache), v_eager)


# ------------------------------------------------------------------------------------------------
# the synthetic stack
# ------------------------------------------------------------------------------------------------
def test_synthetic_decoder_runs_on_byte_caches(device):
    """SyntheticDecoder("tiny", kv_cache_dtype="fp8_e4m3") next to the fp16 decoder of the same seed on the same tokens: a 19-token
    forward(hip_attention=True) and three decode_step_fused steps.  Layer 0 sees the same hidden states in both decoders, so its qkv GEMM
    outputs agree bit for bit and its cache bytes must equal quantize_kv of the fp16 decoder's rows -- prefill rows and appended rows;
    every layer's written rows hold no NaN code and the rows behind the position keep their guard byte.  The per-sequence form of the step
    (pos of B elements, all equal) gives bit for bit the shared step's tokens, hidden state and cache bytes, and a second forward repeats
    the first bit for bit.  The hidden state's distance to the fp16 decoder's is printed, not asserted (it is the format's error, not the
    kernels').  The eager paths of forward refuse a byte cache."""
    from quick_amd.decoder import CONFIGS, SyntheticDecoder, decode_step_fused
    B, Lc, ctx, steps = 2, 48, 19, 3
    ks, vs = 2.0 ** -5, 2.0 ** -7
    kw = dict(kv_cache_dtype="fp8_e4m3", k_scale=ks, v_scale=vs)
    m16 = SyntheticDecoder(CONFIGS["tiny"], batch=B, max_len=Lc, device=device, seed=3)
    m8 = SyntheticDecoder(CONFIGS["tiny"], batch=B, max_len=Lc, device=device, seed=3, **kw)
    m8s = SyntheticDecoder(CONFIGS["tiny"], batch=B, max_len=Lc, device=device, seed=3, **kw)
    assert m8.layers[0]["k"].dtype == F8 and m16.layers[0]["k"].dtype == torch.float16
    for m in (m8, m8s):
        for l in m.layers:
            _u8(l["k"]).fill_(GUARD)
            _u8(l["v"]).fill_(GUARD)
    toks = torch.randint(0, 512, (B, ctx + steps), generator=torch.Generator().manual_seed(9)).to(device)
    arange = torch.arange(ctx, device=device)
    with pytest.raises(ValueError, match="one-byte KV cache"):
        m8.forward(toks[:, :ctx], arange, None)                       # (SDPA over the cache: fp16 only)
    with pytest.raises(ValueError, match="one-byte KV cache"):
        m8.forward(toks[:, :ctx], arange, None, hip_glue=False)
    t16, h16 = m16.forward(toks[:, :ctx], arange, None, hip_attention=True, return_hidden=True)
    t8, h8 = m8.forward(toks[:, :ctx], arange, None, hip_attention=True, return_hidden=True)
    t8b, h8b = m8s.forward(toks[:, :ctx], arange, None, hip_attention=True, return_hidden=True)
    torch.cuda.synchronize()
    assert torch.equal(t8, t8b) and torch.equal(h8.view(torch.int16), h8b.view(torch.int16))
    assert torch.isfinite(h8.float()).all()
    print(f"[fp8-decoder] prefill: hidden fp8 - fp16 cache, largest / largest {float((h8.float() - h16.float()).abs().max() / h16.float().abs().max()):.4f}")

    def check_rows(lo, hi):
        l8, l16 = m8.layers[0], m16.layers[0]
        assert torch.equal(_u8(l8["k"])[:, :, lo:hi], _u8(quantize_kv(l16["k"][:, :, lo:hi], ks))), ("layer 0 K bytes", lo, hi)
        assert torch.equal(_u8(l8["v"])[:, :, lo:hi], _u8(quantize_kv(l16["v"][:, :, lo:hi], vs))), ("layer 0 V bytes", lo, hi)
        for l in m8.layers:
            for c in (_u8(l["k"]), _u8(l["v"])):
                assert bool(((c[:, :, :hi] & 0x7F) != 0x7F).all()), "a NaN code in a written row"
                assert bool((c[:, :, hi:] == GUARD).all()), "a row behind the position was written"
    check_rows(0, ctx)
    for i in range(steps):
        p = ctx + i
        tok = toks[:, p].contiguous()
        one = torch.full((1,), p, dtype=torch.int64, device=device)
        each = torch.full((B,), p, dtype=torch.int64, device=device)
        _, g16 = decode_step_fused(m16, tok, one)
        n8, g8 = decode_step_fused(m8, tok, one)
        n8s, g8s = decode_step_fused(m8s, tok, each)
        torch.cuda.synchronize()
        check_rows(p, p + 1)
        assert torch.isfinite(g8.float()).all()
        assert torch.equal(n8, n8s) and torch.equal(g8.view(torch.int16), g8s.view(torch.int16)), ("per-sequence step differs", p)
        for la, lb in zip(m8.layers, m8s.layers):
            assert torch.equal(_u8(la["k"]), _u8(lb["k"])) and torch.equal(_u8(la["v"]), _u8(lb["v"])), ("per-sequence caches differ", p)
        print(f"[fp8-decoder] step at {p}: hidden fp8 - fp16 cache, largest / largest {float((g8.float() - g16.float()).abs().max() / g16.float().abs().max()):.4f}")
