"""Sliding-window attention over a ring KV cache, host side: the exported symbols and their refusals with no GPU present, the describe
words, ring_rows / ring_slot / window_attention_reference as the restatement of the launches (against the full causal float64 reference
and against torch SDPA with an explicit banded mask over a wrapped ring), the module's constructor, and the GPU suite's emulations of the
kernels' rounding points against the bounds they are held to there."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from quick_amd import QuantAttentionFused, WQLinear_QUICK, _lib, kernels
from quick_amd.attention import ring_rows, ring_slot, window_attention_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 4
P16 = ctypes.c_void_p(1 << 40)      # never dereferenced: every call below is refused first
NAMES = ("quick_rope_kv_write_win_f16", "quick_decode_rope_attention_win_f16", "quick_prefill_attention_win_f16", "quick_attention_win_describe")


def test_symbols_are_exported_with_the_declared_signatures():
    header = open(os.path.join(ROOT, "include", "quick_amd.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    lib = _lib.load()
    assert lib.quick_amd_abi_version() == 1
    c_types = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float,
               "char*": ctypes.c_char_p, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        m = re.search(r"int " + name + r"\(([^)]*)\);", flat)
        assert m, name
        declared = [c_types[a.strip().rsplit(" ", 1)[0]] for a in m.group(1).split(",")]
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and args == declared, (name, args, declared)
    for fn in (kernels.rope_kv_write, kernels.rope_attention, kernels.prefill_attention):
        sig = inspect.signature(fn).parameters
        assert sig["window"].default is None and sig["table_rows"].default is None and sig["per_sequence"].default is False


def test_refusals_come_back_before_any_gpu_work():
    """Every refusal of the header's table with its code and a sentence; null pointers unless the pointers are the subject (then fake
    addresses: the call is refused before anything could read them)."""
    lib = _lib.load()
    n7, buf = [None] * 7, ctypes.create_string_buffer(160)
    write = lambda ptrs, B, T, nh, nkv, D, R, NP, seq=0: lib.quick_rope_kv_write_win_f16(*ptrs, B, T, nh, nkv, D, R, NP, seq, None)
    decode = lambda ptrs, B, nh, nkv, D, R, W, NP, seq=0: lib.quick_decode_rope_attention_win_f16(*ptrs, B, nh, nkv, D, R, W, NP, 0.1, seq, None)
    prefill = lambda ptrs, B, T, nh, nkv, D, R, W, NP, seq=0: lib.quick_prefill_attention_win_f16(*ptrs, B, T, nh, nkv, D, R, W, NP, 0.1, seq, None)
    describe = lambda B, T, nh, nkv, D, R, W, NP: lib.quick_attention_win_describe(B, T, nh, nkv, D, R, W, NP, buf, len(buf))

    def refused(rc, code, words):
        msg = _lib.last_error()
        assert rc == code and msg and words in msg and "window" in msg, (rc, code, msg)

    for seq in (0, 1):
        # a size <= 0, window < 1
        for B, T, nh, nkv, R, NP in ((0, 4, 8, 2, 64, 512), (1, 0, 8, 2, 64, 512), (1, 4, 0, 2, 64, 512), (1, 4, 8, 0, 64, 512),
                                     (1, 4, 8, 2, 0, 512), (1, 4, 8, 2, 64, 0), (-1, 4, 8, 2, 64, 512)):
            refused(write(n7, B, T, nh, nkv, 128, R, NP, seq), INVALID, "must be positive")
            refused(prefill(n7[:5], B, T, nh, nkv, 128, R, 16, NP, seq), INVALID, "must be positive")
            assert describe(B, T, nh, nkv, 128, R, 16, NP) == INVALID
            if T:
                refused(decode(n7, B, nh, nkv, 128, R, 16, NP, seq), INVALID, "must be positive")
        for W in (0, -3):
            refused(decode(n7, 1, 8, 2, 128, 64, W, 512, seq), INVALID, "window must be at least 1")
            refused(prefill(n7[:5], 1, 4, 8, 2, 128, 64, W, 512, seq), INVALID, "window must be at least 1")
        # window > ring_rows, tokens > ring_rows, tokens > table_rows
        refused(decode(n7, 1, 8, 2, 128, 64, 65, 512, seq), INVALID, "window > ring_rows")
        refused(prefill(n7[:5], 1, 4, 8, 2, 128, 64, 65, 512, seq), INVALID, "window > ring_rows")
        refused(write(n7, 1, 65, 8, 2, 128, 64, 512, seq), INVALID, "tokens > ring_rows")
        refused(prefill(n7[:5], 1, 65, 8, 2, 128, 64, 1, 512, seq), INVALID, "tokens > ring_rows")
        refused(write(n7, 1, 33, 8, 2, 128, 64, 32, seq), INVALID, "tokens > table_rows")
        refused(prefill(n7[:5], 1, 33, 8, 2, 128, 64, 1, 32, seq), INVALID, "tokens > table_rows")
        # the ring rule: window + tokens - 1 == ring_rows is accepted up to the pointer check, one more is refused
        refused(prefill(n7[:5], 1, 25, 8, 2, 128, 64, 40, 512, seq), INVALID, "null pointer")
        refused(prefill(n7[:5], 1, 26, 8, 2, 128, 64, 40, 512, seq), INVALID, "window + tokens - 1 > ring_rows")
        refused(prefill(n7[:5], 1, 25, 8, 2, 128, 64, 41, 512, seq), INVALID, "window + tokens - 1 > ring_rows")
        refused(decode(n7, 1, 8, 2, 128, 64, 64, 512, seq), INVALID, "null pointer")              # (one token: W <= R is the rule)
        # ... and a ring that can never wrap (ring_rows >= table_rows) takes any chunk that fits it
        refused(prefill(n7[:5], 1, 64, 8, 2, 128, 64, 64, 64, seq), INVALID, "null pointer")
        refused(prefill(n7[:5], 1, 26, 8, 2, 128, 64, 40, 60, seq), INVALID, "null pointer")
        refused(prefill(n7[:5], 1, 26, 8, 2, 128, 64, 40, 65, seq), INVALID, "window + tokens - 1 > ring_rows")
        # head_dim, n_heads % n_kv_heads, the decode groups, the grid limits
        for D in (64, 127, 256):
            refused(write(n7, 1, 4, 8, 2, D, 64, 512, seq), UNSUPPORTED, "head_dim must be 128")
            refused(decode(n7, 1, 8, 2, D, 64, 16, 512, seq), UNSUPPORTED, "head_dim must be 128")
            refused(prefill(n7[:5], 1, 4, 8, 2, D, 64, 16, 512, seq), UNSUPPORTED, "head_dim must be 128")
        refused(write(n7, 1, 4, 8, 3, 128, 64, 512, seq), UNSUPPORTED, "multiple of n_kv_heads")
        refused(decode(n7, 1, 8, 3, 128, 64, 16, 512, seq), UNSUPPORTED, "multiple of n_kv_heads")
        refused(prefill(n7[:5], 1, 4, 8, 3, 128, 64, 16, 512, seq), UNSUPPORTED, "multiple of n_kv_heads")
        for nh, nkv in ((3, 1), (12, 2), (16, 1), (48, 16)):
            refused(decode(n7, 1, nh, nkv, 128, 64, 16, 512, seq), UNSUPPORTED, "1, 2, 4 or 8 query heads per KV head")
            assert describe(1, 1, nh, nkv, 128, 64, 16, 512) == UNSUPPORTED
            refused(prefill(n7[:5], 1, 4, nh, nkv, 128, 64, 16, 512, seq), INVALID, "null pointer")     # (the prefill serves any group)
        refused(write(n7, 256, 257, 8, 2, 128, 512, 1024, seq), UNSUPPORTED, "65535")
        refused(decode(n7, 65536, 8, 2, 128, 64, 16, 512, seq), UNSUPPORTED, "65535")
        refused(prefill(n7[:5], 65536, 4, 8, 2, 128, 64, 16, 512, seq), UNSUPPORTED, "65535")
        # pointers: each one null
        for count, call in ((7, lambda p: write(p, 1, 4, 8, 2, 128, 64, 512, seq)), (7, lambda p: decode(p, 1, 8, 2, 128, 64, 16, 512, seq)),
                            (5, lambda p: prefill(p, 1, 4, 8, 2, 128, 64, 16, 512, seq))):
            for i in range(count):
                ptrs = [P16] * count
                ptrs[i] = None
                refused(call(ptrs), INVALID, "null pointer")
    # the order of the table: an argument error is answered before an unsupported shape
    refused(prefill(n7[:5], 1, 4, 8, 2, 64, 64, 65, 512), INVALID, "window > ring_rows")


def test_describe_words():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(160)
    assert lib.quick_attention_win_describe(64, 1, 32, 8, 128, 4607, 4096, 32768, buf, len(buf)) == 0
    assert buf.value.decode() == "decode-win-mfma heads=4 waves=4 set_rows=64 ring_rows=4607 window=4096 grid=8x64"
    assert lib.quick_attention_win_describe(2, 128, 32, 8, 128, 4607, 4096, 32768, buf, len(buf)) == 0
    assert buf.value.decode() == "prefill-win-mfma q_rows=64 kv_rows=32 waves=4 ring_rows=4607 window=4096 grid=2x32x2"
    assert kernels.window_attention_describe(1, 1, 32, 32, 128, 4096, 4096, 4096).startswith("decode-win-mfma heads=1 ")
    assert kernels.window_attention_describe(1, 512, 32, 32, 128, 4096, 4096, 4096).startswith("prefill-win-mfma ")
    assert lib.quick_attention_win_describe(1, 1, 8, 2, 128, 64, 16, 512, None, 0) == INVALID
    with pytest.raises(ValueError, match="window \\+ tokens - 1 > ring_rows"):
        kernels.window_attention_describe(1, 513, 32, 8, 128, 4607, 4096, 32768)
    with pytest.raises(NotImplementedError, match="head_dim"):
        kernels.window_attention_describe(1, 1, 32, 8, 64, 4607, 4096, 32768)


def test_ring_rows_and_ring_slot():
    assert ring_rows(4096, 512, 32768) == 4607 and ring_rows(4096, 512, 4096) == 4096 and ring_rows(40, 24, 256) == 63
    assert ring_rows(1, 1, 10) == 1 and ring_rows(8, 1, 100) == 8
    for bad in ((0, 1, 10), (1, 0, 10), (1, 1, 0), (-4, 8, 10)):
        with pytest.raises(ValueError):
            ring_rows(*bad)
    assert [ring_slot(p, 80) for p in (0, 79, 80, 81, 200)] == [0, 79, 0, 1, 40]
    assert ring_slot(torch.arange(78, 83), 80).tolist() == [78, 79, 0, 1, 2]
    with pytest.raises(ValueError):
        ring_slot(3, 0)
    # the ring rule, by brute force: after a chunk of T = prefill_chunk tokens at any pos0, every position a query of the chunk attends
    # is still the last position written to its row
    W, C, N = 7, 5, 64
    R = ring_rows(W, C, N)
    for p0 in range(0, N - C + 1):
        owner = {}
        for j in range(p0 + C):
            owner[ring_slot(j, R)] = j
        for t in range(C):
            for j in range(max(0, p0 + t - W + 1), p0 + t + 1):
                assert owner[ring_slot(j, R)] == j, (p0, t, j)


def _ring_of(lin, lo, hi, R, fill):
    ring = torch.full(lin.shape[:2] + (R, lin.shape[3]), fill, dtype=lin.dtype)
    span = torch.arange(lo, hi + 1)
    ring[:, :, ring_slot(span, R)] = lin[:, :, span]
    return ring


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2)])
def test_reference_equals_the_full_causal_reference_when_the_window_covers_everything(nh, nkv):
    import test_prefill_attention_gpu as PF
    g = torch.Generator().manual_seed(nh)
    B, T, p0, L = 2, 17, 30, 64
    q = torch.randn(B, nh, T, 128, generator=g).half()
    kc, vc = torch.randn(B, nkv, L, 128, generator=g).half(), torch.randn(B, nkv, L, 128, generator=g).half()
    *_, ref = PF._reference(q, kc, vc, p0)
    want = PF._rows_out(ref, B, T, nh)
    for W in (p0 + T, p0 + T + 5, 1000):
        got = window_attention_reference(q, kc, vc, p0, W)
        assert got.dtype == torch.float64 and tuple(got.shape) == (B * T, nh * 128)
        assert float((got - want).abs().max()) < 1e-13
    assert float((window_attention_reference(q, kc, vc, p0, p0 + T - 1) - want).abs().max()) > 1e-6     # one row fewer: another result


@pytest.mark.parametrize("p0,T,W,R", [(200, 17, 40, 80), (70, 24, 40, 63), (0, 33, 8, 40), (500, 1, 80, 80)])
def test_reference_equals_sdpa_with_a_banded_mask_over_a_wrapped_ring(p0, T, W, R):
    """torch SDPA in float64 over the LINEAR stream with an explicit banded mask, against the reference gathering from the ring -- whose
    other rows hold NaN: it looks at no row outside the attended span.  One start per sequence is the same thing sequence by sequence."""
    nh, nkv, B = 4, 2, 2
    g = torch.Generator().manual_seed(p0 + T)
    q = torch.randn(B, nh, T, 128, generator=g).half()
    lin_k, lin_v = torch.randn(B, nkv, p0 + T, 128, generator=g).half(), torch.randn(B, nkv, p0 + T, 128, generator=g).half()
    lo = max(0, p0 - W + 1)
    kr, vr = _ring_of(lin_k, lo, p0 + T - 1, R, float("nan")), _ring_of(lin_v, lo, p0 + T - 1, R, float("nan"))
    j, qp = torch.arange(p0 + T)[None, :], p0 + torch.arange(T)[:, None]
    mask = (j <= qp) & (j > qp - W)
    ke, ve = (t.double().repeat_interleave(nh // nkv, 1) for t in (lin_k, lin_v))
    want = torch.nn.functional.scaled_dot_product_attention(q.double(), ke, ve, attn_mask=mask)        # [B, nh, T, D]
    want = want.transpose(1, 2).reshape(B * T, nh * 128)
    got = window_attention_reference(q, kr, vr, p0, W)
    assert not torch.isnan(got).any() and float((got - want).abs().max()) < 1e-12
    assert torch.equal(window_attention_reference(q, kr, vr, [p0, p0], W), got)
    with pytest.raises(ValueError):
        window_attention_reference(q, kr, vr, p0, 0)
    if W + T - 1 > R:
        pytest.fail("the case breaks the ring rule")


HIDDEN, NH, NKV, G, MAXLEN = 512, 4, 2, 128, 256


def _module(**kw):
    qkv = WQLinear_QUICK(4, G, HIDDEN, (NH + 2 * NKV) * 128, False, "cpu")
    o = WQLinear_QUICK(4, G, HIDDEN, HIDDEN, False, "cpu")
    return QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, **kw)


def test_module_constructor(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "3")
    sig = inspect.signature(QuantAttentionFused.__init__).parameters
    assert sig["sliding_window"].default is None and sig["prefill_chunk"].default == 512
    default, m = _module(), _module(sliding_window=40, prefill_chunk=24)
    # sliding_window=None leaves the caches at max_seq_len rows
    assert default.sliding_window is None and tuple(default.k_cache.shape) == (3, NKV, MAXLEN, 128) == tuple(default.v_cache.shape)
    assert (m.sliding_window, m.prefill_chunk) == (40, 24)
    assert tuple(m.k_cache.shape) == (3, NKV, 63, 128) == tuple(m.v_cache.shape) and m.k_cache.dtype == torch.float16
    assert m.cos.shape[0] == MAXLEN == m.max_seq_len                          # max_seq_len keeps its meaning: the position bound
    assert tuple(_module(sliding_window=40).k_cache.shape) == (3, NKV, MAXLEN, 128)      # min(max_seq_len, 40 + 512 - 1)
    assert tuple(_module(sliding_window=300, prefill_chunk=1).k_cache.shape) == (3, NKV, MAXLEN, 128)
    assert tuple(_module(sliding_window=1, prefill_chunk=1).k_cache.shape) == (3, NKV, 1, 128)
    m._allocate(5, "cpu")                                                     # a batch-size change keeps the ring
    assert tuple(m.v_cache.shape) == (5, NKV, 63, 128)
    ps = _module(sliding_window=40, prefill_chunk=24, per_sequence=True)
    assert ps.pos.tolist() == [0, 0, 0] and tuple(ps.k_cache.shape) == (3, NKV, 63, 128)
    assert set(default.state_dict()) == set(m.state_dict()) == {f"{p}.{n}" for p in ("qkv_proj", "o_proj") for n in ("qweight", "qzeros", "scales")}
    for kw in (dict(sliding_window=0), dict(sliding_window=-5), dict(sliding_window=2.5), dict(prefill_chunk=0), dict(prefill_chunk=-1),
               dict(sliding_window=40, prefill_chunk=0), dict(sliding_window=40, kv_cache_dtype="fp8_e4m3")):
        with pytest.raises(ValueError):
            _module(**kw)
    with pytest.raises(ValueError, match="prefill_chunk"):
        m(torch.zeros(5, 25, HIDDEN, dtype=torch.float16))
    with pytest.raises(ValueError, match="max_seq_len"):
        m(torch.zeros(5, MAXLEN + 1, HIDDEN, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(5, 24, HIDDEN, dtype=torch.float16))
    # a ring that never wraps takes any chunk the positions allow
    with pytest.raises(RuntimeError, match="GPU"):
        _module(sliding_window=40)(torch.zeros(3, 200, HIDDEN, dtype=torch.float16))


def test_kernels_refuse_a_window_over_byte_caches():
    kb = torch.zeros(1, 2, 16, 128, dtype=torch.uint8)
    x = torch.zeros(1, 8 * 128, dtype=torch.float16)
    pos = torch.zeros(1, dtype=torch.int64)
    for cache in (kb, kb.view(torch.float8_e4m3fn)):
        with pytest.raises(ValueError, match="one-byte"):
            kernels.rope_attention(x, x, x, pos, cache, cache, x, 4, 2, 128, window=8)
        with pytest.raises(ValueError, match="one-byte"):
            kernels.rope_kv_write(x, x, x, pos, x, cache, cache, 1, 4, 2, 128, window=8)
        with pytest.raises(ValueError, match="one-byte"):
            kernels.prefill_attention(x, cache, cache, pos, x, 4, 2, 128, window=8, table_rows=64)


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2), (8, 1)])
def test_the_emulation_of_the_prefill_rounding_points_stays_inside_the_bound(nh, nkv):
    """What the GPU suite demands of the kernel it first demands of its own model of the kernel, with no GPU: the emulation of the
    windowed prefill's rounding points is within prefill_bound_win of the float64 reference on the GPU test's shapes (inputs drawn on the
    CPU by the same code), at the positions where the window starts, wraps and has lapped."""
    import test_sliding_window_gpu as GW
    for R, W, T in GW.PF_SHAPES:
        for p0 in (0, 32, 90, 500):
            for variant in ("random", "peaked"):
                q, kr, vr = GW.prefill_case(2, nh, nkv, R, W, T, p0, variant, "cpu")
                qd, Kd, Vd, vis, s, P, ref = GW.reference_parts(q, kr, vr, p0, W)
                pub = GW.rows_to_heads(window_attention_reference(q, kr, vr, p0, W), 2, T, nkv, nh // nkv)
                assert float((pub - ref).abs().max()) < 1e-12
                bound = GW.prefill_bound_win(qd, Kd, Vd, vis, s, P, ref, p0, W)
                emu = float(((GW.emulate_prefill_win(q, kr, vr, p0, W) - pub).abs() / bound).max())
                assert emu <= 1.0, (R, W, T, p0, variant, emu)


@pytest.mark.parametrize("nh,nkv", [(4, 4), (4, 2), (8, 2), (8, 1)])
def test_the_emulation_of_the_decode_rounding_points_stays_inside_the_bound(nh, nkv):
    """The same for the decode step: its rounding points (per wave and row quarter, merged as the kernel merges them) against
    decode_bound_win over the n = min(p + 1, W) rows of the window, at every position of the GPU test."""
    import test_sliding_window_gpu as GW
    B, R, W = 3, 80, 40
    cos_np, sin_np = GW._tables(GW.NP, 1e4)
    for p in GW.DEC_P:
        qkv, kr, vr, q_rot, k_rot = GW.decode_case(B, nh, nkv, R, W, p, 7 * p + nh, "cpu", cos_np, sin_np)
        kr[:, :, p % R] = k_rot
        vr[:, :, p % R] = qkv.view(B, nh + 2 * nkv, 128)[:, nh + nkv:]
        q4 = q_rot.view(B, nh, 1, 128)
        qd, Kd, Vd, vis, s, P, ref = GW.reference_parts(q4, kr, vr, p, W)
        bound = GW.decode_bound_win(qd[:, :, :, 0], Kd, Vd, s[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])
        span = torch.arange(max(0, p - W + 1), p + 1)
        emu = GW.emulate_decode_win(q_rot.view(B, nkv, nh // nkv, 128), kr[:, :, ring_slot(span, R)], vr[:, :, ring_slot(span, R)])
        ratio = float(((emu - ref[:, :, :, 0]).abs() / bound).max())
        assert ratio <= 1.0, (p, ratio)
