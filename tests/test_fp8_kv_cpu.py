"""The one-byte (OCP e4m3fn) KV cache, host side: the exported symbols and their refusals with no GPU present, quantize_kv / dequantize_kv
as the restatement of the format (round trip, ties to even, saturation, underflow, NaN, scales), the module's and the synthetic decoder's
constructors, and the GPU suite's emulation of the prefill kernel's rounding points against the bound it is held to there."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from quick_amd import QuantAttentionFused, WQLinear_QUICK, _lib, kernels
from quick_amd.attention import dequantize_kv, quantize_kv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 4
F8, U8 = torch.float8_e4m3fn, torch.uint8
P16, P8 = ctypes.c_void_p(1 << 40), ctypes.c_void_p((1 << 40) + 8)      # never dereferenced: every call below is refused first


def test_symbols_are_exported_with_the_declared_signatures():
    header = open(os.path.join(ROOT, "include", "quick_amd.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    lib = _lib.load()
    assert lib.quick_amd_abi_version() == 1
    c_types = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float,
               "char*": ctypes.c_char_p, "size_t": ctypes.c_size_t}
    for name in ("quick_rope_kv_write_fp8", "quick_decode_rope_attention_fp8", "quick_decode_rope_attention_fp8_describe",
                 "quick_prefill_attention_fp8"):
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        m = re.search(r"int " + name + r"\(([^)]*)\);", flat)
        assert m, name
        declared = [c_types[a.strip().rsplit(" ", 1)[0]] for a in m.group(1).split(",")]
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and args == declared, (name, args, declared)
    for fn in (kernels.rope_kv_write, kernels.rope_attention, kernels.prefill_attention):
        sig = inspect.signature(fn).parameters
        assert sig["k_scale"].default == 1.0 and sig["v_scale"].default == 1.0 and sig["per_sequence"].default is False


def test_refusals_come_back_before_any_gpu_work():
    """Every refusal of the three launches (and the describe) with its code and a sentence; null pointers unless the pointers are the
    subject (then fake aligned addresses: the call is refused before anything could read them)."""
    lib = _lib.load()
    n7, buf = [None] * 7, ctypes.create_string_buffer(128)
    write = lambda ptrs, B, T, nh, nkv, D, L, ks=1.0, vs=1.0, seq=0: lib.quick_rope_kv_write_fp8(*ptrs, B, T, nh, nkv, D, L, ks, vs, seq, None)
    decode = lambda ptrs, B, nh, nkv, D, L, ks=1.0, vs=1.0, seq=0: lib.quick_decode_rope_attention_fp8(*ptrs, B, nh, nkv, D, L, 0.1, ks, vs, seq, None)
    prefill = lambda ptrs, B, T, nh, nkv, D, L, ks=1.0, vs=1.0, seq=0: lib.quick_prefill_attention_fp8(*ptrs, B, T, nh, nkv, D, L, 0.1, ks, vs, seq, None)

    def refused(rc, code, words):
        msg = _lib.last_error()
        assert rc == code and words in msg and "fp8" in msg, (rc, code, msg)

    for seq in (0, 1):
        # head_dim
        for D in (64, 127, 256):
            refused(write(n7, 1, 4, 8, 2, D, 64, seq=seq), UNSUPPORTED, "head_dim must be 128")
            refused(decode(n7, 1, 8, 2, D, 64, seq=seq), UNSUPPORTED, "head_dim must be 128")
            refused(prefill(n7[:5], 1, 4, 8, 2, D, 64, seq=seq), UNSUPPORTED, "head_dim must be 128")
        # n_heads % n_kv_heads, and the decode groups
        refused(write(n7, 1, 4, 8, 3, 128, 64, seq=seq), INVALID, "multiple of n_kv_heads")
        refused(decode(n7, 1, 8, 3, 128, 64, seq=seq), UNSUPPORTED, "multiple of n_kv_heads")
        refused(prefill(n7[:5], 1, 4, 8, 3, 128, 64, seq=seq), UNSUPPORTED, "multiple of n_kv_heads")
        for nh, nkv in ((3, 1), (12, 2), (16, 1), (48, 16)):
            refused(decode(n7, 1, nh, nkv, 128, 64, seq=seq), UNSUPPORTED, "1, 2, 4 or 8 query heads per KV head")
            assert lib.quick_decode_rope_attention_fp8_describe(1, nh, nkv, 128, 64, buf, len(buf)) == UNSUPPORTED
        # non-positive sizes
        for B, T, nh, nkv, L in ((0, 4, 8, 2, 64), (1, 0, 8, 2, 64), (1, 4, 0, 2, 64), (1, 4, 8, 0, 64), (1, 4, 8, 2, 0), (-1, 4, 8, 2, 64)):
            refused(write(n7, B, T, nh, nkv, 128, L, seq=seq), INVALID, "must be positive")
            refused(prefill(n7[:5], B, T, nh, nkv, 128, L, seq=seq), INVALID, "must be positive")
            if T:
                refused(decode(n7, B, nh, nkv, 128, L, seq=seq), UNSUPPORTED, "must be positive")
        refused(prefill(n7[:5], 1, 65, 8, 2, 128, 64, seq=seq), INVALID, "tokens > cache_len")
        refused(write(n7, 256, 257, 8, 2, 128, 512, seq=seq), UNSUPPORTED, "65535")
        refused(decode(n7, 65536, 8, 2, 128, 64, seq=seq), UNSUPPORTED, "65535")
        # scales
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            for ks, vs in ((bad, 1.0), (1.0, bad)):
                refused(write(n7, 1, 4, 8, 2, 128, 64, ks, vs, seq), INVALID, "finite and positive")
                refused(decode(n7, 1, 8, 2, 128, 64, ks, vs, seq), INVALID, "finite and positive")
                refused(prefill(n7[:5], 1, 4, 8, 2, 128, 64, ks, vs, seq), INVALID, "finite and positive")
        # pointers: each one null, each one misaligned (pos: 8 bytes, the others 16)
        for count, call, pos_at in ((7, lambda p: write(p, 1, 4, 8, 2, 128, 64, seq=seq), 3), (7, lambda p: decode(p, 1, 8, 2, 128, 64, seq=seq), 3),
                                    (5, lambda p: prefill(p, 1, 4, 8, 2, 128, 64, seq=seq), 3)):
            for i in range(count):
                ptrs = [P16] * count
                ptrs[i] = None
                refused(call(ptrs), INVALID, "null or misaligned pointer")
                ptrs[i] = ctypes.c_void_p((1 << 40) + 4) if i == pos_at else P8
                refused(call(ptrs), INVALID, "null or misaligned pointer")
    # the describe of the decode launch: host only
    assert lib.quick_decode_rope_attention_fp8_describe(64, 32, 8, 128, 2048, buf, len(buf)) == 0
    assert buf.value.decode() == "gqa-mfma-fp8 heads=4 gsplit=1 waves=4 set_rows=64 grid=8x64"
    assert kernels.attention_describe(16, 64, 8, 128, 4096, kv_cache_dtype="fp8_e4m3").startswith("gqa-mfma-fp8 heads=8 gsplit=1")
    assert lib.quick_decode_rope_attention_fp8_describe(1, 8, 2, 128, 64, None, 0) == INVALID
    assert kernels.attention_describe(16, 64, 8, 128, 4096, kv_cache_dtype="fp16").startswith("gqa-mfma heads=4 gsplit=2")
    for bad in ("fp8", "fp8_e5m2", None):
        with pytest.raises(ValueError, match="kv_cache_dtype"):
            kernels.attention_describe(16, 64, 8, 128, 4096, kv_cache_dtype=bad)


def _codes(keep_nan=False):
    b = torch.arange(256, dtype=torch.int16).to(U8)
    return b if keep_nan else b[(b & 0x7F) != 0x7F]


def test_round_trip_of_all_254_codes():
    b = _codes()
    assert b.numel() == 254
    v = dequantize_kv(b, 1.0)
    assert v.dtype == torch.float32 and float(v.max()) == 448.0 and float(v.min()) == -448.0
    assert torch.equal(quantize_kv(v, 1.0).view(U8), b)                        # -0 (0x80) included
    assert torch.equal(quantize_kv(v.half(), 1.0).view(U8), b)                 # every code is an fp16 value
    assert torch.equal(dequantize_kv(b.view(F8), 1.0), v)
    # the values are OCP e4m3fn's: bias 7, subnormals 2^-9 .. 7 * 2^-9, no infinities
    e, m = ((b & 0x78) >> 3).double(), (b & 7).double()
    mag = torch.where(e == 0, m * 2.0 ** -9, (1 + m / 8) * torch.exp2(e - 7))
    assert torch.equal(v.double(), torch.where((b & 0x80) != 0, -mag, mag))


def test_rounding_saturation_underflow_and_nan():
    pos = _codes()[:0x7F]                                                       # 0x00 .. 0x7E
    v = dequantize_kv(pos, 1.0).double()
    mid = ((v[:-1] + v[1:]) / 2).float()
    assert torch.equal(mid.double(), (v[:-1] + v[1:]) / 2)
    even = torch.where(pos[:-1] % 2 == 0, pos[:-1], pos[1:])
    assert torch.equal(quantize_kv(mid, 1.0).view(U8), even)                   # exact midpoints go to the even code
    assert torch.equal(quantize_kv(-mid, 1.0).view(U8), even | 0x80)
    up, down = torch.nextafter(mid, torch.tensor(1e9)), torch.nextafter(mid, torch.tensor(-1e9))
    assert torch.equal(quantize_kv(up, 1.0).view(U8), pos[1:]) and torch.equal(quantize_kv(down, 1.0).view(U8), pos[:-1])
    sat = torch.tensor([448.0001, 65504.0, 464.0, 480.0, float("inf")])
    assert quantize_kv(sat, 1.0).view(U8).tolist() == [0x7E] * 5 and quantize_kv(-sat, 1.0).view(U8).tolist() == [0xFE] * 5
    assert quantize_kv(torch.tensor([65504.0, -65504.0]).half(), 1.0).view(U8).tolist() == [0x7E, 0xFE]
    tiny = torch.tensor([2.0 ** -10, 2.0 ** -11, 1e-30, 0.0])                  # at and below the smallest subnormal's midpoint
    assert quantize_kv(tiny, 1.0).view(U8).tolist() == [0, 0, 0, 0] and quantize_kv(-tiny, 1.0).view(U8).tolist() == [0x80] * 4
    assert quantize_kv(torch.nextafter(tiny[:1], torch.tensor(1.0)), 1.0).view(U8).tolist() == [1]
    nan = quantize_kv(torch.tensor([float("nan")]), 1.0).view(U8)
    assert int(nan[0]) & 0x7F == 0x7F
    assert torch.isnan(dequantize_kv(torch.tensor([0x7F, 0xFF], dtype=U8), 0.5)).all()


@pytest.mark.parametrize("scale", [2.0 ** -3, 0.37])
def test_scales_reproduce_the_fp32_expression_of_the_contract(scale):
    """byte = rne_e4m3(clamp(float(h) * inv, -448, 448)) with inv = 1.0f / scale in fp32, on every finite fp16 value h: the multiply in
    numpy float32, the rounding by a nearest-code search in float64 with ties to the even code; value = float(byte) * scale in fp32."""
    h = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    h = h[torch.isfinite(h)]
    got = quantize_kv(h, scale).view(U8)
    inv = np.float32(1.0) / np.float32(scale)
    y = np.clip(h.numpy().astype(np.float32) * inv, np.float32(-448), np.float32(448)).astype(np.float64)
    grid = dequantize_kv(_codes()[:0x7F], 1.0).double().numpy()               # the non-negative codes, ascending
    a = np.abs(y)
    hi = np.clip(np.searchsorted(grid, a), 1, len(grid) - 1)
    lo = hi - 1
    dl, dh = a - grid[lo], grid[hi] - a
    code = np.where(dl < dh, lo, np.where(dh < dl, hi, np.where(lo % 2 == 0, lo, hi)))
    want = code.astype(np.uint8) | (np.signbit(y).astype(np.uint8) << 7)
    assert np.array_equal(got.numpy(), want)
    assert torch.equal(dequantize_kv(got, scale), torch.from_numpy(grid[code] * np.where(np.signbit(y), -1.0, 1.0)).float() * np.float32(scale))
    with pytest.raises(ValueError):
        quantize_kv(h, 0.0)
    with pytest.raises(ValueError):
        dequantize_kv(got, float("nan"))


HIDDEN, NH, NKV, G, MAXLEN = 512, 4, 2, 128, 64


def _module(**kw):
    qkv = WQLinear_QUICK(4, G, HIDDEN, (NH + 2 * NKV) * 128, False, "cpu")
    o = WQLinear_QUICK(4, G, HIDDEN, HIDDEN, False, "cpu")
    return QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, **kw)


def test_module_constructor(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "3")
    default, m = _module(), _module(kv_cache_dtype="fp8_e4m3", k_scale=0.25, v_scale=0.37)
    nbytes = lambda mod: sum(c.numel() * c.element_size() for c in (mod.k_cache, mod.v_cache))
    assert m.k_cache.dtype == F8 == m.v_cache.dtype and tuple(m.k_cache.shape) == (3, NKV, MAXLEN, 128)
    assert 2 * nbytes(m) == nbytes(default)
    assert (m.kv_cache_dtype, m.k_scale, m.v_scale) == ("fp8_e4m3", 0.25, 0.37)
    m._allocate(5, "cpu")                                                       # a batch-size change keeps the byte caches
    assert m.k_cache.dtype == F8 and tuple(m.v_cache.shape) == (5, NKV, MAXLEN, 128)
    assert m.half().k_cache.dtype == F8 and m.cos.dtype == torch.float16       # (a dtype cast of the module leaves the bytes bytes)
    # the default module is what it was
    assert default.k_cache.dtype == torch.float16 == default.v_cache.dtype and (default.kv_cache_dtype, default.k_scale, default.v_scale) == ("fp16", 1.0, 1.0)
    assert set(default.state_dict()) == set(m.state_dict()) == {f"{p}.{n}" for p in ("qkv_proj", "o_proj") for n in ("qweight", "qzeros", "scales")}
    assert default.start_pos == 0 and default.pos.tolist() == [0] and default.per_sequence is False
    for kw in (dict(kv_cache_dtype="fp8"), dict(kv_cache_dtype="fp8_e5m2"), dict(kv_cache_dtype="int8"), dict(kv_cache_dtype=None),
               dict(kv_cache_dtype="fp8_e4m3", k_scale=0.0), dict(kv_cache_dtype="fp8_e4m3", v_scale=-1.0),
               dict(kv_cache_dtype="fp8_e4m3", k_scale=float("inf")), dict(kv_cache_dtype="fp8_e4m3", v_scale=float("nan")), dict(k_scale=0.0)):
        with pytest.raises(ValueError):
            _module(**kw)
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(5, 1, HIDDEN, dtype=torch.float16))
    with pytest.raises(ValueError, match="max_seq_len"):
        m(torch.zeros(5, MAXLEN + 1, HIDDEN, dtype=torch.float16))


def test_synthetic_decoder_takes_the_cache_dtype():
    from quick_amd.decoder import DecoderConfig, SyntheticDecoder
    sig = inspect.signature(SyntheticDecoder.__init__).parameters
    assert sig["kv_cache_dtype"].default == "fp16" and sig["k_scale"].default == 1.0 and sig["v_scale"].default == 1.0
    cfg = DecoderConfig("tiny", 256, 1, 2, 1, 512)
    with pytest.raises(ValueError):
        SyntheticDecoder(cfg, 1, 16, "cpu", kv_cache_dtype="fp4")
    with pytest.raises(ValueError):
        SyntheticDecoder(cfg, 1, 16, "cpu", kv_cache_dtype="fp8_e4m3", k_scale=0.0)


def test_kernels_dispatch_on_the_cache_dtype_and_refuse_mixed_or_cpu_caches():
    kb, kh = torch.zeros(1, 2, 16, 128, dtype=U8), torch.zeros(1, 2, 16, 128, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="one kind"):
        kernels._byte_caches(kb, kh)
    with pytest.raises(RuntimeError, match="GPU"):
        kernels._byte_caches(kb.view(F8), kb)
    assert kernels._byte_caches(kh, kh) is False


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2), (8, 1)])
def test_the_emulation_of_the_prefill_rounding_points_stays_inside_the_bound(nh, nkv):
    """What the GPU suite demands of the kernel it first demands of its own model of the kernel, here, with no GPU: the float64 emulation
    of the fp8 prefill's rounding points is within _prefill_bound (applied to the dequantised cache) of the float64 reference on every
    case of the GPU test -- its head pairs, the four DENSE (pos0, T) cases, both variants, its scale pairs -- with the inputs generated on
    the CPU by the same code (another generator than the GPU's, so other draws of the same distributions).  The bound does not exclude
    the reference's own arithmetic."""
    import test_fp8_kv_gpu as G8
    assert [(nh, nkv)] and (nh, nkv) in G8.PF.HEADS
    for i, (p0, T) in enumerate(G8.PF.DENSE):
        for variant in ("random", "peaked"):
            ks, vs = G8.SCALES[i % 2]
            q, kb, vb = G8._prefill_case(2, nh, nkv, p0, T, variant, ks, vs, "cpu")
            ref, bound = G8.prefill_reference_and_bound(q, kb, vb, p0, ks, vs)
            emu = float(((G8.emulate_fp8_prefill(q, kb, vb, p0, ks, vs) - ref).abs() / bound).max())
            assert emu <= 1.0, (p0, T, variant, emu)
