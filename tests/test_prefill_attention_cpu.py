"""quick_prefill_attention_f16 / quick_prefill_attention_describe, host side: the exports, their signatures, and every refusal of
include/quick_amd.h answered before any GPU work (null device pointers, no GPU needed)."""
import ctypes
import os
import re

import pytest

from quick_amd import _lib, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I, _Z = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
INVALID, UNSUPPORTED = 1, 4

# (batch, tokens, n_heads, n_kv_heads, head_dim, cache_len), status, words of the sentence
REFUSALS = [
    ((0, 16, 8, 2, 128, 512), INVALID, "must be positive"),
    ((2, 0, 8, 2, 128, 512), INVALID, "must be positive"),
    ((2, -1, 8, 2, 128, 512), INVALID, "must be positive"),
    ((2, 16, 0, 2, 128, 512), INVALID, "must be positive"),
    ((2, 16, 8, 0, 128, 512), INVALID, "must be positive"),
    ((2, 16, 8, 2, 128, 0), INVALID, "must be positive"),
    ((2, 513, 8, 2, 128, 512), INVALID, "tokens > cache_len"),
    ((2, 16, 8, 2, 64, 512), UNSUPPORTED, "head_dim must be 128"),
    ((2, 16, 8, 2, 256, 512), UNSUPPORTED, "head_dim must be 128"),
    ((2, 16, 8, 3, 128, 512), UNSUPPORTED, "multiple of n_kv_heads"),
    ((65536, 16, 8, 2, 128, 512), UNSUPPORTED, "grid dimensions"),
    ((2, 16, 65536, 2, 128, 512), UNSUPPORTED, "grid dimensions"),
]


def test_both_symbols_are_exported_with_the_declared_signatures():
    assert _lib._SIGNATURES["quick_prefill_attention_f16"] == (_I, [_P] * 5 + [_I] * 6 + [ctypes.c_float, _P])
    assert _lib._SIGNATURES["quick_prefill_attention_describe"] == (_I, [_I] * 6 + [ctypes.c_char_p, _Z])
    lib = _lib.load()
    for name in ("quick_prefill_attention_f16", "quick_prefill_attention_describe"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "quick_amd.h")).read(), flags=re.S)
    launch = re.search(r"int quick_prefill_attention_f16\((.*?)\);", header, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in launch.split(",")] == ["q", "k_cache", "v_cache", "pos0", "out", "batch", "tokens", "n_heads",
                                                                      "n_kv_heads", "head_dim", "cache_len", "scale", "hip_stream"]
    describe = re.search(r"int quick_prefill_attention_describe\((.*?)\);", header, re.S).group(1)
    assert [a.split()[-1].lstrip("*") for a in describe.split(",")] == ["batch", "tokens", "n_heads", "n_kv_heads", "head_dim", "cache_len",
                                                                        "text", "text_bytes"]


@pytest.mark.parametrize("shape,status,words", REFUSALS)
def test_launch_and_describe_answer_every_refusal_before_any_gpu_work(shape, status, words):
    lib = _lib.load()
    rc = lib.quick_prefill_attention_f16(None, None, None, None, None, *shape, 128 ** -0.5, None)
    assert rc == status and words in _lib.last_error(), (rc, _lib.last_error())
    buf = ctypes.create_string_buffer(128)
    rc = lib.quick_prefill_attention_describe(*shape, buf, len(buf))
    assert rc == status and words in _lib.last_error(), (rc, _lib.last_error())
    with pytest.raises(ValueError if status == INVALID else NotImplementedError, match=words):
        kernels.prefill_attention_describe(*shape)


def test_a_null_pointer_is_refused_for_a_good_shape():
    lib = _lib.load()
    fake = 4096      # never dereferenced: the refusal comes first
    for hole in range(5):
        ptrs = [None if i == hole else fake for i in range(5)]
        rc = lib.quick_prefill_attention_f16(*ptrs, 2, 16, 8, 2, 128, 512, 128 ** -0.5, None)
        assert rc == INVALID and "null pointer" in _lib.last_error(), (hole, rc)
    assert lib.quick_prefill_attention_describe(2, 16, 8, 2, 128, 512, None, 0) == INVALID


@pytest.mark.parametrize("shape,grid", [((1, 1, 4, 4, 128, 512), "1x4x1"), ((3, 130, 8, 2, 128, 512), "3x8x3"), ((64, 128, 32, 8, 128, 4096), "2x32x64"),
                                        ((1, 512, 64, 8, 128, 512), "8x64x1")])
def test_describe_leads_with_its_kernel_word(shape, grid):
    text = kernels.prefill_attention_describe(*shape)
    assert text.startswith("prefill-mfma ") and text == f"prefill-mfma q_rows=64 kv_rows=32 waves=4 grid={grid}"
