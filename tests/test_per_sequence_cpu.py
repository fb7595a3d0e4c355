"""Per-sequence positions, host side: the three *_seq_f16 entry points are exported and refuse what their shared siblings refuse before
any launch (null device pointers, no GPU needed); kernels.*(per_sequence=True) checks its position tensor before it calls the library;
QuantAttentionFused(per_sequence=True) keeps one position per sequence, resets single slots, validates host-side new_tokens and keeps
start_pos as an upper bound."""
import ctypes
import os
import re

import pytest
import torch

from quick_amd import QuantAttentionFused, WQLinear_QUICK, _lib, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_P, _I = ctypes.c_void_p, ctypes.c_int
INVALID, UNSUPPORTED = 1, 4
HIDDEN, NH, NKV, G, MAXLEN = 512, 4, 2, 128, 64
SEQ = ("quick_decode_rope_attention_seq_f16", "quick_rope_kv_write_seq_f16", "quick_prefill_attention_seq_f16")


def _module(**kw):
    qkv = WQLinear_QUICK(4, G, HIDDEN, (NH + 2 * NKV) * 128, False, "cpu")
    o = WQLinear_QUICK(4, G, HIDDEN, HIDDEN, False, "cpu")
    return QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, **kw)


def test_the_three_symbols_are_exported_with_their_siblings_signatures():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "quick_amd.h")).read(), flags=re.S)
    for name in SEQ:
        sibling = name.replace("_seq_f16", "_f16")
        assert name in _lib.EXPORTS and hasattr(lib, name)
        assert _lib._SIGNATURES[name] == _lib._SIGNATURES[sibling] and getattr(lib, name).argtypes == _lib._SIGNATURES[name][1]
        args = lambda n: [a.split()[-1].lstrip("*") for a in re.search(r"int %s\((.*?)\);" % n, header, re.S).group(1).split(",")]
        assert args(name) == args(sibling), name


def test_seq_entry_points_refuse_what_their_siblings_refuse_before_launching():
    """Null device pointers throughout: every call must come back with its sibling's error code (tests/test_module_cpu.py,
    test_decode_entry_points_refuse_before_launching, and tests/test_prefill_attention_cpu.py hold the siblings to the same lists)."""
    lib = _lib.load()
    pair = lambda name: (getattr(lib, name), getattr(lib, name.replace("_seq_f16", "_f16")))
    seq, shared = pair("quick_rope_kv_write_seq_f16")
    cases = [(1, 4, 8, 2, D, 64) for D in (127, 63, 130, 256)] + [(1, 4, nh, nkv, 128, 64) for nh, nkv in ((8, 3), (8, 0), (0, 2), (-8, 2))]
    cases += [(0, 4, 8, 2, 128, 64), (1, 0, 8, 2, 128, 64)]
    for args in cases:
        assert seq(*[None] * 7, *args, None) == shared(*[None] * 7, *args, None) == INVALID, args
    for args in ((65536, 1, 8, 2, 128, 64), (256, 257, 8, 2, 128, 64), (1, 65536, 8, 2, 128, 64)):
        assert seq(*[None] * 7, *args, None) == shared(*[None] * 7, *args, None) == UNSUPPORTED, args
    seq, shared = pair("quick_decode_rope_attention_seq_f16")
    for args in ((1, 8, 2, 64, 64), (1, 8, 2, 127, 64), (65536, 8, 2, 128, 64), (1, 8, 3, 128, 64), (1, 8, 0, 128, 64), (0, 8, 2, 128, 64),
                 (1, 8, 2, 128, 0)):
        assert seq(*[None] * 7, *args, 0.1, None) == shared(*[None] * 7, *args, 0.1, None) == UNSUPPORTED, args
    seq, shared = pair("quick_prefill_attention_seq_f16")
    refusals = [((0, 16, 8, 2, 128, 512), INVALID, "must be positive"), ((2, 0, 8, 2, 128, 512), INVALID, "must be positive"),
                ((2, 16, 8, 2, 128, 0), INVALID, "must be positive"), ((2, 513, 8, 2, 128, 512), INVALID, "tokens > cache_len"),
                ((2, 16, 8, 2, 64, 512), UNSUPPORTED, "head_dim must be 128"), ((2, 16, 8, 3, 128, 512), UNSUPPORTED, "multiple of n_kv_heads"),
                ((65536, 16, 8, 2, 128, 512), UNSUPPORTED, "grid dimensions"), ((2, 16, 65536, 2, 128, 512), UNSUPPORTED, "grid dimensions")]
    for shape, status, words in refusals:
        assert shared(*[None] * 5, *shape, 128 ** -0.5, None) == status
        assert seq(*[None] * 5, *shape, 128 ** -0.5, None) == status and words in _lib.last_error(), (shape, _lib.last_error())
    fake = 4096      # never dereferenced: the refusal comes first
    for hole in range(5):
        ptrs = [None if i == hole else fake for i in range(5)]
        assert seq(*ptrs, 2, 16, 8, 2, 128, 512, 128 ** -0.5, None) == INVALID and "null pointer" in _lib.last_error(), hole


def test_kernels_per_sequence_refuses_a_bad_position_tensor_before_the_library_is_called(monkeypatch):
    """Wrong dtype, wrong element count, wrong device: ValueError, and the library is not reached (its loader is made to fail)."""
    B, T, L = 3, 4, 16
    f16 = lambda *shape: torch.zeros(shape, dtype=torch.float16)
    qkv1, qkvT = f16(B, (NH + 2 * NKV) * 128), f16(B * T, (NH + 2 * NKV) * 128)
    cos, sin, kc, vc = f16(L, 128), f16(L, 128), f16(B, NKV, L, 128), f16(B, NKV, L, 128)
    q, att1, attT = f16(B, NH, T, 128), f16(B, NH * 128), f16(B * T, NH * 128)
    calls = {
        "rope_attention": lambda pos: kernels.rope_attention(qkv1, cos, sin, pos, kc, vc, att1, NH, NKV, 128, per_sequence=True),
        "rope_kv_write": lambda pos: kernels.rope_kv_write(qkvT, cos, sin, pos, q, kc, vc, T, NH, NKV, 128, per_sequence=True),
        "prefill_attention": lambda pos: kernels.prefill_attention(q, kc, vc, pos, attT, NH, NKV, 128, per_sequence=True),
    }

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "load", no_library)
    for name, call in calls.items():
        with pytest.raises(ValueError, match="int64"):
            call(torch.zeros(B, dtype=torch.int32))
        with pytest.raises(ValueError, match="int64"):
            call([0] * B)
        for n in (1, B - 1, B + 1):
            with pytest.raises(ValueError, match=f"one contiguous position per sequence \\({B}\\)"):
                call(torch.zeros(n, dtype=torch.int64))
        with pytest.raises(ValueError, match="GPU tensor"):
            call(torch.zeros(B, dtype=torch.int64))


def test_module_keeps_one_position_per_sequence_and_resets_slots(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "3")
    m = _module(per_sequence=True)
    assert m.per_sequence and m.pos.dtype == torch.int64 and m.pos.tolist() == [0, 0, 0] and m.start_pos == 0
    m._allocate(5, "cpu")                    # a batch-size change re-makes the positions with the caches
    assert m.pos.tolist() == [0] * 5 and tuple(m.k_cache.shape) == (5, NKV, MAXLEN, 128)
    m.pos.copy_(torch.tensor([7, 30, 2, 11, 30]))
    m.start_pos = 40                         # an upper bound that had grown past the positions
    m.reset(slots=[1])
    assert m.pos.tolist() == [7, 0, 2, 11, 30] and m.start_pos == 30
    m.reset(slots=(4, 0))
    assert m.pos.tolist() == [0, 0, 2, 11, 0] and m.start_pos == 11
    m.reset(slots=[])
    assert m.pos.tolist() == [0, 0, 2, 11, 0] and m.start_pos == 11
    for bad in ([5], [-1], [0, 9]):
        with pytest.raises(ValueError, match="slots are 0 .. 4"):
            m.reset(slots=bad)
    m.reset()
    assert m.pos.tolist() == [0] * 5 and m.start_pos == 0
    # the shared-position module is what it was: one position, the reference's positional constructor, no slots
    monkeypatch.delenv("AWQ_BATCH_SIZE")
    shared = _module()
    assert not shared.per_sequence and shared.pos.tolist() == [0]
    with pytest.raises(ValueError, match="per_sequence=True"):
        shared.reset(slots=[0])
    qkv, o = shared.qkv_proj, shared.o_proj
    assert QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, False, None, 10000).per_sequence is False


def test_new_tokens_is_validated_on_the_host_and_refused_without_per_sequence(monkeypatch):
    """Every refusal is a ValueError raised before the device check; a forward that gets past them ends at the GPU error, on the CPU."""
    monkeypatch.setenv("AWQ_BATCH_SIZE", "3")
    x = torch.zeros(3, 4, HIDDEN, dtype=torch.float16)
    shared = _module()
    for nt in ([4, 4, 4], torch.tensor([1, 2, 3])):
        with pytest.raises(ValueError, match="new_tokens needs per_sequence=True"):
            shared(x, new_tokens=nt)
    assert shared.start_pos == 0
    m = _module(per_sequence=True)
    for nt in ([4, 4], (1, 2, 3, 4), torch.tensor([1, 2])):
        with pytest.raises(ValueError, match="the batch has 3 sequences"):
            m(x, new_tokens=nt)
    for nt in ([5, 0, 0], [0, -1, 4], torch.tensor([4, 4, 9]), [1.5, 2, 3]):
        with pytest.raises(ValueError, match=r"whole numbers in 0 \.\. T = 4"):
            m(x, new_tokens=nt)
    assert m.start_pos == 0 and m.pos.tolist() == [0, 0, 0]
    for nt in (None, [4, 0, 2], (0, 0, 0), torch.tensor([1, 2, 3])):
        with pytest.raises(RuntimeError, match="GPU"):
            m(x, new_tokens=nt)
    assert m.start_pos == 0 and m.pos.tolist() == [0, 0, 0]


def test_start_pos_is_a_bound_and_the_overflow_message_names_the_padding(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "2")
    m = _module(per_sequence=True)
    # _new_tokens: what pos advances by on the device, what the host bound advances by
    step, advance = m._new_tokens([3, 0], 2, 5)
    assert step.dtype == torch.int64 and step.tolist() == [3, 0] and advance == 3
    assert m._new_tokens(None, 2, 5) == (None, 5)
    step, advance = m._new_tokens(torch.tensor([5, 5]), 2, 5)
    assert step.tolist() == [5, 5] and advance == 5
    # the bound, not the positions, decides: a chunk of T rows needs T rows behind the bound, whatever new_tokens says
    m.start_pos = MAXLEN - 4
    m.pos.copy_(torch.tensor([3, MAXLEN - 4]))
    x = torch.zeros(2, 5, HIDDEN, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"60 \+ 5 exceeds max_seq_len = 64.*does not roll.*padded chunk needs room for its padding"):
        m(x, new_tokens=[1, 1])
    with pytest.raises(RuntimeError, match="GPU"):
        m(x[:, :4], new_tokens=[1, 1])
    m.reset(slots=[1])                       # the long sequence leaves: the bound falls back to the largest remaining position
    assert m.start_pos == 3
    with pytest.raises(RuntimeError, match="GPU"):
        m(x, new_tokens=[1, 1])
    # the shared-position module's message is the one it had
    monkeypatch.delenv("AWQ_BATCH_SIZE")
    shared = _module()
    with pytest.raises(ValueError) as e:
        shared(torch.zeros(1, MAXLEN + 1, HIDDEN, dtype=torch.float16))
    assert "padding" not in str(e.value) and "does not roll" in str(e.value)


def test_decode_step_fused_refuses_a_position_count_that_is_neither_one_nor_the_batch():
    from quick_amd.decoder import decode_step_fused

    class Stub:                              # the check comes before anything of the model but its config is touched
        from quick_amd.decoder import CONFIGS
        cfg = CONFIGS["tiny"]
    with pytest.raises(ValueError, match=r"one per sequence \(3\), it holds 2"):
        decode_step_fused(Stub, torch.zeros(3, dtype=torch.int64), torch.zeros(2, dtype=torch.int64))
