"""The paged KV cache, host side: the exported symbols and their refusals with no GPU present (in the order of the header's table), the
describe words, paged_slot / gather_pages / scatter_pages on a scrambled table, the PageAllocator, and the bookkeeping of
QuantAttentionFused(page_size=..., num_pages=...) -- reserve, reset, free_pages, the bounds, no allocation while capturing -- with the
launches and the projections replaced by recorders."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from quick_amd import QuantAttentionFused, WQLinear_QUICK, _lib, kernels
from quick_amd.attention import PAGE_SIZES, PageAllocator, gather_pages, paged_slot, scatter_pages

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = 1, 4
P16 = ctypes.c_void_p(1 << 40)      # never dereferenced: every call below is refused first
NAMES = ("quick_rope_kv_write_paged_f16", "quick_decode_rope_attention_paged_f16", "quick_prefill_attention_paged_f16",
         "quick_attention_paged_describe")


def test_symbols_are_exported_with_the_declared_signatures():
    header = open(os.path.join(ROOT, "include", "quick_amd.h")).read()
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", header, flags=re.S))
    lib = _lib.load()
    assert lib.quick_amd_abi_version() == 1 and "#define QUICK_AMD_ABI_VERSION 1" in flat
    c_types = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "float": ctypes.c_float,
               "char*": ctypes.c_char_p, "size_t": ctypes.c_size_t}
    for name in NAMES:
        assert name in _lib.EXPORTS and hasattr(lib, name), name
        m = re.search(r"int " + name + r"\(([^)]*)\);", flat)
        assert m, name
        declared = [c_types[a.strip().rsplit(" ", 1)[0]] for a in m.group(1).split(",")]
        res, args = _lib._SIGNATURES[name]
        assert res is ctypes.c_int and args == declared, (name, args, declared)
        names = [a.strip().rsplit(" ", 1)[1] for a in m.group(1).split(",")]
        for i, want in enumerate(("num_pages", "page_size", "max_pages", "table_rows")):
            assert names[names.index("head_dim") + 1 + i] == want, (name, names)
        assert "ring_rows" not in names and "window" not in names
    for fn in (kernels.rope_kv_write, kernels.rope_attention, kernels.prefill_attention):
        sig = inspect.signature(fn).parameters
        assert sig["block_table"].default is None and sig["page_size"].default is None and sig["table_rows"].default is None
    assert PAGE_SIZES == (32, 64, 128, 256)


def _calls(lib):
    buf = ctypes.create_string_buffer(160)
    # (B, T, nh, nkv, D, N, P, MP, NP): batch, tokens, heads, KV heads, head_dim, num_pages, page_size, max_pages, table_rows
    write = lambda ptrs, B, T, nh, nkv, D, N, P, MP, NP, seq=0: lib.quick_rope_kv_write_paged_f16(*ptrs, B, T, nh, nkv, D, N, P, MP, NP, seq, None)
    decode = lambda ptrs, B, nh, nkv, D, N, P, MP, NP, seq=0: lib.quick_decode_rope_attention_paged_f16(*ptrs, B, nh, nkv, D, N, P, MP, NP, 0.1, seq, None)
    prefill = lambda ptrs, B, T, nh, nkv, D, N, P, MP, NP, seq=0: lib.quick_prefill_attention_paged_f16(*ptrs, B, T, nh, nkv, D, N, P, MP, NP, 0.1, seq, None)
    describe = lambda B, T, nh, nkv, D, N, P, MP, NP: lib.quick_attention_paged_describe(B, T, nh, nkv, D, N, P, MP, NP, buf, len(buf))
    return write, decode, prefill, describe


def test_refusals_come_back_before_any_gpu_work():
    """Every refusal of the header's table with its code and a sentence, in its order; null pointers unless the pointers are the subject
    (then fake addresses: the call is refused before anything could read them)."""
    lib = _lib.load()
    write, decode, prefill, describe = _calls(lib)
    n8 = [None] * 8

    def refused(rc, code, words):
        msg = _lib.last_error()
        assert rc == code and msg and words in msg and "paged" in msg, (rc, code, msg)

    for seq in (0, 1):
        # a size <= 0
        good = dict(B=1, T=4, nh=8, nkv=2, N=24, P=64, MP=8, NP=512)
        for key in good:
            for bad in (0, -1):
                a = dict(good, **{key: bad})
                refused(write(n8, a["B"], a["T"], a["nh"], a["nkv"], 128, a["N"], a["P"], a["MP"], a["NP"], seq), INVALID, "must be positive")
                refused(prefill(n8[:6], a["B"], a["T"], a["nh"], a["nkv"], 128, a["N"], a["P"], a["MP"], a["NP"], seq), INVALID, "must be positive")
                assert describe(a["B"], a["T"], a["nh"], a["nkv"], 128, a["N"], a["P"], a["MP"], a["NP"]) == INVALID
                if key != "T":
                    refused(decode(n8, a["B"], a["nh"], a["nkv"], 128, a["N"], a["P"], a["MP"], a["NP"], seq), INVALID, "must be positive")
        # a page size outside the set
        for P in (1, 16, 48, 96, 512, 65):
            refused(write(n8, 1, 4, 8, 2, 128, 24, P, 8, 512, seq), INVALID, "page_size must be 32, 64, 128 or 256")
            refused(decode(n8, 1, 8, 2, 128, 24, P, 8, 512, seq), INVALID, "page_size must be 32, 64, 128 or 256")
            refused(prefill(n8[:6], 1, 4, 8, 2, 128, 24, P, 8, 512, seq), INVALID, "page_size must be 32, 64, 128 or 256")
            assert describe(1, 4, 8, 2, 128, 24, P, 8, 512) == INVALID
        for P in PAGE_SIZES:                                      # ... and every size of the set passes up to the pointers
            refused(write(n8, 1, 4, 8, 2, 128, 24, P, 8, 512, seq), INVALID, "null pointer")
            refused(decode(n8, 1, 8, 2, 128, 24, P, 8, 512, seq), INVALID, "null pointer")
            refused(prefill(n8[:6], 1, 4, 8, 2, 128, 24, P, 8, 512, seq), INVALID, "null pointer")
        # tokens > table_rows, then max_pages * page_size < tokens (equality passes)
        refused(write(n8, 1, 33, 8, 2, 128, 24, 32, 8, 32, seq), INVALID, "tokens > table_rows")
        refused(prefill(n8[:6], 1, 33, 8, 2, 128, 24, 32, 8, 32, seq), INVALID, "tokens > table_rows")
        refused(write(n8, 1, 65, 8, 2, 128, 24, 32, 2, 512, seq), INVALID, "max_pages * page_size < tokens")
        refused(prefill(n8[:6], 1, 65, 8, 2, 128, 24, 32, 2, 512, seq), INVALID, "max_pages * page_size < tokens")
        refused(prefill(n8[:6], 1, 64, 8, 2, 128, 24, 32, 2, 512, seq), INVALID, "null pointer")
        refused(write(n8, 1, 65, 8, 2, 128, 24, 32, 2, 64, seq), INVALID, "tokens > table_rows")        # (the order of the two)
        # head_dim, n_heads % n_kv_heads, the decode groups, the grid limits
        for D in (64, 127, 256):
            refused(write(n8, 1, 4, 8, 2, D, 24, 64, 8, 512, seq), UNSUPPORTED, "head_dim must be 128")
            refused(decode(n8, 1, 8, 2, D, 24, 64, 8, 512, seq), UNSUPPORTED, "head_dim must be 128")
            refused(prefill(n8[:6], 1, 4, 8, 2, D, 24, 64, 8, 512, seq), UNSUPPORTED, "head_dim must be 128")
        refused(write(n8, 1, 4, 8, 3, 128, 24, 64, 8, 512, seq), UNSUPPORTED, "multiple of n_kv_heads")
        refused(decode(n8, 1, 8, 3, 128, 24, 64, 8, 512, seq), UNSUPPORTED, "multiple of n_kv_heads")
        refused(prefill(n8[:6], 1, 4, 8, 3, 128, 24, 64, 8, 512, seq), UNSUPPORTED, "multiple of n_kv_heads")
        for nh, nkv in ((3, 1), (12, 2), (16, 1), (48, 16)):
            refused(decode(n8, 1, nh, nkv, 128, 24, 64, 8, 512, seq), UNSUPPORTED, "1, 2, 4 or 8 query heads per KV head")
            assert describe(1, 1, nh, nkv, 128, 24, 64, 8, 512) == UNSUPPORTED
            refused(prefill(n8[:6], 1, 4, nh, nkv, 128, 24, 64, 8, 512, seq), INVALID, "null pointer")     # (the prefill serves any group)
        refused(write(n8, 256, 257, 8, 2, 128, 24, 64, 8, 1024, seq), UNSUPPORTED, "65535")
        refused(decode(n8, 65536, 8, 2, 128, 24, 64, 8, 512, seq), UNSUPPORTED, "65535")
        refused(prefill(n8[:6], 65536, 4, 8, 2, 128, 24, 64, 8, 512, seq), UNSUPPORTED, "65535")
        # pointers: each one null
        for count, call in ((8, lambda p: write(p, 1, 4, 8, 2, 128, 24, 64, 8, 512, seq)), (8, lambda p: decode(p, 1, 8, 2, 128, 24, 64, 8, 512, seq)),
                            (6, lambda p: prefill(p, 1, 4, 8, 2, 128, 24, 64, 8, 512, seq))):
            for i in range(count):
                ptrs = [P16] * count
                ptrs[i] = None
                refused(call(ptrs), INVALID, "null pointer")
    # the order of the table: an argument error is answered before an unsupported shape, an unsupported shape before the pointers
    refused(prefill(n8[:6], 1, 4, 8, 2, 64, 24, 48, 8, 512), INVALID, "page_size must be")
    refused(prefill(n8[:6], 1, 65, 8, 3, 128, 24, 32, 2, 512), INVALID, "max_pages * page_size < tokens")
    refused(decode([P16] * 8, 1, 12, 2, 128, 24, 64, 8, 512), UNSUPPORTED, "1, 2, 4 or 8")


def test_describe_words():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(160)
    assert lib.quick_attention_paged_describe(16, 1, 32, 8, 128, 1000, 64, 64, 4096, buf, len(buf)) == 0
    assert buf.value.decode() == "decode-paged-mfma heads=4 waves=4 set_rows=64 page_size=64 max_pages=64 grid=8x16"
    assert lib.quick_attention_paged_describe(16, 128, 32, 8, 128, 1000, 64, 64, 4096, buf, len(buf)) == 0
    assert buf.value.decode() == "prefill-paged-mfma q_rows=64 kv_rows=32 waves=4 page_size=64 max_pages=64 grid=2x32x16"
    assert kernels.paged_attention_describe(1, 1, 32, 32, 128, 24, 256, 16, 4096).startswith("decode-paged-mfma heads=1 ")
    assert kernels.paged_attention_describe(1, 512, 32, 32, 128, 24, 32, 128, 4096).startswith("prefill-paged-mfma ")
    assert lib.quick_attention_paged_describe(1, 1, 8, 2, 128, 24, 64, 8, 512, None, 0) == INVALID
    with pytest.raises(ValueError, match="page_size must be"):
        kernels.paged_attention_describe(1, 1, 32, 8, 128, 24, 48, 8, 512)
    with pytest.raises(NotImplementedError, match="head_dim"):
        kernels.paged_attention_describe(1, 1, 32, 8, 64, 24, 64, 8, 512)


@pytest.mark.parametrize("P", [32, 64])
def test_paged_slot_gather_and_scatter_round_trip_on_a_scrambled_table(P):
    g = torch.Generator().manual_seed(P)
    nkv, N, length = 2, 24, 3 * P + 7
    table = torch.full((8,), -1, dtype=torch.int32)
    table[:4] = torch.tensor([19, 3, 22, 0], dtype=torch.int32)                      # four needed columns, -1 behind them
    assert paged_slot(0, table, P) == (19, 0) and paged_slot(P - 1, table, P) == (19, P - 1)
    assert paged_slot(P, table, P) == (3, 0) and paged_slot(3 * P + 6, table, P) == (0, 6)
    page, row = paged_slot(torch.tensor([0, P - 1, P, 2 * P + 5]), table, P)
    assert page.tolist() == [19, 19, 3, 22] and row.tolist() == [0, P - 1, 0, 5]
    with pytest.raises(ValueError):
        paged_slot(0, table, 48)
    lin = torch.randn(nkv, length, 128, generator=g).half()
    pool = torch.full((N, nkv, P, 128), float("nan"), dtype=torch.float16)
    assert scatter_pages(pool, table, lin) is pool
    assert torch.equal(gather_pages(pool, table, length), lin)
    assert torch.equal(gather_pages(pool, table, P + 1), lin[:, :P + 1])
    for pos in (0, P - 1, P, 3 * P + 6):                                             # row by row: the mapping, not only its inverse
        pg, r = paged_slot(pos, table, P)
        assert torch.equal(pool[pg, :, r], lin[:, pos])
    written = torch.zeros(N, P, dtype=torch.bool)
    for pos in range(length):
        written[paged_slot(pos, table, P)] = True
    rows = pool.transpose(1, 2)                                                      # [N, P, nkv, D]
    assert bool(torch.isnan(rows[~written]).all()) and not torch.isnan(rows[written]).any()   # nothing else was touched


def test_page_allocator():
    a = PageAllocator(6)
    assert a.free == 6 and a.num_pages == 6
    first = a.take(4)
    assert len(set(first)) == 4 and all(0 <= p < 6 for p in first) and a.free == 2
    with pytest.raises(RuntimeError, match="2 of 6 are free, 3 were asked for"):
        a.take(3)
    assert a.free == 2                                           # all or nothing: the failed take changed nothing
    rest = a.take(2)
    assert a.free == 0 and sorted(first + rest) == list(range(6))
    assert a.take(0) == [] and a.free == 0
    a.give(first[1:3])
    assert a.free == 2
    again = a.take(2)
    assert sorted(again) == sorted(first[1:3]) and a.free == 0   # given back and reused
    for bad in ([first[0], first[0]], [6], [-1]):
        with pytest.raises(ValueError):
            a.give(bad)
    a.give([first[0]])
    with pytest.raises(ValueError):
        a.give([first[0]])                                       # free already
    assert a.free == 1
    for bad in (0, -3, 2.5):
        with pytest.raises(ValueError):
            PageAllocator(bad)


HIDDEN, NH, NKV, G, MAXLEN = 512, 4, 2, 128, 256


def _module(**kw):
    qkv = WQLinear_QUICK(4, G, HIDDEN, (NH + 2 * NKV) * 128, False, "cpu")
    o = WQLinear_QUICK(4, G, HIDDEN, HIDDEN, False, "cpu")
    return QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, **kw)


def test_module_constructor(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "3")
    sig = inspect.signature(QuantAttentionFused.__init__).parameters
    assert sig["page_size"].default is None and sig["num_pages"].default is None
    default = _module()
    assert default.page_size is None and tuple(default.k_cache.shape) == (3, NKV, MAXLEN, 128) and not hasattr(default, "block_table")
    for kw in (dict(page_size=32, num_pages=8, sliding_window=40), dict(page_size=32, num_pages=8, kv_cache_dtype="fp8_e4m3"),
               dict(page_size=48, num_pages=8), dict(page_size=16, num_pages=8), dict(page_size=32), dict(page_size=32, num_pages=0),
               dict(num_pages=8)):
        with pytest.raises(ValueError):
            _module(**kw)
    for P in PAGE_SIZES:
        m = _module(page_size=P, num_pages=11)
        assert tuple(m.k_pool.shape) == (11, NKV, P, 128) == tuple(m.v_pool.shape) and m.k_pool.dtype == torch.float16
        assert m.block_table.dtype == torch.int32 and tuple(m.block_table.shape) == (3, -(-MAXLEN // P))
        assert bool((m.block_table == -1).all()) and m.free_pages == 11 and m.cos.shape[0] == MAXLEN
    assert set(m.state_dict()) == set(default.state_dict())
    with pytest.raises(ValueError, match="paged"):
        default.reserve(10)
    with pytest.raises(ValueError, match="paged"):
        default.free_pages


class _Hidden:
    """What forward asks of hidden_states before the (replaced) projection takes it."""
    is_cuda = True

    def __init__(self, B, T):
        self.shape = (B, T, HIDDEN)

    def reshape(self, *shape):
        return self

    def contiguous(self):
        return self


class _DeviceTensor(torch.Tensor):
    """new_tokens as a device tensor, with no device: forward must not look at its values before the launches."""
    is_cuda = True


def _recording(monkeypatch, calls):
    def proj(self, x):
        rows = x.shape[0] * x.shape[1] if isinstance(x, _Hidden) else x.shape[0]
        return torch.zeros(rows, self.out_features, dtype=torch.float16)
    monkeypatch.setattr(WQLinear_QUICK, "forward", proj)
    for name in ("rope_attention", "rope_kv_write", "prefill_attention"):
        monkeypatch.setattr(kernels, name, (lambda name: lambda *a, **kw: calls.append((name, dict(kw))))(name))


def _held(m):
    return [int((row >= 0).sum()) for row in m.block_table]


def test_module_bookkeeping_over_a_sequence_of_steps(monkeypatch):
    """per_sequence, P = 32, 12 pages: list new_tokens give exact bounds, a device tensor (here a stand-in that says it is one; its
    values are never read) gives + T, reserve ahead, all or nothing, reset of one slot, reuse of its pages."""
    monkeypatch.setenv("AWQ_BATCH_SIZE", "2")
    calls = []
    _recording(monkeypatch, calls)
    m = _module(page_size=32, num_pages=12, per_sequence=True)
    table0 = m.block_table
    assert m.free_pages == 12 and _held(m) == [0, 0]
    m(_Hidden(2, 40), new_tokens=[40, 33])                       # 2 + 2 pages
    assert [c[0] for c in calls] == ["rope_kv_write", "prefill_attention"]
    for _, kw in calls:
        assert kw["block_table"] is m.block_table and kw["page_size"] == 32 and kw["table_rows"] == MAXLEN and kw["per_sequence"] is True
        assert "window" not in kw and "k_scale" not in kw
    assert m._len_bound == [40, 33] and _held(m) == [2, 2] and m.free_pages == 8
    m(_Hidden(2, 24), new_tokens=[24, 0])                        # exactly 64: still two pages; the idle slot takes nothing
    assert m._len_bound == [64, 33] and _held(m) == [2, 2] and m.free_pages == 8
    calls.clear()
    m(_Hidden(2, 1), new_tokens=[1, 1])                          # position 64: a third page for sequence 0
    assert [c[0] for c in calls] == ["rope_attention"] and calls[0][1]["block_table"] is m.block_table
    assert m._len_bound == [65, 34] and _held(m) == [3, 2] and m.free_pages == 7
    m(_Hidden(2, 9), new_tokens=torch.tensor([2, 9]).as_subclass(_DeviceTensor))     # a device tensor is not read: + T for both
    assert m._len_bound == [74, 43] and _held(m) == [3, 2] and m.free_pages == 7 and m.pos.tolist() == [67, 43]
    m(_Hidden(2, 8))                                             # no counts: + T for every sequence
    assert m._len_bound == [82, 51] and _held(m) == [3, 2] and m.free_pages == 7
    m.reserve([100, 51])                                         # ahead of time: one more page for sequence 0 only
    assert _held(m) == [4, 2] and m.free_pages == 6 and m._len_bound == [82, 51]
    m.reserve(60)                                                # never gives pages back
    assert _held(m) == [4, 2] and m.free_pages == 6
    pages = [m.block_table[b][:n].tolist() for b, n in enumerate(_held(m))]
    assert len(set(pages[0] + pages[1])) == 6                    # no page twice
    for bad in ([1], [1, 2, 3], [MAXLEN + 1, 0], [-1, 0]):
        with pytest.raises(ValueError):
            m.reserve(bad)
    # all or nothing: 2 * 8 pages are not there; nothing changes
    before = m.block_table.clone()
    with pytest.raises(RuntimeError, match="6 of 12 are free, 10 were asked for"):
        m.reserve([MAXLEN, MAXLEN])
    assert torch.equal(m.block_table, before) and m.free_pages == 6
    with pytest.raises(RuntimeError, match="pool is exhausted"):
        m(_Hidden(2, 150))
    assert torch.equal(m.block_table, before) and m.free_pages == 6 and m._len_bound == [82, 51] and m.pos.tolist() == [75, 51]
    # one slot ends: its pages go back, its row is -1 again, the other sequence keeps its own
    m.reset(slots=[1])
    assert _held(m) == [4, 0] and m.free_pages == 8 and bool((m.block_table[1] == -1).all())
    assert m._len_bound == [75, 0]                               # (reset reads the positions: the other slot's bound is exact again)
    assert m.block_table[0][:4].tolist() == pages[0]
    m(_Hidden(2, 33), new_tokens=[0, 33])                        # a new request in the freed slot reuses the freed pages
    assert _held(m) == [4, 2] and m.free_pages == 6 and set(m.block_table[1][:2].tolist()) == set(pages[1])
    assert m.block_table is table0                               # updated in place, at the same address, all along
    m.reset()
    assert m.free_pages == 12 and bool((m.block_table == -1).all()) and m._len_bound == [0, 0] and m.block_table is table0


def test_module_allocates_nothing_while_a_stream_is_capturing(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "2")
    calls = []
    _recording(monkeypatch, calls)
    m = _module(page_size=32, num_pages=12)                      # shared mode: + T for every sequence
    m(_Hidden(2, 31))
    assert m._len_bound == [31, 31] and m.free_pages == 10
    monkeypatch.setattr(QuantAttentionFused, "_capturing", staticmethod(lambda: True))
    m(_Hidden(2, 1))                                             # position 31: the page is there, nothing to allocate
    assert m.free_pages == 10 and m._len_bound == [32, 32]
    before = m.block_table.clone()
    calls.clear()
    with pytest.raises(RuntimeError, match="reserve"):
        m(_Hidden(2, 1))                                         # position 32 needs a page: refused, told to reserve
    assert calls == [] and torch.equal(m.block_table, before) and m.free_pages == 10 and m._len_bound == [32, 32]
    with pytest.raises(RuntimeError, match="capturing"):
        m.reserve(40)
    monkeypatch.setattr(QuantAttentionFused, "_capturing", staticmethod(lambda: False))
    m.reserve(40)
    monkeypatch.setattr(QuantAttentionFused, "_capturing", staticmethod(lambda: True))
    m(_Hidden(2, 1))
    assert m.free_pages == 8 and m._len_bound == [33, 33] and [c[0] for c in calls] == ["rope_attention"]


def test_kernels_refuse_block_table_combinations():
    pool = torch.zeros(4, 2, 32, 128, dtype=torch.float16)
    table = torch.zeros(1, 4, dtype=torch.int32)
    x = torch.zeros(1, 8 * 128, dtype=torch.float16)
    pos = torch.zeros(1, dtype=torch.int64)
    paged = dict(block_table=table, page_size=32, table_rows=64)
    launches = (lambda k, v, **kw: kernels.rope_attention(x, x, x, pos, k, v, x, 4, 2, 128, **kw),
                lambda k, v, **kw: kernels.rope_kv_write(x, x, x, pos, x, k, v, 1, 4, 2, 128, **kw),
                lambda k, v, **kw: kernels.prefill_attention(x, k, v, pos, x, 4, 2, 128, **kw))
    for launch in launches:
        with pytest.raises(ValueError, match="window"):
            launch(pool, pool, window=8, **paged)
        for cache in (pool.view(torch.uint8)[..., :128].contiguous(), pool.view(torch.uint8)[..., :128].contiguous().view(torch.float8_e4m3fn)):
            with pytest.raises(ValueError, match="one-byte"):
                launch(cache, cache, **paged)
        for scales in (dict(k_scale=0.5), dict(v_scale=2.0)):
            with pytest.raises(ValueError, match="k_scale / v_scale"):
                launch(pool, pool, **scales, **paged)
        with pytest.raises(ValueError, match="page_size"):
            launch(pool, pool, block_table=table, table_rows=64)
        with pytest.raises(ValueError, match="pool"):
            launch(pool, pool, block_table=table, page_size=64, table_rows=64)           # the pools' third dimension is the page size
        with pytest.raises(ValueError, match="int32"):
            launch(pool, pool, block_table=table.long(), page_size=32, table_rows=64)
        with pytest.raises(ValueError, match="int32"):
            launch(pool, pool, block_table=torch.zeros(2, 4, dtype=torch.int32), page_size=32, table_rows=64)   # one row per sequence
        with pytest.raises(ValueError, match="GPU"):
            launch(pool, pool, **paged)                                                  # a CPU table: refused before the library
