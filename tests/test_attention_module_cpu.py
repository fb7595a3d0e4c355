"""QuantAttentionFused, host side: construction on the CPU from small WQLinear_QUICK layers (hidden 512, 4 heads, 2 KV heads, G = 128),
what state_dict() holds, every refusal of the constructor and of forward, and the error of a forward without a GPU."""
import pytest
import torch

import quick_amd
from quick_amd import QuantAttentionFused, WQLinear_QUICK

HIDDEN, NH, NKV, G, MAXLEN = 512, 4, 2, 128, 64
WIDTH = (NH + 2 * NKV) * 128


def _layers(width=WIDTH):
    return WQLinear_QUICK(4, G, HIDDEN, width, False, "cpu"), WQLinear_QUICK(4, G, HIDDEN, HIDDEN, False, "cpu")


def _module(**kw):
    qkv, o = _layers()
    return QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, **kw)


def test_construction_state_and_state_dict(monkeypatch):
    monkeypatch.delenv("AWQ_BATCH_SIZE", raising=False)
    assert quick_amd.QuantAttentionFused is QuantAttentionFused
    qkv, o = _layers()
    m = QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN)
    assert m.qkv_proj is qkv and m.o_proj is o and [n for n, _ in m.named_children()] == ["qkv_proj", "o_proj"]
    assert (m.hidden_size, m.n_heads, m.n_kv_heads, m.n_kv_groups, m.head_dim, m.max_seq_len) == (HIDDEN, NH, NKV, 2, 128, MAXLEN)
    assert m.start_pos == 0 and m.cache_batch_size == 1 and m.use_alibi is False and m.is_neox and m.rotary_dim == 128 and m.rope_theta == 10000
    want = {f"{p}.{n}" for p in ("qkv_proj", "o_proj") for n in ("qweight", "qzeros", "scales")}
    assert set(m.state_dict()) == want == {f"qkv_proj.{k}" for k in qkv.state_dict()} | {f"o_proj.{k}" for k in o.state_dict()}
    assert list(m.parameters()) == [] and {n for n, _ in m.named_buffers()} == want
    for cache in (m.k_cache, m.v_cache):
        assert cache.dtype == torch.float16 and tuple(cache.shape) == (1, NKV, MAXLEN, 128)
    assert m.pos.dtype == torch.int64 and m.pos.tolist() == [0]
    # the tables: HF rotate-half, both halves carry the same angles, built as quick_amd.decoder builds them
    inv = 1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))
    ang = torch.outer(torch.arange(MAXLEN).float(), inv)
    assert m.cos.dtype == torch.float16 and tuple(m.cos.shape) == (MAXLEN, 128)
    assert torch.equal(m.cos, torch.cat((ang.cos(), ang.cos()), -1).half()) and torch.equal(m.sin, torch.cat((ang.sin(), ang.sin()), -1).half())
    m.start_pos = 5
    m.pos.fill_(5)
    m.reset()
    assert m.start_pos == 0 and m.pos.tolist() == [0]


def test_cache_batch_size_comes_from_the_environment(monkeypatch):
    monkeypatch.setenv("AWQ_BATCH_SIZE", "3")
    m = _module()
    assert m.cache_batch_size == 3 and tuple(m.k_cache.shape) == (3, NKV, MAXLEN, 128)


def test_constructor_refusals_name_their_cause():
    qkv, o = _layers()
    with pytest.raises(ValueError, match="use_alibi"):
        QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, use_alibi=True)
    with pytest.raises(ValueError, match="attention_shapes"):
        QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, "cpu", MAXLEN, attention_shapes={"xqkv_view": (-1, 128)})
    with pytest.raises(ValueError, match="head_dim must be 128"):
        QuantAttentionFused(HIDDEN, 8, 2, qkv, o, "cpu", MAXLEN)                       # 512 // 8 == 64
    with pytest.raises(ValueError, match=r"qkv_layer must map 512 to .* 1024 channels, it maps 512 to 1536"):
        QuantAttentionFused(HIDDEN, NH, NKV, _layers(1536)[0], o, "cpu", MAXLEN)
    with pytest.raises(ValueError, match="multiple of n_kv_heads"):
        QuantAttentionFused(HIDDEN, NH, 3, qkv, o, "cpu", MAXLEN)


def test_forward_refuses_to_run_past_the_cache_and_says_so():
    m = _module()
    x = torch.zeros(1, MAXLEN + 1, HIDDEN, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"start_pos \+ tokens = 0 \+ 65 exceeds max_seq_len = 64.*does not roll"):
        m(x)
    m.start_pos = 60
    with pytest.raises(ValueError, match=r"60 \+ 5 exceeds max_seq_len"):
        m(x[:, :5])


def test_forward_without_a_gpu_raises_the_gpu_error():
    m = _module()
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 4, HIDDEN, dtype=torch.float16))
    with pytest.raises(RuntimeError, match="GPU"):
        m(torch.zeros(1, 1, HIDDEN, dtype=torch.float16), attention_mask=torch.zeros(1, 1, 1, 1))
    assert m.start_pos == 0
