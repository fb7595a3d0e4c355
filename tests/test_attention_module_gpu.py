"""QuantAttentionFused on the GPU, stage by stage so that no tolerance compounds: the cache rows against the RoPE model bit for bit, the
attention in front of o_proj against float64 attention of the module's own fp16 qkv output within the kernels' bounds, o_proj against the
oracle's GEMM at the suite's 2e-3; chunked prefill against one prefill; and the synthetic decoder's hip_attention switch.

The layer: hidden 512, 4 heads, 2 KV heads, G = 128, weights from quantize_linear on seeded fp16 matrices, max_seq_len = 256."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import w4a16
from quick_amd import QuantAttentionFused, quantize_linear
from test_prefill_attention_gpu import D, _bits_equal, _decode_bound, _prefill_bound, _reference

pytestmark = pytest.mark.gpu

TOL = 2e-3      # tests/test_gemm_gpu.py's bound, as tests/test_gate_up_gpu.py applies it
HIDDEN, NH, NKV, G, MAXLEN = 512, 4, 2, 128, 256
CALLS = (37, 5, 64, 1, 1, 1)     # a prefill from 0, two chunks, three single tokens
NAN = float("nan")


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


@pytest.fixture(scope="module")
def layer(device):
    """(module, logical o_proj weights for the oracle, the hidden states of all calls [2, 109, 512]); made once."""
    g = torch.Generator().manual_seed(2024)
    lin = lambda n_out: torch.nn.Linear(HIDDEN, n_out, bias=False, dtype=torch.float16)
    qkv_lin, o_lin = lin((NH + 2 * NKV) * D), lin(HIDDEN)
    qkv_lin.weight.data = (torch.randn(qkv_lin.weight.shape, generator=g) * 0.06).half()
    o_lin.weight.data = (torch.randn(o_lin.weight.shape, generator=g) * 0.04).half()
    qkv, o = quantize_linear(qkv_lin, 4, G).to(device), quantize_linear(o_lin, 4, G).to(device)
    o_logical = w4a16.unpack_mi355x(*[t.cpu().numpy() for t in (o.qweight, o.scales, o.qzeros)])
    m = QuantAttentionFused(HIDDEN, NH, NKV, qkv, o, device, MAXLEN)
    allocate = m._allocate

    def allocate_poisoned(batch, dev):        # rows nobody wrote hold NaN: an untouched row shows as such, a row read too early poisons the output
        allocate(batch, dev)
        m.k_cache.fill_(NAN)
        m.v_cache.fill_(NAN)
    m._allocate = allocate_poisoned
    m._allocate(m.cache_batch_size, device)
    x = torch.randn(2, sum(CALLS), HIDDEN, generator=g).half().to(device)
    return m, o_logical, x


def _call(m, x, o_logical, kc_want, vc_want, qkv_rows=None):
    """One forward of `m` on x [B, T, hidden] at its current position, every stage checked; the expected caches are advanced in place.
    ``qkv_rows``: what qkv_proj is made to return (the hook replaces its output).  Returns (qkv output, attention_weight, its bound)."""
    B, T, _ = x.shape
    p0 = m.start_pos
    seen = []
    hook = m.qkv_proj.register_forward_hook(lambda mod, inp, out: seen.append(out if qkv_rows is None else qkv_rows) or seen[-1])
    try:
        attn_output, attention_weight, past = m(x, attention_mask=None)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert m.start_pos == p0 + T and m.pos.tolist() == [p0 + T]
    assert len(past) == 1 and tuple(past[0].shape) == (1, 1, p0 + T, 1)
    assert tuple(attn_output.shape) == (B, T, HIDDEN) == tuple(attention_weight.shape) and attn_output.dtype == torch.float16
    qkv = seen[0].reshape(B, T, NH + 2 * NKV, D)
    # the caches: rows p0 .. p0 + T - 1 are the RoPE model's, every other row is as it was
    c, s = (t[p0:p0 + T].cpu().numpy()[None, :, None] for t in (m.cos, m.sin))
    qkv_np = qkv.cpu().numpy()
    q_rot = torch.from_numpy(_rope_model(qkv_np[:, :, :NH], c, s)).to(x.device).transpose(1, 2).contiguous()           # [B, nh, T, D]
    kc_want[:, :, p0:p0 + T] = torch.from_numpy(_rope_model(qkv_np[:, :, NH:NH + NKV], c, s)).to(x.device).transpose(1, 2)
    vc_want[:, :, p0:p0 + T] = qkv[:, :, NH + NKV:].transpose(1, 2)
    assert _bits_equal(m.k_cache, kc_want) and _bits_equal(m.v_cache, vc_want), (p0, T, "cache rows")
    # attention_weight against float64 attention of the module's own fp16 q and caches
    qd, Kd, Vd, vis, sc, P, ref = _reference(q_rot, kc_want, vc_want, p0)
    if T > 1:
        bound = _prefill_bound(qd, Kd, Vd, vis, sc, P, ref, p0)
    else:
        bound = _decode_bound(qd[:, :, :, 0], Kd, Vd, p0, sc[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])[:, :, :, None]
    got = attention_weight.double().view(B, T, NKV, NH // NKV, D).permute(0, 2, 3, 1, 4)
    ratio = float(((got - ref).abs() / bound).max())
    print(f"[attention-module] B={B} pos0={p0} T={T}: attention err/bound {ratio:.3f}")
    assert ratio <= 1.0, (B, p0, T, ratio)
    # attn_output against the oracle's GEMM of that attention_weight
    want = attention_weight.double().cpu().numpy().reshape(B * T, HIDDEN) @ w4a16.dequantize(*o_logical, G).astype(np.float64)
    err = rel_err(attn_output.float().cpu().numpy().reshape(B * T, HIDDEN), want)
    assert err <= TOL, (B, p0, T, err)
    return seen[0], got, bound


@pytest.mark.parametrize("B", [2, 1])
def test_prefill_chunks_and_single_tokens_stage_by_stage(device, layer, B):
    """One instance: prefill of 37 from 0, chunks of 5 and 64, three single tokens (B = 2: the module starts with AWQ_BATCH_SIZE = 1 rows
    and reallocates; B = 1 afterwards reallocates again), every call checked by _call.  Then, after reset(), the 106 prefill tokens as
    ONE prefill on the chunked run's qkv rows: attention_weight agrees with the chunked rows within twice the bound -- chunking does not
    change the answer."""
    m, o_logical, x = layer
    m.reset()
    x = x[:B]
    kc_want = torch.full((B, NKV, MAXLEN, D), NAN, dtype=torch.float16, device=device)
    vc_want = kc_want.clone()
    at, qkvs, atts = 0, [], []
    for T in CALLS:
        qkv, got, _ = _call(m, x[:, at:at + T], o_logical, kc_want, vc_want)
        assert m.cache_batch_size == B
        qkvs.append(qkv.reshape(B, T, -1))
        atts.append(got)
        at += T
    n = sum(CALLS[:3])
    m.reset()
    assert m.start_pos == 0 and m.pos.tolist() == [0]
    kc_one, vc_one = kc_want.clone(), vc_want.clone()       # (reset() leaves the rows; the prefill rewrites the first 106 with the same bits)
    rows = torch.cat(qkvs[:3], 1).reshape(B * n, -1).contiguous()
    _, one, bound = _call(m, x[:, :n], o_logical, kc_one, vc_one, qkv_rows=rows)
    diff = (one - torch.cat(atts[:3], 3)).abs()
    assert float((diff / (2 * bound)).max()) <= 1.0, float((diff / (2 * bound)).max())


def test_synthetic_decoder_hip_attention_matches_sdpa_and_the_eager_mask(device):
    """SyntheticDecoder("tiny"): a prefill from 0 with hip_attention gives the same next tokens as SDPA and the hidden state within the
    full-stack tolerance of tests/test_gemm_gpu.py (1e-2 of the largest element); a chunk of 8 at position 16 matches the eager-torch
    branch run with an explicit causal-over-cache mask."""
    from quick_amd.decoder import CONFIGS, SyntheticDecoder
    batch, L = 3, 40
    models = [SyntheticDecoder(CONFIGS["tiny"], batch=batch, max_len=L, device=device, seed=3) for _ in range(3)]
    tokens = torch.randint(0, 512, (batch, 24), generator=torch.Generator().manual_seed(5)).to(device)
    first = torch.arange(16, device=device)
    tok_a, hid_a = models[0].forward(tokens[:, :16], first, None, hip_attention=True, return_hidden=True)
    tok_b, hid_b = models[1].forward(tokens[:, :16], first, None, hip_attention=False, return_hidden=True)
    close = lambda a, b: float((a.float() - b.float()).abs().max() / b.float().abs().max())
    assert torch.equal(tok_a, tok_b) and close(hid_a, hid_b) <= 1e-2, close(hid_a, hid_b)
    models[2].forward(tokens[:, :16], first, None, hip_glue=False)
    chunk = torch.arange(16, 24, device=device)
    mask = torch.full((1, 1, 8, L), float("-inf"), dtype=torch.float16, device=device)
    for t in range(8):
        mask[0, 0, t, :16 + t + 1] = 0
    _, hid_hip = models[0].forward(tokens[:, 16:], chunk, None, hip_attention=True, return_hidden=True)
    _, hid_ref = models[2].forward(tokens[:, 16:], chunk, mask, hip_glue=False, return_hidden=True)
    assert close(hid_hip, hid_ref) <= 1e-2, close(hid_hip, hid_ref)
    for la, lc in zip(models[0].layers, models[2].layers):
        ka, kc = la["k"][:, :, :24].float(), lc["k"][:, :, :24].float()
        assert float((ka - kc).abs().max()) <= 1e-2 * float(kc.abs().max()) + 1e-3
