"""QuantAttentionFused(per_sequence=True) on the GPU: a ragged batch -- a right-padded prompt chunk, decode steps with an idle sequence, a
slot that is reset and refilled while the others decode -- against each sequence run ALONE through a per_sequence=False, batch-1 module
(the code path as it was), fed the same real tokens.

The layers: hidden 512, 4 heads, 4 or 1 KV heads, G = 128, weights that quantise exactly (conftest.exact_layer), max_seq_len = 96.

The bounds are those tests/test_attention_module_gpu.py applies between its stages, taken from that file.  The batch-1 module is handed the
batch's own qkv rows (that file's qkv_rows hook), so that what differs is the attention launch: attention_weight of every real token, of
both modules, lies within the kernel's bound (_prefill_bound for a chunk, _decode_bound for a single token) of float64 attention of the
batch-1 module's fp16 q and caches -- they then agree within the sum; attn_output lies within TOL = 2e-3 of the oracle's GEMM of its own
attention_weight, and the two attn_outputs agree within the sum of those and the attention bounds carried through |W|.  The float64
references are checked to be finite for every examined row.  Outputs of padding rows and of idle sequences are not examined."""
import numpy as np
import pytest
import torch

from conftest import exact_layer, rel_err
from oracle import w4a16
from quick_amd import QuantAttentionFused, WQLinear_QUICK, packing
from test_attention_module_gpu import TOL, _rope_model
from test_prefill_attention_gpu import D, _bits_equal, _decode_bound, _prefill_bound, _reference

pytestmark = pytest.mark.gpu

HIDDEN, NH, G, MAXLEN, B = 512, 4, 128, 96, 3
PROMPTS = (5, 33, 18)
# (T, new_tokens, slots to reset first)
SCHEDULE = [(33, [5, 33, 18], None), (1, [1, 1, 1], None), (1, [1, 0, 1], None), (1, [1, 1, 1], None), (1, [1, 1, 1], None),
            (7, [7, 1, 1], [0])]


def _linear(K, N, seed, device):
    iw, s, z = (torch.from_numpy(a) for a in exact_layer(K, N, G, seed))
    m = WQLinear_QUICK(4, G, K, N, False, "cpu")
    m.load_state_dict(dict(zip(("qweight", "scales", "qzeros"), packing.pack_cuda_order(iw, s, z))))
    return m.to(device), (iw.numpy(), s.numpy(), z.numpy())


@pytest.fixture(scope="module", params=[4, 1], ids=["nkv4", "nkv1"])
def layers(request, device, monkeypatch_module):
    nkv = request.param
    qkv, _ = _linear(HIDDEN, (NH + 2 * nkv) * D, 81 + nkv, device)
    o, o_logical = _linear(HIDDEN, HIDDEN, 91 + nkv, device)
    w_abs = np.abs(w4a16.dequantize(*o_logical, G).astype(np.float64))
    x = [(torch.randn(B, T, HIDDEN, generator=torch.Generator().manual_seed(100 + i)) * 0.5).half().to(device)
         for i, (T, _, _) in enumerate(SCHEDULE)]
    return nkv, qkv, o, o_logical, w_abs, x


@pytest.fixture(scope="module")
def monkeypatch_module():
    mp = pytest.MonkeyPatch()
    mp.delenv("AWQ_BATCH_SIZE", raising=False)
    yield mp
    mp.undo()


def _forward(m, x, rows=None, **kw):
    """One forward; returns (qkv_proj's output -- replaced by `rows` when given --, attn_output, attention_weight)."""
    seen = []
    hook = m.qkv_proj.register_forward_hook(lambda mod, inp, out: seen.append(out if rows is None else rows) or seen[-1])
    try:
        attn_output, attention_weight, past = m(x, **kw)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert len(past) == 1 and tuple(past[0].shape) == (1, 1, m.start_pos, 1)
    return seen[0], attn_output, attention_weight


def _run_schedule(m, x):
    """The ragged batch through `m`; returns per call (qkv rows [B, T, W], attn_output [B, T, H], attention_weight [B, T, H]) and checks the
    positions after every forward."""
    lengths, bound, calls = [0] * B, 0, []
    for (T, nt, reset), xt in zip(SCHEDULE, x):
        if reset is not None:
            m.reset(slots=reset)
            for b in reset:
                lengths[b] = 0
            bound = max(lengths)
            assert m.start_pos == bound
        qkv, out, att = _forward(m, xt, new_tokens=nt)
        lengths = [n + k for n, k in zip(lengths, nt)]
        bound += max(nt)
        assert m.pos.tolist() == lengths and m.start_pos == bound, (m.pos.tolist(), lengths, m.start_pos, bound)
        calls.append((qkv.view(B, T, -1), out, att.reshape(B, T, -1)))
    return calls


def test_ragged_batch_matches_each_sequence_alone(device, layers):
    nkv, qkv_l, o_l, o_logical, w_abs, x = layers
    m = QuantAttentionFused(HIDDEN, NH, nkv, qkv_l, o_l, device, MAXLEN, per_sequence=True)
    allocate = m._allocate

    def allocate_poisoned(batch, dev):       # rows nobody wrote hold NaN: a row read too early poisons the output
        allocate(batch, dev)
        m.k_cache.fill_(float("nan"))
        m.v_cache.fill_(float("nan"))
    m._allocate = allocate_poisoned
    assert m.pos.tolist() == [0]            # (allocated for one sequence; the first forward re-makes caches and positions for three)
    calls = _run_schedule(m, x)
    assert m.cache_batch_size == B and tuple(m.k_cache.shape) == (B, nkv, MAXLEN, D) and m.pos.tolist() == [7, 37, 23]
    w_deq = w4a16.dequantize(*o_logical, G).astype(np.float64)
    alone = QuantAttentionFused(HIDDEN, NH, nkv, qkv_l, o_l, device, MAXLEN)       # today's module: one position, batch 1
    examined = 0
    for b in range(B):
        alone.reset()
        for (T, nt, reset), xt, (qkv, out, att) in zip(SCHEDULE, x, calls):
            n = nt[b]
            if reset is not None and b in reset:
                alone.reset()
            if n == 0:
                continue                     # an idle step of this sequence
            p0 = alone.start_pos
            rows = qkv[b, :n].contiguous()
            _, out_1, att_1 = _forward(alone, xt[b:b + 1, :n], rows=rows)
            assert alone.pos.tolist() == [p0 + n]
            # float64 attention of the batch-1 module's fp16 q and caches
            c, s = (t[p0:p0 + n].cpu().numpy()[None, :, None] for t in (alone.cos, alone.sin))
            q_np = rows.view(1, n, NH + 2 * nkv, D)[:, :, :NH].cpu().numpy()
            q_rot = torch.from_numpy(_rope_model(q_np, c, s)).to(device).transpose(1, 2).contiguous()
            qd, Kd, Vd, vis, sc, P, ref = _reference(q_rot, alone.k_cache, alone.v_cache, p0)
            assert torch.isfinite(ref).all() and torch.isfinite(att_1).all() and torch.isfinite(out_1).all(), (b, p0, n, "a reference is not finite")
            chunk = _prefill_bound(qd, Kd, Vd, vis, sc, P, ref, p0)
            single = _decode_bound(qd[:, :, :, 0], Kd, Vd, p0, sc[:, :, :, 0], P[:, :, :, 0], ref[:, :, :, 0])[:, :, :, None] if n == 1 else None
            bound_1 = single if n == 1 else chunk         # the batch-1 module ran n tokens, the batch T rows
            bound_b = single if T == 1 else chunk
            view = lambda a: a.double().reshape(1, n, nkv, NH // nkv, D).permute(0, 2, 3, 1, 4)
            got_1, got_b = view(att_1), view(att[b, :n])
            r1, rb = float(((got_1 - ref).abs() / bound_1).max()), float(((got_b - ref).abs() / bound_b).max())
            assert r1 <= 1.0 and rb <= 1.0, (b, p0, n, T, r1, rb)
            # attn_output: each within TOL of the oracle's GEMM of its own attention_weight; the two agree within the sum and what the
            # attention bounds become behind |W|
            a1, ab = att_1.double().cpu().numpy().reshape(n, HIDDEN), att[b, :n].double().cpu().numpy().reshape(n, HIDDEN)
            o1, ob = out_1.double().cpu().numpy().reshape(n, HIDDEN), out[b, :n].double().cpu().numpy().reshape(n, HIDDEN)
            want_1, want_b = a1 @ w_deq, ab @ w_deq
            assert rel_err(o1, want_1) <= TOL and rel_err(ob, want_b) <= TOL, (b, p0, n, rel_err(o1, want_1), rel_err(ob, want_b))
            carried = (bound_1 + bound_b).permute(0, 3, 1, 2, 4).reshape(n, HIDDEN).cpu().numpy() @ w_abs
            allowed = TOL * (np.abs(want_1).max() + np.abs(want_b).max()) + carried
            assert (np.abs(o1 - ob) <= allowed).all(), (b, p0, n, float((np.abs(o1 - ob) / allowed).max()))
            examined += n
    assert examined == sum(sum(nt) for _, nt, _ in SCHEDULE)


def test_a_captured_decode_step_replays_the_eager_steps_bit_for_bit(device, layers):
    """One decode step with a device new_tokens and static inputs, captured in a graph and replayed three times, against the same three
    steps run eagerly from the same state: outputs, positions and caches bit for bit.  Sequence 1 idles (new_tokens = [1, 0, 1])."""
    nkv, qkv_l, o_l, _, _, x = layers
    m = QuantAttentionFused(HIDDEN, NH, nkv, qkv_l, o_l, device, MAXLEN, per_sequence=True)
    m(x[0], new_tokens=list(PROMPTS))
    torch.cuda.synchronize()
    state = (m.pos.clone(), m.k_cache.clone(), m.v_cache.clone(), m.start_pos)

    def restore():
        m.pos.copy_(state[0])
        m.k_cache.copy_(state[1])
        m.v_cache.copy_(state[2])
        m.start_pos = state[3]
    steps = [x[i].clone() for i in (1, 2, 3)]
    nt = torch.tensor([1, 0, 1], dtype=torch.int64, device=device)
    eager = []
    for xt in steps:
        out, att, _ = m(xt, new_tokens=nt)
        eager.append((out.clone(), att.clone()))
    torch.cuda.synchronize()
    assert m.pos.tolist() == [PROMPTS[0] + 3, PROMPTS[1], PROMPTS[2] + 3] and m.start_pos == max(PROMPTS) + 3     # (a device count: the bound moves by T)
    eager_state = (m.pos.clone(), m.k_cache.clone(), m.v_cache.clone())
    restore()
    static_x = steps[0].clone()
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):            # warm-up on a side stream, as torch requires before capture
        m(static_x, new_tokens=nt)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_g, att_g, _ = m(static_x, new_tokens=nt)
    restore()                                # (capture executes nothing, but advances the host-side bound)
    torch.cuda.synchronize()
    for xt, (out_e, att_e) in zip(steps, eager):
        static_x.copy_(xt)
        graph.replay()
        torch.cuda.synchronize()
        real = [0, 2]
        assert _bits_equal(out_g[real], out_e[real]) and _bits_equal(att_g[real], att_e[real])
    assert torch.equal(m.pos, eager_state[0]) and _bits_equal(m.k_cache, eager_state[1]) and _bits_equal(m.v_cache, eager_state[2])


def test_decode_step_fused_takes_one_position_per_sequence(device):
    """SyntheticDecoder("tiny"), three sequences at positions 20, 7 and 13 over a prefilled cache: the fused step with pos of B elements
    against torch_decode_hidden of each sequence alone at its position, <= 1e-2 on the hidden state (tests/test_gemm_gpu.py's closeness
    for the synthetic decoder); one element still means one position for all."""
    from quick_amd.decoder import CONFIGS, SyntheticDecoder, decode_step_fused, torch_decode_hidden
    L, ctx = 40, 20
    mb = SyntheticDecoder(CONFIGS["tiny"], batch=B, max_len=L, device=device, seed=3)
    m1 = SyntheticDecoder(CONFIGS["tiny"], batch=1, max_len=L, device=device, seed=3)
    tokens = torch.randint(0, 512, (B, ctx), generator=torch.Generator().manual_seed(9)).to(device)
    tok = mb.forward(tokens, torch.arange(ctx, device=device), None).view(B, 1)
    before = [(l["k"].clone(), l["v"].clone()) for l in mb.layers]
    pos = torch.tensor([20, 7, 13], dtype=torch.int64, device=device)
    _, hid = decode_step_fused(mb, tok, pos)
    torch.cuda.synchronize()
    for b in range(B):
        p = int(pos[b])
        for l1, (k0, v0) in zip(m1.layers, before):
            l1["k"].copy_(k0[b:b + 1])
            l1["v"].copy_(v0[b:b + 1])
        mask = torch.full((1, 1, 1, L), float("-inf"), dtype=torch.float16, device=device)
        mask[..., :p + 1] = 0
        ref = torch_decode_hidden(m1, tok[b:b + 1], pos[b:b + 1], mask)
        assert torch.isfinite(ref).all()
        err = (hid[b:b + 1].float() - ref.float()).abs().max() / ref.float().abs().max()
        assert err <= 1e-2, (b, p, float(err))
        for lb, l1, (k0, v0) in zip(mb.layers, m1.layers, before):
            ka, kb = l1["k"][0, :, p].float(), lb["k"][b, :, p].float()
            assert (ka - kb).abs().max() <= 1e-2 * ka.abs().max() + 1e-3
            keep = [r for r in range(L) if r != p]
            assert _bits_equal(lb["k"][b, :, keep], k0[b, :, keep]) and _bits_equal(lb["v"][b, :, keep], v0[b, :, keep])
    with pytest.raises(ValueError, match="one per sequence"):
        decode_step_fused(mb, tok, pos[:2])
