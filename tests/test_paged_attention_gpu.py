"""Attention over a paged KV cache on the GPU (quick_*_paged_f16): the pool write bit for bit against the linear write, the fused decode
step bit for bit against the grouped MFMA sweep on the gathered linear cache (quick_decode_rope_attention_win_f16 with ring_rows = window
= table_rows) and within its float64 bound, the MFMA prefill bit for bit against quick_prefill_attention_f16 and within its float64
bound, the launches against each other, per-sequence positions, the safety rules for table entries that name no page, a shared prefix,
reproducibility against the forcezero twin, and QuantAttentionFused(page_size=..., num_pages=...) stage by stage against the default
module and a never-wrapping windowed module, with the page accounting, a captured decode step and an exhausted pool.

Fixtures: pools of 24 pages; tables scrambled (reversed, and interleaved between the sequences); every page no sequence holds and every
row of a held page that no position has written poisoned (NaN keys, +-Inf values) AFTER the fill; table columns behind the last needed
one are -1.  After every launch the WHOLE pool is compared bit for bit with the pool before it plus the rows the launch must write.
Shapes are the smallest at which the mapping can go wrong: pages of 32 and 64 positions, at most 256 positions."""
import pytest
import torch

import test_prefill_attention_gpu as PF
import test_sliding_window_gpu as GW
from quick_amd.attention import gather_pages, paged_slot
from test_decode_ops_gpu import _check_guard, _poisoned, _tables
from test_sliding_window_gpu import _i16, _pos

pytestmark = pytest.mark.gpu

D = 128
NP = GW.NP                     # rows of the cos / sin tables
TR = 256                       # table_rows of every launch here: with max_pages * P = 256 the exclusive bound on positions
NPAGES = 24
SCALE = D ** -0.5
PAGES = (32, 64)
DEC_P = (0, 15, 16, 31, 32, 63, 64, 95, 200)
PF_CASES = ((0, 65), (20, 17), (100, 65), (190, 33))


@pytest.fixture(scope="module")
def K_(device):
    from quick_amd import _lib, kernels
    _lib.load()
    return kernels


@pytest.fixture(scope="module")
def tables(device):
    cos_np, sin_np = _tables(NP, 1e4)
    return cos_np, sin_np, torch.from_numpy(cos_np).to(device), torch.from_numpy(sin_np).to(device)


def poison_pool(nkv, P, device, pages=NPAGES):
    """A pool nobody has written: NaN keys, +-Inf values."""
    k = torch.full((pages, nkv, P, D), float("nan"), dtype=torch.float16, device=device)
    v = torch.full((pages, nkv, P, D), float("inf"), dtype=torch.float16, device=device)
    v[:, :, 1::2] = float("-inf")
    return k, v


def scrambled_table(lengths, P, device, pages=NPAGES):
    """int32 [B, 256 / P]: sequence b holds the pages of positions 0 .. lengths[b] - 1 and -1 behind them.  Column i of sequence b is page
    pages - 1 - (i B + b): reversed, and interleaved between the sequences."""
    B, MP = len(lengths), TR // P
    assert B * MP <= pages
    t = torch.full((B, MP), -1, dtype=torch.int32)
    for b, n in enumerate(lengths):
        for i in range(-(-n // P)):
            t[b, i] = pages - 1 - (i * B + b)
    return t.to(device)


def put_rows(k, v, table, lin_k, lin_v, b, lo, hi):
    """Positions lo .. hi - 1 of sequence b from the linear [B, nkv, *, D] streams into their pool rows; nothing else is touched."""
    if hi <= lo:
        return
    pos = torch.arange(lo, hi, device=k.device)
    page, row = paged_slot(pos, table[b], k.shape[2])
    assert int(page.min()) >= 0
    k[page, :, row] = lin_k[b][:, lo:hi].transpose(0, 1)
    v[page, :, row] = lin_v[b][:, lo:hi].transpose(0, 1)


def pools_equal(k, v, k_want, v_want):
    return torch.equal(_i16(k), _i16(k_want)) and torch.equal(_i16(v), _i16(v_want))


def paged_kw(table, P):
    return dict(block_table=table, page_size=P, table_rows=TR)


# ------------------------------------------------------------------------------------------------
# the write
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_sequence", [False, True], ids=["shared", "per-sequence"])
@pytest.mark.parametrize("T", [1, 17, 65])
@pytest.mark.parametrize("P", PAGES)
def test_pool_write_equals_the_linear_write_bit_for_bit(K_, device, tables, P, T, per_sequence):
    """pos0 in {0, 20, 100} (page boundaries fall inside a chunk): gather_pages of the pool and q_out equal what quick_rope_kv_write_f16
    writes into a linear cache of table_rows rows, bit for bit; every other pool row keeps its poison.  Per-sequence: mixed positions and
    one skipped slot, whose pages and rows of q_out keep their poison."""
    _, _, cos, sin = tables
    B, nh, nkv = 3, 8, 2
    for pos0 in (0, 20, 100):
        g = torch.Generator(device=device).manual_seed(100 * pos0 + T + P)
        qkv = (torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device) * 2).half()
        starts = [pos0, (-1 if pos0 % 40 else TR - T + 1), (pos0 + 37) % (TR - T)] if per_sequence else [pos0] * B
        pos = torch.tensor(starts if per_sequence else starts[:1], dtype=torch.int64, device=device)
        kl = torch.zeros(B, nkv, TR, D, dtype=torch.float16, device=device)
        vl = torch.zeros_like(kl)
        ql = torch.full((B, nh, T, D), 7.0, dtype=torch.float16, device=device)
        K_.rope_kv_write(qkv, cos, sin, pos, ql, kl, vl, T, nh, nkv, D, per_sequence=per_sequence)
        valid = [0 <= s <= TR - T for s in starts]
        table = scrambled_table([s + T if ok else 40 for s, ok in zip(starts, valid)], P, device)     # (a skipped slot holds pages too)
        kp, vp = poison_pool(nkv, P, device)
        k_want, v_want = kp.clone(), vp.clone()
        qbuf, qp = _poisoned(B, (nh, T, D), device, fill=7.0)
        K_.rope_kv_write(qkv, cos, sin, pos, qp, kp, vp, T, nh, nkv, D, per_sequence=per_sequence, **paged_kw(table, P))
        torch.cuda.synchronize()
        assert bool((qbuf[0] == 7.0).all()) and bool((qbuf[B + 1] == 7.0).all()), "wrote next to q_out"
        assert PF._bits_equal(qp, ql), (pos0, T, "q_out differs from the linear launch")
        for b, s in enumerate(starts):
            if valid[b]:
                put_rows(k_want, v_want, table, kl, vl, b, s, s + T)
                assert torch.equal(_i16(gather_pages(kp, table[b], s + T)[:, s:]), _i16(kl[b][:, s:s + T])), (pos0, T, b, "K rows")
                assert torch.equal(_i16(gather_pages(vp, table[b], s + T)[:, s:]), _i16(vl[b][:, s:s + T])), (pos0, T, b, "V rows")
            else:
                assert bool((qp[b] == 7.0).all()), "a skipped sequence's q_out was written"
        assert pools_equal(kp, vp, k_want, v_want), (pos0, T, per_sequence, "a row outside the written positions changed")


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def decode_case(B, nh, nkv, P, p, seed, device, cos_np, sin_np, lengths=None):
    """GW.decode_case on a cache that never wraps (R = W = table_rows: rows 0 .. p - 1 of a random stream, the rest poisoned) and the same
    thing paged: a scrambled table that holds the pages of positions 0 .. p, the pool with positions 0 .. p - 1 in their rows and every
    other row poisoned.  Returns (qkv, k_lin, v_lin, q_rot, k_rot, table, k_pool, v_pool)."""
    qkv, kl, vl, q_rot, k_rot = GW.decode_case(B, nh, nkv, TR, TR, p, seed, device, cos_np, sin_np)
    table = scrambled_table([p + 1] * B if lengths is None else lengths, P, device)
    kp, vp = poison_pool(nkv, P, device)
    for b in range(B):
        put_rows(kp, vp, table, kl, vl, b, 0, p)
    return qkv, kl, vl, q_rot, k_rot, table, kp, vp


@pytest.mark.parametrize("nh,nkv", GW.DEC_HEADS, ids=[f"group{a // b}" for a, b in GW.DEC_HEADS])
@pytest.mark.parametrize("P", PAGES)
def test_decode_equals_the_grouped_sweep_on_the_gathered_cache(K_, device, tables, P, nh, nkv):
    """B = 3, every p of DEC_P: out and the appended row are bit for bit those of quick_decode_rope_attention_win_f16 on the gathered
    linear cache with ring_rows = window = table_rows (the same sweep in the same order); the rest of the pool keeps its poison; and out
    is within decode_bound_win of the float64 reference."""
    cos_np, sin_np, cos, sin = tables
    B = 3
    assert K_.paged_attention_describe(B, 1, nh, nkv, D, NPAGES, P, TR // P, TR) == \
        f"decode-paged-mfma heads={nh // nkv} waves=4 set_rows=64 page_size={P} max_pages={TR // P} grid={nkv}x{B}"
    for p in DEC_P:
        qkv, kl, vl, q_rot, k_rot, table, kp, vp = decode_case(B, nh, nkv, P, p, 7 * p + nh + P, device, cos_np, sin_np)
        kl0, vl0, k_want, v_want = kl.clone(), vl.clone(), kp.clone(), vp.clone()
        want = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kl, vl, want, nh, nkv, D, window=TR, table_rows=TR)
        buf, out = _poisoned(B, (nh * D,), device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kp, vp, out, nh, nkv, D, **paged_kw(table, P))
        torch.cuda.synchronize()
        _check_guard(buf, B)
        assert PF._bits_equal(out, want), (p, "out differs from the sweep over the linear cache")
        for b in range(B):
            put_rows(k_want, v_want, table, kl, vl, b, p, p + 1)           # the appended row is the linear launch's row p
        assert pools_equal(kp, vp, k_want, v_want), (p, "the appended row / a row outside it")
        ratio = GW.decode_check(qkv, kl, vl, kl0, vl0, out, p, TR, nh, nkv, q_rot, k_rot)
        print(f"[paged-decode] P={P} {nh}/{nkv} p={p}: max err/bound {ratio:.3f}")
        assert ratio <= 1.0, (nh, nkv, p, ratio)


# ------------------------------------------------------------------------------------------------
# prefill
# ------------------------------------------------------------------------------------------------
def prefill_case(B, nh, nkv, P, p0, T, variant, device):
    """PF._dense_case (linear caches of 512 rows, poisoned from pos0 + T on) and the same thing paged.  Returns (q, k_lin, v_lin, table,
    k_pool, v_pool)."""
    q, kc, vc = PF._dense_case(B, nh, nkv, p0, T, variant, device)
    table = scrambled_table([p0 + T] * B, P, device)
    kp, vp = poison_pool(nkv, P, device)
    for b in range(B):
        put_rows(kp, vp, table, kc, vc, b, 0, p0 + T)
    return q, kc, vc, table, kp, vp


def prefill_launch(K_, q, kp, vp, table, P, pos, nh, nkv, per_sequence=False, lib=None, fill=float("nan")):
    """One launch into a poisoned output with guard rows; the pool must come back bit for bit.  Returns out [B * T, nh * D]."""
    B, T = q.shape[0], q.shape[2]
    kp0, vp0 = kp.clone(), vp.clone()
    buf, out = _poisoned(B * T, (nh * D,), q.device, fill=fill)
    if lib is None:
        K_.prefill_attention(q, kp, vp, pos, out, nh, nkv, D, per_sequence=per_sequence, **paged_kw(table, P))
    else:
        rc = lib.quick_prefill_attention_paged_f16(q.data_ptr(), kp.data_ptr(), vp.data_ptr(), pos.data_ptr(), out.data_ptr(), table.data_ptr(),
                                                   B, T, nh, nkv, D, kp.shape[0], P, table.shape[1], TR, SCALE, int(per_sequence),
                                                   torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    torch.cuda.synchronize()
    if fill != fill:
        _check_guard(buf, B * T)
    else:
        assert bool((buf[0] == fill).all()) and bool((buf[B * T + 1] == fill).all()), "wrote next to the output"
    assert pools_equal(kp, vp, kp0, vp0), "the kernel wrote the pool"
    return out


@pytest.mark.parametrize("nh,nkv", PF.HEADS)
@pytest.mark.parametrize("P", PAGES)
def test_prefill_equals_the_linear_launch_on_the_gathered_cache(K_, device, P, nh, nkv):
    """B = 2, every (pos0, T) of PF_CASES, random and peaked: bit for bit quick_prefill_attention_f16 on the gathered linear cache, and
    within PF._prefill_bound of the float64 reference."""
    B = 2
    for p0, T in PF_CASES:
        assert K_.paged_attention_describe(B, T, nh, nkv, D, NPAGES, P, TR // P, TR) == \
            f"prefill-paged-mfma q_rows=64 kv_rows=32 waves=4 page_size={P} max_pages={TR // P} grid={-(-T // 64)}x{nh}x{B}"
        for variant in ("random", "peaked"):
            q, kc, vc, table, kp, vp = prefill_case(B, nh, nkv, P, p0, T, variant, device)
            for b in range(B):
                assert torch.equal(_i16(gather_pages(kp, table[b], p0 + T)), _i16(kc[b][:, :p0 + T]))
            want = PF._launch(K_, q, kc, vc, p0, nh, nkv)
            out = prefill_launch(K_, q, kp, vp, table, P, _pos(p0, device), nh, nkv)
            assert not torch.isnan(out.float()).any(), (p0, T, "NaN in the output: a poisoned row was read")
            assert PF._bits_equal(out, want), (p0, T, variant, "out differs from the linear launch")
            qd, Kd, Vd, vis, s, Pm, ref = PF._reference(q, kc, vc, p0)
            bound = PF._prefill_bound(qd, Kd, Vd, vis, s, Pm, ref, p0)
            err = (GW.rows_to_heads(out.double(), B, T, nkv, nh // nkv) - ref).abs()
            ratio = float((err / bound).max())
            print(f"[paged-prefill] P={P} {nh}/{nkv} pos0={p0} T={T} {variant}: max err/bound {ratio:.3f}")
            assert ratio <= 1.0, (p0, T, variant, ratio)


@pytest.mark.parametrize("nh,nkv", [(4, 4), (8, 2), (8, 1)])
def test_single_token_prefill_agrees_with_decode_on_the_same_pool(K_, device, tables, nh, nkv):
    """The decode step at p appends its row; a one-token prefill at p on that pool, fed the RoPE model's q, is within the sum of both
    kernels' bounds of the decode step's output."""
    cos_np, sin_np, cos, sin = tables
    B, P = 3, 32
    for p in (0, 31, 32, 200):
        qkv, kl, vl, q_rot, k_rot, table, kp, vp = decode_case(B, nh, nkv, P, p, 3 * p + nh, device, cos_np, sin_np)
        dec = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, _pos(p, device), kp, vp, dec, nh, nkv, D, **paged_kw(table, P))
        q = q_rot.view(B, nh, 1, D).contiguous()
        out = prefill_launch(K_, q, kp, vp, table, P, _pos(p, device), nh, nkv)
        lin_k = torch.stack([gather_pages(kp, table[b], p + 1) for b in range(B)])
        lin_v = torch.stack([gather_pages(vp, table[b], p + 1) for b in range(B)])
        qd, Kd, Vd, vis, s, Pm, ref = PF._reference(q, lin_k, lin_v, p)
        bound = PF._prefill_bound(qd, Kd, Vd, vis, s, Pm, ref, p)[:, :, :, 0] + \
            GW.decode_bound_win(qd[:, :, :, 0], Kd, Vd, s[:, :, :, 0], Pm[:, :, :, 0], ref[:, :, :, 0])
        diff = (out.double().view(B, nkv, nh // nkv, D) - dec.double().view(B, nkv, nh // nkv, D)).abs()
        assert float((diff / bound).max()) <= 1.0, (p, float((diff / bound).max()))


# ------------------------------------------------------------------------------------------------
# per-sequence positions
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PAGES)
def test_per_sequence_launches_equal_the_shared_launch_at_each_position(K_, device, tables, P):
    """Each sequence of a per-sequence launch equals the shared launch at its position, bit for bit; a sequence whose position lies
    outside the valid range is skipped: its pages, q_out and out keep their poison."""
    cos_np, sin_np, cos, sin = tables
    B, nh, nkv = 3, 8, 2
    # decode: positions 40 | skipped | 95 -- the skipped slot holds pages (poisoned) all the same
    for bad in (-1, TR):
        ps = [40, bad, 95]
        g = torch.Generator(device=device).manual_seed(P + bad % 7)
        qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
        lin_k, lin_v = GW.stream(B, nkv, 11, device)
        table = scrambled_table([41, 64, 96], P, device)
        kp, vp = poison_pool(nkv, P, device)
        for b in (0, 2):
            put_rows(kp, vp, table, lin_k, lin_v, b, 0, ps[b])
        kp0, vp0 = kp.clone(), vp.clone()
        buf, out = _poisoned(B, (nh * D,), device, fill=7.0)
        K_.rope_attention(qkv, cos, sin, torch.tensor(ps, dtype=torch.int64, device=device), kp, vp, out, nh, nkv, D, per_sequence=True,
                          **paged_kw(table, P))
        torch.cuda.synchronize()
        assert bool((buf[0] == 7.0).all()) and bool((buf[B + 1] == 7.0).all()) and bool((out[1] == 7.0).all())
        k_want, v_want = kp0.clone(), vp0.clone()
        for b in (0, 2):
            k1, v1 = kp0.clone(), vp0.clone()
            one = torch.empty(1, nh * D, dtype=torch.float16, device=device)
            K_.rope_attention(qkv[b:b + 1].contiguous(), cos, sin, _pos(ps[b], device), k1, v1, one, nh, nkv, D,
                              **paged_kw(table[b:b + 1].contiguous(), P))
            torch.cuda.synchronize()
            assert PF._bits_equal(out[b:b + 1], one), ("decode", ps[b])
            page, row = paged_slot(ps[b], table[b], P)
            k_want[page, :, row], v_want[page, :, row] = k1[page, :, row], v1[page, :, row]
        assert pools_equal(kp, vp, k_want, v_want), "decode: the pool outside the two appended rows changed"
    # write + prefill: starts 20 | skipped | 100, T = 17
    T = 17
    for bad in (-1, TR - T + 1):
        starts = [20, bad, 100]
        pos = torch.tensor(starts, dtype=torch.int64, device=device)
        g = torch.Generator(device=device).manual_seed(P + 5)
        qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device).half()
        lin_k, lin_v = GW.stream(B, nkv, 12, device)
        table = scrambled_table([20 + T, 64, 100 + T], P, device)
        kp, vp = poison_pool(nkv, P, device)
        for b in (0, 2):
            put_rows(kp, vp, table, lin_k, lin_v, b, 0, starts[b])
        kp0, vp0 = kp.clone(), vp.clone()
        q = torch.full((B, nh, T, D), 7.0, dtype=torch.float16, device=device)
        K_.rope_kv_write(qkv, cos, sin, pos, q, kp, vp, T, nh, nkv, D, per_sequence=True, **paged_kw(table, P))
        out = prefill_launch(K_, q, kp, vp, table, P, pos, nh, nkv, per_sequence=True, fill=7.0)
        assert bool((q[1] == 7.0).all()) and bool((out[T:2 * T] == 7.0).all()), "a skipped sequence's rows were written"
        k_want, v_want = kp0.clone(), vp0.clone()
        for b in (0, 2):
            k1, v1 = kp0.clone(), vp0.clone()
            q1 = torch.empty(1, nh, T, D, dtype=torch.float16, device=device)
            tb = table[b:b + 1].contiguous()
            K_.rope_kv_write(qkv[b * T:(b + 1) * T].contiguous(), cos, sin, _pos(starts[b], device), q1, k1, v1, T, nh, nkv, D, **paged_kw(tb, P))
            one = prefill_launch(K_, q1, k1, v1, tb, P, _pos(starts[b], device), nh, nkv)
            assert PF._bits_equal(q[b:b + 1], q1) and PF._bits_equal(out[b * T:(b + 1) * T], one), ("write + prefill", starts[b])
            page, row = paged_slot(torch.arange(starts[b], starts[b] + T, device=device), table[b], P)
            k_want[page, :, row], v_want[page, :, row] = k1[page, :, row], v1[page, :, row]
        assert pools_equal(kp, vp, k_want, v_want), "write: the pool outside the two chunks changed"


# ------------------------------------------------------------------------------------------------
# safety: table entries that name no page, padding in pages nobody reserved, a shared prefix
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [-1, NPAGES + 5], ids=["minus-one", "beyond-the-pool"])
@pytest.mark.parametrize("P", PAGES)
def test_a_needed_entry_that_names_no_page_writes_nothing_and_stays_in_the_pool(K_, device, tables, P, bad):
    """Sequence 1 of 3 has a needed table entry of -1 or num_pages + 5 (valid inputs by the rules of the header; nothing here is meant to
    fault): the write launch and the decode launch's append drop its rows of that page -- the whole pool is, bit for bit, the pool before
    plus the other rows -- and the other sequences' q_out and out are those of the run with a sound table."""
    cos_np, sin_np, cos, sin = tables
    B, nh, nkv, T = 3, 8, 2, 17
    pos0 = 2 * P - 12                                             # the chunk crosses from column 1 into column 2
    sound = scrambled_table([pos0 + T] * B, P, device)
    broken = sound.clone()
    broken[1, 2] = bad
    g = torch.Generator(device=device).manual_seed(P)
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=g, device=device).half()
    lin_k, lin_v = GW.stream(B, nkv, 21, device)
    runs = []
    for table in (sound, broken):
        kp, vp = poison_pool(nkv, P, device)
        for b in range(B):
            put_rows(kp, vp, sound, lin_k, lin_v, b, 0, pos0)
        q = torch.empty(B, nh, T, D, dtype=torch.float16, device=device)
        K_.rope_kv_write(qkv, cos, sin, _pos(pos0, device), q, kp, vp, T, nh, nkv, D, **paged_kw(table, P))
        out = prefill_launch(K_, q, kp, vp, table, P, _pos(pos0, device), nh, nkv)
        runs.append((q, kp, vp, out))
    (q_a, k_a, v_a, out_a), (q_b, k_b, v_b, out_b) = runs
    assert PF._bits_equal(q_a, q_b), "q_out depends on the table"
    k_want, v_want = k_a.clone(), v_a.clone()
    kpo, vpo = poison_pool(nkv, P, device)
    page = int(sound[1, 2])
    k_want[page], v_want[page] = kpo[page], vpo[page]             # sequence 1's rows of column 2 were dropped: the page keeps its poison
    assert pools_equal(k_b, v_b, k_want, v_want), "write: a dropped row was stored somewhere, or another row changed"
    for b in (0, 2):
        assert PF._bits_equal(out_a[b * T:(b + 1) * T], out_b[b * T:(b + 1) * T]), "prefill: another sequence's output changed"
    # decode at p = 2 P + 3: the append goes to column 2, the sweep reads columns 0 .. 2
    p = 2 * P + 3
    qkv1 = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
    runs = []
    for table in (sound, broken):
        kp, vp = poison_pool(nkv, P, device)
        for b in range(B):
            put_rows(kp, vp, sound, lin_k, lin_v, b, 0, p)
        before = (kp.clone(), vp.clone())
        out = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv1, cos, sin, _pos(p, device), kp, vp, out, nh, nkv, D, **paged_kw(table, P))
        torch.cuda.synchronize()
        runs.append((kp, vp, out, before))
    (k_a, v_a, out_a, _), (k_b, v_b, out_b, (k0, v0)) = runs
    k_want, v_want = k_a.clone(), v_a.clone()
    row = p % P
    k_want[page, :, row], v_want[page, :, row] = k0[page, :, row], v0[page, :, row]     # sequence 1's append was dropped
    assert pools_equal(k_b, v_b, k_want, v_want), "decode: a dropped append was stored somewhere, or another row changed"
    for b in (0, 2):
        assert PF._bits_equal(out_a[b:b + 1], out_b[b:b + 1]), "decode: another sequence's output changed"


@pytest.mark.parametrize("P", PAGES)
def test_padding_in_a_page_nobody_reserved_does_not_reach_the_real_queries(K_, device, tables, P):
    """A right-padded chunk (the module's ragged step): 22 real tokens at position P - 22, 18 rows of padding behind them, and pages for
    the real tokens only -- the padding's column is -1 and every other page is poisoned.  The padding's rows are dropped and the real
    queries' outputs are those of the run that holds a page for the padding, bit for bit (the padding's tile is staged as zeros: a
    pulled-in page's Inf times a zero weight would be NaN in the queries of the wave that do not attend it)."""
    _, _, cos, sin = tables
    nh, nkv, T, real = 8, 2, 40, 22
    pos0 = P - real
    g = torch.Generator(device=device).manual_seed(P + 1)
    qkv = torch.randn(T, (nh + 2 * nkv) * D, generator=g, device=device).half()
    lin_k, lin_v = GW.stream(1, nkv, 31, device)
    outs = []
    for length in (pos0 + T, pos0 + real):
        table = scrambled_table([length], P, device)
        kp, vp = poison_pool(nkv, P, device)
        put_rows(kp, vp, table, lin_k, lin_v, 0, 0, pos0)
        q = torch.empty(1, nh, T, D, dtype=torch.float16, device=device)
        K_.rope_kv_write(qkv, cos, sin, _pos(pos0, device), q, kp, vp, T, nh, nkv, D, **paged_kw(table, P))
        outs.append(prefill_launch(K_, q, kp, vp, table, P, _pos(pos0, device), nh, nkv))
    assert not torch.isnan(outs[1][:real].float()).any(), "a poisoned page reached a real query"
    assert PF._bits_equal(outs[0][:real], outs[1][:real])


@pytest.mark.parametrize("P", PAGES)
def test_a_shared_prefix_gives_the_results_of_two_private_copies(K_, device, tables, P):
    """Two sequences whose tables name the SAME pages for positions 0 .. 63 and different pages behind them: decode and prefill give,
    bit for bit, what two private copies of the prefix give."""
    _, _, cos, sin = tables
    B, nh, nkv, T, p0 = 2, 8, 2, 17, 70
    lin_k, lin_v = GW.stream(B, nkv, 41, device)
    lin_k[1, :, :64], lin_v[1, :, :64] = lin_k[0, :, :64], lin_v[0, :, :64]
    private = scrambled_table([p0 + T + 1] * B, P, device)
    shared = private.clone()
    shared[1, :64 // P] = shared[0, :64 // P]
    g = torch.Generator(device=device).manual_seed(P + 2)
    q = torch.randn(B, nh, T, D, generator=g, device=device).half()
    qkv = torch.randn(B, (nh + 2 * nkv) * D, generator=g, device=device).half()
    got = []
    for table in (private, shared):
        kp, vp = poison_pool(nkv, P, device)
        for b in range(B):
            put_rows(kp, vp, table, lin_k, lin_v, b, 0, p0 + T)
        pf = prefill_launch(K_, q, kp, vp, table, P, _pos(p0, device), nh, nkv)
        dec = torch.empty(B, nh * D, dtype=torch.float16, device=device)
        K_.rope_attention(qkv, cos, sin, _pos(p0 + T, device), kp, vp, dec, nh, nkv, D, **paged_kw(table, P))
        torch.cuda.synchronize()
        got.append((pf, dec, torch.stack([gather_pages(kp, table[b], p0 + T + 1) for b in range(B)])))
    if P == 32:
        assert int(shared[1, 0]) == int(shared[0, 0]) and int(shared[1, 1]) == int(shared[0, 1]) and int(shared[1, 2]) != int(shared[0, 2])
    for a, b in zip(*got):
        assert PF._bits_equal(a, b)


# ------------------------------------------------------------------------------------------------
# reproducibility
# ------------------------------------------------------------------------------------------------
def test_paged_launches_are_reproducible_and_equal_their_forcezero_build(K_, device, tables):
    """Write, decode (every group) and prefill: two launches give bit-equal results, and so does the -amdgpu-waitcnt-forcezero build."""
    from quick_amd import _lib
    from quick_amd.build import FORCEZERO_LIB
    other = _lib.load_other(FORCEZERO_LIB)
    cos_np, sin_np, cos, sin = tables
    st = torch.cuda.current_stream().cuda_stream
    P, MP = 32, TR // 32
    for nh, nkv in GW.DEC_HEADS:
        B, p = 2, 175
        qkv, _, _, _, _, table, kp, vp = decode_case(B, nh, nkv, P, p, nh + nkv, device, cos_np, sin_np)
        pos = _pos(p, device)
        got = []
        for lib in (_lib.load(), _lib.load(), other):
            k1, v1 = kp.clone(), vp.clone()
            out = torch.empty(B, nh * D, dtype=torch.float16, device=device)
            rc = lib.quick_decode_rope_attention_paged_f16(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), k1.data_ptr(),
                                                           v1.data_ptr(), out.data_ptr(), table.data_ptr(), B, nh, nkv, D, NPAGES, P, MP, TR,
                                                           SCALE, 0, st)
            assert rc == 0, rc
            torch.cuda.synchronize()
            got.append((out, k1, v1))
        for run in got[1:]:
            for a, b in zip(got[0], run):
                assert torch.equal(_i16(a), _i16(b)), (nh, nkv, "decode: launches / forcezero build differ")
    B, nh, nkv, T = 2, 8, 2, 17
    qkv = torch.randn(B * T, (nh + 2 * nkv) * D, generator=torch.Generator(device=device).manual_seed(3), device=device).half()
    pos = _pos(20, device)
    table = scrambled_table([20 + T] * B, P, device)
    got = []
    for lib in (_lib.load(), _lib.load(), other):
        k1, v1 = poison_pool(nkv, P, device)
        q1 = torch.empty(B, nh, T, D, dtype=torch.float16, device=device)
        rc = lib.quick_rope_kv_write_paged_f16(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), pos.data_ptr(), q1.data_ptr(), k1.data_ptr(),
                                               v1.data_ptr(), table.data_ptr(), B, T, nh, nkv, D, NPAGES, P, MP, TR, 0, st)
        assert rc == 0, rc
        torch.cuda.synchronize()
        got.append((q1, k1, v1))
    for run in got[1:]:
        for a, b in zip(got[0], run):
            assert torch.equal(_i16(a), _i16(b)), "write: launches / forcezero build differ"
    for (nh, nkv), (p0, T) in zip(PF.HEADS, PF_CASES[1:]):
        q, _, _, table, kp, vp = prefill_case(2, nh, nkv, P, p0, T, "random", device)
        a = prefill_launch(K_, q, kp, vp, table, P, _pos(p0, device), nh, nkv)
        b = prefill_launch(K_, q, kp, vp, table, P, _pos(p0, device), nh, nkv)
        z = prefill_launch(K_, q, kp, vp, table, P, _pos(p0, device), nh, nkv, lib=other)
        assert PF._bits_equal(a, b), (nh, nkv, p0, T, "two launches differ")
        assert PF._bits_equal(a, z), (nh, nkv, p0, T, "the forcezero build differs")


# ------------------------------------------------------------------------------------------------
# the module
# ------------------------------------------------------------------------------------------------
MAXLEN, PM = GW.MAXLEN, 32
assert MAXLEN == 256


def _modules(hidden, nh, nkv, device, per_sequence, monkeypatch, num_pages=16):
    """The paged module, the default module and a windowed module that never wraps (sliding_window = max_seq_len: the grouped sweep over
    a linear cache), with the same weights; and the input stream."""
    mp, _, x = GW._module(hidden, nh, nkv, device, per_sequence, monkeypatch, page_size=PM, num_pages=num_pages)
    md, _, _ = GW._module(hidden, nh, nkv, device, per_sequence, monkeypatch)
    mw, _, _ = GW._module(hidden, nh, nkv, device, per_sequence, monkeypatch, sliding_window=MAXLEN)
    assert tuple(mw.k_cache.shape) == (2, nkv, MAXLEN, D) and tuple(mp.k_pool.shape) == (num_pages, nkv, PM, D)
    assert tuple(mp.block_table.shape) == (2, MAXLEN // PM) and bool((mp.block_table == -1).all()) and mp.free_pages == num_pages
    return mp, md, mw, x


@pytest.mark.parametrize("per_sequence", [False, True], ids=["shared", "per-sequence"])
@pytest.mark.parametrize("hidden,nh,nkv", [(512, 4, 4), (512, 4, 2)], ids=["group1", "group2"])
def test_paged_module_stage_by_stage(device, monkeypatch, hidden, nh, nkv, per_sequence):
    """page_size = 32, 16 pages, max_seq_len = 256.  A 40-token prefill, a ragged 17-token chunk, 16 decode steps (both sequences cross
    position 64 into a third page), then slot 1 ends (per-sequence: reset(slots=[1]); shared: reset()) and a new 33-token request reuses
    the freed pages, and three more steps.  Every T > 1 step equals the default module bit for bit, every T = 1 step the never-wrapping
    windowed module (the same sweep); after every step the gathered pools equal both modules' caches bit for bit over every sequence's
    length, and free_pages = num_pages - sum of ceil(length / 32)."""
    mp, md, mw, x = _modules(hidden, nh, nkv, device, per_sequence, monkeypatch)
    B, N = 2, mp.num_pages
    table_at = mp.block_table.data_ptr()
    length = [0] * B
    at = 0

    def step(T, counts=None):
        nonlocal at
        counts = [T] * B if counts is None else counts
        kw = dict(new_tokens=counts) if per_sequence else {}
        xs = x[:, at:at + T].contiguous()
        got, want_d, want_w = mp(xs, **kw), md(xs, **kw), mw(xs, **kw)
        torch.cuda.synchronize()
        want = want_w if T == 1 else want_d
        for b in range(B):
            n = counts[b]
            for i in (0, 1):                                       # attn_output, and the attention in front of o_proj
                assert PF._bits_equal(got[i][b, :n], want[i][b, :n]), (T, b, i, "differs from the linear module")
            length[b] += n
            for m in (md, mw):
                assert torch.equal(_i16(gather_pages(mp.k_pool, mp.block_table[b], length[b])), _i16(m.k_cache[b][:, :length[b]])), (T, b, "K")
                assert torch.equal(_i16(gather_pages(mp.v_pool, mp.block_table[b], length[b])), _i16(m.v_cache[b][:, :length[b]])), (T, b, "V")
        assert mp.free_pages == N - sum(-(-n // PM) for n in length), (T, length, mp.free_pages)
        assert [int((r >= 0).sum()) for r in mp.block_table] == [-(-n // PM) for n in length]
        assert mp.pos.tolist() == md.pos.tolist() and mp.start_pos == md.start_pos and mp.block_table.data_ptr() == table_at
        at += T

    step(40)
    step(17, [17, 9] if per_sequence else None)
    for _ in range(16):
        step(1)
    assert min(length) > 64 and mp.free_pages == N - 6
    held = mp.block_table[1][:3].tolist()
    if per_sequence:
        for m in (mp, md, mw):
            m.reset(slots=[1])
        length[1] = 0
        assert mp.free_pages == N - 3 and bool((mp.block_table[1] == -1).all()) and int((mp.block_table[0] >= 0).sum()) == 3
        step(33, [0, 33])
        assert set(mp.block_table[1][:2].tolist()) <= set(held), "the freed pages were not reused"
    else:
        for m in (mp, md, mw):
            m.reset()
        length[:] = [0, 0]
        assert mp.free_pages == N and bool((mp.block_table == -1).all())
        step(33)
    for _ in range(3):
        step(1)


def test_a_captured_decode_step_replays_across_a_page_boundary(device, monkeypatch):
    """A decode step captured after reserve, replayed at positions 62, 63 and 64 with reserve called between the replays (the table is
    updated in place, outside the graph): every replay equals the eager step of a second module, bit for bit, and so do the pools."""
    nh, nkv = 4, 2
    mp, _, x = GW._module(512, nh, nkv, device, False, monkeypatch, page_size=PM, num_pages=16)
    eager = GW._module(512, nh, nkv, device, False, monkeypatch, page_size=PM, num_pages=16)[0]
    for m in (mp, eager):
        m(x[:, :62].contiguous())
    want = [eager(x[:, 62 + i:63 + i].contiguous())[0].clone() for i in range(3)]
    torch.cuda.synchronize()
    assert eager.free_pages == 16 - 6 and mp.free_pages == 16 - 4
    static = x[:, 62:63].clone()
    state = (mp.pos.clone(), mp.k_pool.clone(), mp.v_pool.clone(), mp.start_pos, list(mp._len_bound))

    def restore():
        mp.pos.copy_(state[0])
        mp.k_pool.copy_(state[1])
        mp.v_pool.copy_(state[2])
        mp.start_pos, mp._len_bound = state[3], list(state[4])
    mp.reserve(64)                                         # (held already: positions 62 and 63 lie in the second page)
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        mp(static)                                         # warm-up outside the capture (workspaces)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_static = mp(static)[0]
    restore()                                              # (capture executes nothing, but advances the host-side bounds)
    torch.cuda.synchronize()
    table_at = mp.block_table.data_ptr()
    for i in range(3):
        if i == 2:
            assert mp.free_pages == 16 - 4
            mp.reserve(65)                                 # position 64 opens a third page: taken between the replays
            assert mp.free_pages == 16 - 6 and mp.block_table.data_ptr() == table_at
        static.copy_(x[:, 62 + i:63 + i])
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_i16(out_static), _i16(want[i])), ("replay", i)
    assert torch.equal(mp.pos, eager.pos)
    for b in range(2):
        assert torch.equal(_i16(gather_pages(mp.k_pool, mp.block_table[b], 65)), _i16(gather_pages(eager.k_pool, eager.block_table[b], 65)))
        assert torch.equal(_i16(gather_pages(mp.v_pool, mp.block_table[b], 65)), _i16(gather_pages(eager.v_pool, eager.block_table[b], 65)))


def test_a_pool_too_small_for_the_step_raises_and_changes_nothing(device, monkeypatch):
    m, _, x = GW._module(512, 4, 2, device, True, monkeypatch, page_size=PM, num_pages=5)
    m(x[:, :40].contiguous(), new_tokens=[40, 33])        # 2 + 2 pages
    torch.cuda.synchronize()
    before = (m.block_table.clone(), m.k_pool.clone(), m.v_pool.clone(), m.pos.clone(), m.start_pos, list(m._len_bound))
    assert m.free_pages == 1
    with pytest.raises(RuntimeError, match="1 of 5 are free, 2 were asked for"):
        m(x[:, 40:72].contiguous(), new_tokens=[30, 32])  # 70 and 65 positions: a third page each, and one is free
    torch.cuda.synchronize()
    assert torch.equal(m.block_table, before[0]) and pools_equal(m.k_pool, m.v_pool, before[1], before[2]) and torch.equal(m.pos, before[3])
    assert m.free_pages == 1 and m.start_pos == before[4] and m._len_bound == before[5]
    m(x[:, 40:64].contiguous(), new_tokens=[24, 24])      # 64 and 57 positions fit the pages held
    assert m.free_pages == 1 and m.pos.tolist() == [64, 57]


def test_a_default_module_issues_the_existing_launches(device, monkeypatch):
    """page_size=None: the module calls the kernels entry points with the arguments it always passed (no block_table, no page_size, no
    table_rows) on caches [batch, nkv, max_seq_len, 128], and has no pool, table or allocator."""
    from quick_amd import kernels
    m, _, x = GW._module(512, 4, 2, device, False, monkeypatch)
    assert m.page_size is None and tuple(m.k_cache.shape) == (2, 2, MAXLEN, D) and not hasattr(m, "block_table") and not hasattr(m, "allocator")
    calls = []
    for name in ("rope_attention", "rope_kv_write", "prefill_attention"):
        real = getattr(kernels, name)
        monkeypatch.setattr(kernels, name, (lambda real, name: lambda *a, **kw: (calls.append((name, len(a), dict(kw))), real(*a, **kw))[1])(real, name))
    m(x[:, :19])
    m(x[:, 19:20])
    torch.cuda.synchronize()
    assert calls == [("rope_kv_write", 11, {}), ("prefill_attention", 8, {}), ("rope_attention", 10, {})], calls
    mp = GW._module(512, 4, 2, device, False, monkeypatch, page_size=PM, num_pages=8)[0]
    calls.clear()
    mp(x[:, :19])
    mp(x[:, 19:20])
    torch.cuda.synchronize()
    assert [c[0] for c in calls] == ["rope_kv_write", "prefill_attention", "rope_attention"]
    assert all(set(c[2]) == {"block_table", "page_size", "table_rows"} and c[2]["block_table"] is mp.block_table for c in calls), calls
