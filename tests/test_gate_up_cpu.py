"""gate_proj + up_proj -> the interleaved layer of the GEMM's silu_mul epilogue, host side: packing.py's packed-space restatement against
pack_mi355x of the interleaved logical layers, fuse_gate_up / split_gate_up on CPU modules of both checkpoint formats (the golden
quick_cat fixture), the shape rules of the two C entry points, and QuantFusedMLP's construction.  No GPU needed, no forward.

(K, I, G) cases: (128, 64, 128) one k tile and the smallest I; (256, 192, 64) I % 128 == 64, several groups; (384, 64, 32) twelve groups over
three k tiles; (512, 320, 128) an odd count of 64-channel halves; (256, 384, 128) the module's shape."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN_DIR, exact_layer, load_golden
from quick_amd import QuantFusedMLP, QuantLlamaMLP, WQLinear_GEMM, WQLinear_QUICK, _lib, fuse_gate_up, packing, split_gate_up

CASES = [(128, 64, 128), (256, 192, 64), (384, 64, 32), (512, 320, 128), (256, 384, 128)]


def _bits(t):
    return np.ascontiguousarray(t.numpy()).view(np.uint8)


def _same(got, want):
    got, want = tuple(got), tuple(want)
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.dtype == b.dtype, (i, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(_bits(a), _bits(b)), i


def _layer(K, N, G, seed):
    return tuple(torch.from_numpy(a) for a in exact_layer(K, N, G, seed))


def _pack_mi355x_any_width(iw, s, z):
    """pack_mi355x without its N % 128 rule (one projection of I % 128 == 64 channels), from packing.py's position helpers."""
    K, N = iw.shape
    NG = s.shape[0]
    idx, nib = packing._mi355x_weight_pos(K, N, iw.device)
    qweight = packing._scatter_nibbles(K * N // 8, idx, nib, iw).reshape(K // 4, N // 2)
    words = torch.zeros(NG * N, dtype=torch.int64)
    sbits = s.contiguous().view(torch.int16).to(torch.int64) & 0xffff
    words[packing._mi355x_group_word_pos(NG, N, iw.device).reshape(-1)] = (sbits | ((z.to(torch.int64) & 15) << 16)).reshape(-1)
    qscales = packing._to_i32(words).view(torch.float16).reshape(NG, 2 * N)
    qz = torch.zeros((NG, N // 4), dtype=torch.int64)
    n = torch.arange(N)
    qz.scatter_add_(1, (n // 8)[None, :].expand(NG, N), (z.to(torch.int64) & 15) << (4 * (n % 8))[None, :])
    return qweight, qscales, packing._to_i32(qz)


def test_interleave8_is_blocks_of_eight():
    a, b = torch.arange(16), torch.arange(100, 116)
    assert packing.interleave8(a, b).tolist() == list(range(8)) + list(range(100, 108)) + list(range(8, 16)) + list(range(108, 116))
    assert packing.interleave8(a.reshape(2, 8), b.reshape(2, 8)).shape == (2, 16)
    with pytest.raises(ValueError):
        packing.interleave8(torch.arange(12), torch.arange(12))


def test_any_width_packer_is_pack_mi355x():
    layer = _layer(256, 128, 64, 3)
    _same(_pack_mi355x_any_width(*layer), packing.pack_mi355x(*layer))


@pytest.mark.parametrize("K,I,G", CASES)
def test_restatement_equals_pack_mi355x_of_the_interleaved_layers(K, I, G):
    gate, up = _layer(K, I, G, 11), _layer(K, I, G, 12)
    pg, pu = _pack_mi355x_any_width(*gate), _pack_mi355x_any_width(*up)
    keep = [t.clone() for t in pg + pu]
    fused = packing.interleave_gate_up_mi355x(pg, pu)
    _same(fused, packing.pack_mi355x(*[packing.interleave8(a, b) for a, b in zip(gate, up)]))
    back = packing.split_gate_up_mi355x(*fused)
    _same(back[0], pg)
    _same(back[1], pu)
    _same(pg + pu, keep)                                      # inputs untouched
    assert all(t.is_contiguous() for t in fused + back[0] + back[1])


def test_restatement_refuses_shapes_outside_the_envelope():
    pg = _pack_mi355x_any_width(*_layer(128, 32, 128, 1))
    with pytest.raises(ValueError, match="multiple of 64"):
        packing.interleave_gate_up_mi355x(pg, pg)
    pg = _pack_mi355x_any_width(*_layer(128, 64, 128, 1))
    with pytest.raises(ValueError):
        packing.interleave_gate_up_mi355x(pg, (pg[0], pg[1][:, :64], pg[2]))


# ---------------------------------------------------------------------------------------------- modules on the golden fixture
@pytest.fixture(scope="module")
def cat():
    g = load_golden(os.path.join(GOLDEN_DIR, "quick_cat_k128n256g64.npz"))
    quick = [tuple(torch.from_numpy(g[f"in{i}_{n}"]) for n in ("qweight", "scales", "qzeros")) for i in (0, 1)]
    logical = [packing.unpack_cuda_order(*q) for q in quick]
    want = packing.pack_mi355x(*[packing.interleave8(a, b) for a, b in zip(*logical)])
    return {"K": int(g["K"]), "I": int(g["N"]), "G": int(g["G"]), "quick": quick, "logical": logical, "want": want,
            "gemm": [packing.pack_awq_gemm(*l) for l in logical]}


def _modules(cat, kind, bias=False, prepared=False):
    K, I, G = cat["K"], cat["I"], cat["G"]
    out = []
    for i in (0, 1):
        if kind == "quick":
            m = WQLinear_QUICK(4, G, K, I, bias, "cpu")
            sd = dict(zip(("qweight", "scales", "qzeros"), cat["quick"][i]))
        else:
            m = WQLinear_GEMM(4, G, K, I, bias, "cpu")
            sd = dict(zip(("qweight", "qzeros", "scales"), cat["gemm"][i]))
        if bias:
            sd["bias"] = (torch.arange(I, dtype=torch.float32) + 1000 * i).half()
        m.load_state_dict({k: v.clone() for k, v in sd.items()})
        out.append(m.prepare() if prepared else m)
    return out


def _sd_same(m, src):
    a, b = m.state_dict(), src.state_dict()
    assert list(a) == list(b)
    _same(a.values(), b.values())


@pytest.mark.parametrize("prepared", [False, True])
@pytest.mark.parametrize("kind", ["quick", "gemm"])
def test_fuse_gate_up_on_the_golden_fixture_and_back(cat, kind, prepared):
    assert (cat["K"], cat["I"], cat["G"]) == (128, 256, 64)
    gate, up = _modules(cat, kind, prepared=prepared)
    fused = fuse_gate_up(gate, up)
    assert isinstance(fused, WQLinear_QUICK) and fused.is_prepared and fused.bias is None
    assert (fused.in_features, fused.out_features, fused.group_size) == (128, 512, 64)
    _same((fused.qweight, fused.scales, fused.qzeros), cat["want"])
    assert gate.is_prepared == prepared and up.is_prepared == prepared          # the sources are left as they are
    src_ptrs = {t.data_ptr() for m in (gate, up) for t in (m.qweight, m.scales, m.qzeros)}
    assert not src_ptrs & {t.data_ptr() for t in (fused.qweight, fused.scales, fused.qzeros)}
    for back_kind in ("quick", "gemm"):
        g2, u2 = split_gate_up(fused, back_kind)
        assert type(g2) is (WQLinear_QUICK if back_kind == "quick" else WQLinear_GEMM) and g2.out_features == 256
        for m, src in ((g2, 0), (u2, 1)):
            sd = m.state_dict()
            if back_kind == "quick":
                _same((sd["qweight"], sd["scales"], sd["qzeros"]), cat["quick"][src])
            else:
                _same((sd["qweight"], sd["qzeros"], sd["scales"]), cat["gemm"][src])
    # the fused layer's own checkpoint is the reference-order packing of the interleaved layer, and loads back
    sd = fused.state_dict()
    _same((sd["qweight"], sd["scales"], sd["qzeros"]), packing.pack_cuda_order(*[packing.interleave8(a, b) for a, b in zip(*cat["logical"])]))
    again = WQLinear_QUICK(4, 64, 128, 512, False, "cpu")
    again.load_state_dict(sd)
    _sd_same(split_gate_up(again, kind)[1], up)


@pytest.mark.parametrize("kind", ["quick", "gemm"])
def test_fuse_gate_up_interleaves_biases_and_split_returns_them(cat, kind):
    gate, up = _modules(cat, kind, bias=True)
    fused = fuse_gate_up(gate, up)
    assert torch.equal(fused.bias, packing.interleave8(gate.bias, up.bias)) and "bias" in fused.state_dict()
    assert fused.bias.data_ptr() not in (gate.bias.data_ptr(), up.bias.data_ptr())
    g2, u2 = split_gate_up(fused, kind)
    _sd_same(g2, gate)
    _sd_same(u2, up)


def test_fuse_gate_up_refusals(cat):
    gate, up = _modules(cat, "quick")
    K, I, G = cat["K"], cat["I"], cat["G"]
    for other in (WQLinear_QUICK(4, G, 2 * K, I, False, "cpu"), WQLinear_QUICK(4, G, K, 2 * I, False, "cpu"),
                  WQLinear_QUICK(4, 32, K, I, False, "cpu"), WQLinear_QUICK(4, G, K, I, True, "cpu")):
        with pytest.raises(ValueError, match="differ"):
            fuse_gate_up(gate, other)
    with pytest.raises(TypeError):
        fuse_gate_up(gate, torch.nn.Linear(K, I))
    # in_features % 128 != 0: the library's sentence
    a, b = WQLinear_QUICK(4, 64, 192, 128, False, "cpu"), WQLinear_QUICK(4, 64, 192, 128, False, "cpu")
    with pytest.raises(NotImplementedError, match=r"quick_interleave_gate_up_mi355x: in_features must be a multiple of 128.*K=192 I=128 G=64"):
        fuse_gate_up(a, b)
    # I % 64 != 0: the library's sentence; I % 128 == 64: inside the kernels' envelope, but no such projection has an MI355X order of its own
    a, b = WQLinear_GEMM(4, 128, 128, 96, False, "cpu"), WQLinear_GEMM(4, 128, 128, 96, False, "cpu")
    with pytest.raises(NotImplementedError, match=r"intermediate size must be a multiple of 64.*K=128 I=96 G=128"):
        fuse_gate_up(a, b)
    a, b = WQLinear_GEMM(4, 64, 256, 192, False, "cpu"), WQLinear_GEMM(4, 64, 256, 192, False, "cpu")
    with pytest.raises(NotImplementedError, match="192 output channels"):
        fuse_gate_up(a, b)
    with pytest.raises(ValueError, match="kind"):
        split_gate_up(fuse_gate_up(gate, up), "gemv")


# ---------------------------------------------------------------------------------------------- C ABI
def test_both_entry_points_are_exported():
    assert "quick_interleave_gate_up_mi355x" in _lib.EXPORTS and "quick_split_gate_up_mi355x" in _lib.EXPORTS
    assert _lib.load().quick_amd_abi_version() == 1


@pytest.mark.parametrize("K,I,G,want,why", [
    (0, 64, 128, 1, "non-positive"), (128, -64, 128, 1, "non-positive"), (128, 64, 0, 1, "non-positive"),
    (128, 64, 48, 1, "multiple of 32"), (256, 64, 96, 1, "group size"), (128, 60, 128, 1, "pack_num"),
    (64, 64, 64, 4, "multiple of 128"), (192, 128, 64, 4, "multiple of 128"), (128, 32, 128, 4, "multiple of 64"),
    (128, 72, 128, 4, "multiple of 64"), (200, 64, 100, 1, "multiple of 32")])
def test_c_abi_answers_the_shape_rules_before_any_gpu_work(K, I, G, want, why):
    """Null pointers, no GPU: every rule of include/quick_amd.h, in both directions."""
    lib = _lib.load()
    for fn in (lib.quick_interleave_gate_up_mi355x, lib.quick_split_gate_up_mi355x):
        assert fn(*([None] * 9), K, I, G, None) == want
        assert why in _lib.last_error() and f"K={K} I={I} G={G}" in _lib.last_error()


@pytest.mark.parametrize("K,I,G", CASES + [(8192, 28672, 128)])
def test_c_abi_refuses_null_pointers_of_a_good_shape(K, I, G):
    lib = _lib.load()
    for fn, name in ((lib.quick_interleave_gate_up_mi355x, "quick_interleave_gate_up_mi355x"), (lib.quick_split_gate_up_mi355x, "quick_split_gate_up_mi355x")):
        assert fn(*([None] * 9), K, I, G, None) == 1
        assert _lib.last_error() == f"{name}: null tensor pointer"


# ---------------------------------------------------------------------------------------------- QuantFusedMLP, construction only
def _mlp_modules(kind, H, I, G, bias=False):
    mods = []
    for seed, (K, N) in enumerate(((H, I), (I, H), (H, I))):       # gate, down, up
        iw, s, z = _layer(K, N, G, 30 + seed)
        if kind == "quick":
            m = WQLinear_QUICK(4, G, K, N, bias, "cpu")
            sd = dict(zip(("qweight", "scales", "qzeros"), packing.pack_cuda_order(iw, s, z)))
        else:
            m = WQLinear_GEMM(4, G, K, N, bias, "cpu")
            sd = dict(zip(("qweight", "qzeros", "scales"), packing.pack_awq_gemm(iw, s, z)))
        if bias:
            sd["bias"] = torch.arange(N, dtype=torch.float16)
        m.load_state_dict(sd)
        mods.append(m)
    return mods


@pytest.mark.parametrize("kind", ["quick", "gemm"])
def test_quant_fused_mlp_attributes_children_and_unfuse(kind):
    H, I, G = CASES[-1]
    gate, down, up = _mlp_modules(kind, H, I, G)
    m = QuantFusedMLP(gate, down, up)
    assert (m.in_features, m.intermediate_size, m.out_features, m.w_bit) == (H, I, H, 4)
    assert [n for n, _ in m.named_children()] == ["gate_up", "down_proj"] and m.down_proj is down
    assert m.is_fused and m.silu_mul_epilogue and m.activation is F.silu
    assert isinstance(m.gate_up, WQLinear_QUICK) and m.gate_up.is_prepared and m.gate_up.out_features == 2 * I
    g2, u2 = m.unfuse()
    assert type(g2) is type(gate)
    _sd_same(g2, gate)
    _sd_same(u2, up)
    other = "gemm" if kind == "quick" else "quick"
    assert type(m.unfuse(other)[0]) is not type(gate)
    assert not QuantFusedMLP(gate, down, up, activation=F.gelu).silu_mul_epilogue
    alias = QuantLlamaMLP(gate, down, up)
    assert isinstance(alias, QuantFusedMLP) and alias.silu_mul_epilogue


def test_quant_fused_mlp_biased_pair_takes_the_plain_gemm_path():
    H, I, G = CASES[-1]
    gate, down, up = _mlp_modules("quick", H, I, G, bias=True)
    m = QuantFusedMLP(gate, down, up)
    assert m.is_fused and not m.silu_mul_epilogue
    assert torch.equal(m.gate_up.bias, packing.interleave8(gate.bias, up.bias))


def test_quant_fused_mlp_mismatched_sources_raise():
    H, I, G = CASES[-1]
    gate, down, up = _mlp_modules("quick", H, I, G)
    with pytest.raises(ValueError, match="differ"):
        QuantFusedMLP(gate, down, WQLinear_QUICK(4, G, H, 2 * I, False, "cpu"))
    with pytest.raises(ValueError, match="differ"):
        QuantFusedMLP(gate, down, _mlp_modules("quick", H, I, G, bias=True)[2])


@pytest.mark.parametrize("kind,H,I,G", [("quick", 192, 128, 64), ("gemm", 192, 128, 64), ("gemm", 256, 192, 64)])
def test_quant_fused_mlp_keeps_two_projections_where_the_pair_cannot_be_fused(kind, H, I, G):
    """in_features % 128 != 0 (a padded layer), or a projection width no packing of ours holds alone: construction does not fail."""
    gate, up = [WQLinear_QUICK(4, G, H, I, False, "cpu") if kind == "quick" else WQLinear_GEMM(4, G, H, I, False, "cpu") for _ in (0, 1)]
    down = WQLinear_QUICK(4, G, 256, 256, False, "cpu")
    m = QuantFusedMLP(gate, down, up)
    assert not m.is_fused and not m.silu_mul_epilogue and m.gate_up is None
    assert [n for n, _ in m.named_children()] == ["gate_proj", "up_proj", "down_proj"]
    assert m.unfuse() == (gate, up) and (m.in_features, m.intermediate_size, m.out_features) == (H, I, 256)
