"""gate_proj + up_proj -> the interleaved layer of the silu_mul epilogue, on the GPU: the HIP interleave / split kernels against packing.py's
restatement bit for bit (inside poisoned, guarded buffers), and QuantFusedMLP against operators the suite already pins -- the silu_mul GEMM
on pack_mi355x of the interleaved logical layers, bit for bit -- and against the float64 model at the suite's 2e-3.

Kernel shapes (K, I, G): (128, 64, 128) one k tile, the smallest I; (256, 192, 64) I % 128 == 64, several groups; (384, 64, 32) twelve groups over
three k tiles; (512, 320, 128) an odd count of 64-channel halves; (4096, 11008, 128) a Llama-2-7B layer: 2.8 M weight pieces over 11 k
workgroups, the scale and zero-point sections starting far into the grid.  Module shape: H = 256, I = 384, G = 128, M in {1, 16, 64, 300}."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import exact_layer, rel_err
from oracle import w4a16
from quick_amd import QuantFusedMLP, WQLinear_GEMM, WQLinear_QUICK, kernels, packing

pytestmark = pytest.mark.gpu

TOL = 2e-3      # tests/test_gemm_gpu.py's bound
GUARD = 256     # bytes of poison kept in front of and behind every output (a multiple of 16: the pieces stay aligned)
H, I, G = 256, 384, 128
MS = [1, 16, 64, 300]


def _eq(a, b):
    """Bit equality of two tensors on one device, whatever the dtype."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    bits = torch.int16 if a.dtype == torch.float16 else a.dtype
    return torch.equal(a.contiguous().view(bits), b.contiguous().view(bits))


def _guarded(shape, dtype, device, poison):
    """A tensor of `shape` inside a buffer filled with `poison`, GUARD bytes of it on either side: (tensor, whole buffer)."""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((nbytes + 2 * GUARD,), poison, dtype=torch.uint8, device=device)
    return buf[GUARD:GUARD + nbytes].view(dtype).reshape(shape), buf


def _guards_intact(buf, poison):
    return bool((buf[:GUARD] == poison).all()) and bool((buf[-GUARD:] == poison).all())


def _shapes(K, I_, NG, width):
    return (((K // 4, I_ // 2 * width), torch.int32), ((NG, 2 * I_ * width), torch.float16), ((NG, I_ // 4 * width), torch.int32))


@pytest.mark.parametrize("K,I_,G_", [(128, 64, 128), (256, 192, 64), (384, 64, 32), (512, 320, 128), (4096, 11008, 128)])
def test_kernels_equal_the_restatement_both_ways(device, K, I_, G_):
    gen = torch.Generator(device=device).manual_seed(K + I_)
    gate, up = packing.random_mi355x(K, I_, G_, device, gen), packing.random_mi355x(K, I_, G_, device, gen)
    keep = [t.clone() for t in gate + up]
    want = packing.interleave_gate_up_mi355x(gate, up)                     # torch ops on the device
    NG = K // G_
    # two poisons: a byte the kernel skipped keeps the poison, which cannot equal the expected byte both times -- this covers the zero half of
    # every qzeros row, which the expected tensors hold as 0
    for poison in (0xA5, 0x5A):
        outs = [_guarded(s, d, device, poison) for s, d in _shapes(K, I_, NG, 2)]
        got = kernels.interleave_gate_up_mi355x(gate, up, out=tuple(t for t, _ in outs))
        for i, ((t, buf), w) in enumerate(zip(outs, want)):
            assert got[i] is t and _eq(t, w), (poison, i)
            assert _guards_intact(buf, poison), (poison, i)
        outs = [[_guarded(s, d, device, poison) for s, d in _shapes(K, I_, NG, 1)] for _ in (0, 1)]
        back = kernels.split_gate_up_mi355x(*want, out=tuple(tuple(t for t, _ in o) for o in outs))
        for h, src in ((0, gate), (1, up)):
            for i, ((t, buf), w) in enumerate(zip(outs[h], src)):
                assert back[h][i] is t and _eq(t, w), (poison, h, i)
                assert _guards_intact(buf, poison), (poison, h, i)
    assert all(_eq(a, b) for a, b in zip(gate + up, keep))                # inputs untouched
    assert (want[2][:, I_ // 4:] == 0).all() and (gate[2][:, I_ // 8:] == 0).all()
    # without `out`: fresh tensors, the same bits; and the restatement's own inverse agrees with the kernel's
    assert all(_eq(a, b) for a, b in zip(kernels.interleave_gate_up_mi355x(gate, up), want))
    if K <= 512:
        cpu = packing.interleave_gate_up_mi355x(tuple(t.cpu() for t in gate), tuple(t.cpu() for t in up))
        assert all(_eq(a.cpu(), b) for a, b in zip(want, cpu))


def test_python_face_checks_what_the_library_dereferences(device):
    gate = packing.random_mi355x(128, 64, 128, device)
    with pytest.raises(RuntimeError, match="GPU tensor"):
        kernels.interleave_gate_up_mi355x(tuple(t.cpu() for t in gate), gate)
    with pytest.raises(RuntimeError, match="contiguous"):
        kernels.interleave_gate_up_mi355x((gate[0].t().contiguous().t(), gate[1], gate[2]), gate)
    with pytest.raises(RuntimeError, match="scalar type"):
        kernels.interleave_gate_up_mi355x((gate[0], gate[1].view(torch.int32), gate[2]), gate)
    with pytest.raises(ValueError):
        kernels.interleave_gate_up_mi355x(gate, packing.random_mi355x(256, 64, 128, device))
    with pytest.raises(ValueError):
        kernels.interleave_gate_up_mi355x(gate, gate, out=gate)
    with pytest.raises(NotImplementedError, match="multiple of 64"):
        kernels.interleave_gate_up_mi355x(*[packing.random_mi355x(128, 32, 128, device)] * 2)
    with pytest.raises(ValueError):
        kernels.split_gate_up_mi355x(gate[0], gate[1], gate[2][:, :8].contiguous())


# ---------------------------------------------------------------------------------------------- the module
_LAYERS = {}


def _logical():
    """gate, down, up of the module shape as logical (iw, s, z) torch tensors on the CPU, and the fixed activations; made once."""
    if not _LAYERS:
        for name, (K, N), seed in (("gate", (H, I), 61), ("down", (I, H), 62), ("up", (H, I), 63)):
            _LAYERS[name] = tuple(torch.from_numpy(a) for a in exact_layer(K, N, G, seed))
        g = torch.Generator().manual_seed(64)
        _LAYERS["x"] = (torch.randn(max(MS), H, generator=g) * 0.5).half()
        _LAYERS["fused"] = packing.pack_mi355x(*[packing.interleave8(a, b) for a, b in zip(_LAYERS["gate"], _LAYERS["up"])])
    return _LAYERS


def _module(kind, name, device, bias=None, logical=None):
    iw, s, z = logical or _logical()[name]
    K, N = iw.shape
    G_ = K // s.shape[0]
    if kind == "quick":
        m = WQLinear_QUICK(4, G_, K, N, bias is not None, "cpu")
        sd = dict(zip(("qweight", "scales", "qzeros"), packing.pack_cuda_order(iw, s, z)))
    else:
        m = WQLinear_GEMM(4, G_, K, N, bias is not None, "cpu")
        sd = dict(zip(("qweight", "qzeros", "scales"), packing.pack_awq_gemm(iw, s, z)))
    if bias is not None:
        sd["bias"] = bias
    m.load_state_dict(sd)
    return m.to(device)


@pytest.fixture(scope="module", params=["quick", "gemm"])
def mlp(request, device):
    gate, down, up = (_module(request.param, n, device) for n in ("gate", "down", "up"))
    return QuantFusedMLP(gate, down, up), gate, down, up


def test_module_holds_pack_mi355x_of_the_interleaved_layers_and_unfuses(device, mlp):
    m, gate, down, up = mlp
    gu = m.gate_up
    assert m.is_fused and m.silu_mul_epilogue and gu.is_prepared and gu.qweight.is_cuda and gu.out_features == 2 * I
    assert all(_eq(a.cpu(), b) for a, b in zip((gu.qweight, gu.scales, gu.qzeros), _logical()["fused"]))
    for got, src in zip(m.unfuse(), (gate, up)):
        a, b = got.state_dict(), src.state_dict()
        assert type(got) is type(src) and list(a) == list(b) and all(_eq(a[k], b[k]) for k in a)


@pytest.mark.parametrize("M", MS)
def test_module_equals_the_pinned_operators_bit_for_bit(device, mlp, M):
    m, _, down, _ = mlp
    x = _logical()["x"][:M].to(device)
    act = kernels.gemm_forward(x, *[t.to(device) for t in _logical()["fused"]], silu_mul=True)
    y = m(x)
    assert y.dtype == torch.float16 and tuple(y.shape) == (M, H)
    assert _eq(y, down(act))


@pytest.mark.parametrize("M", MS)
def test_fused_activation_against_the_float64_model(device, mlp, M):
    m = mlp[0]
    L = _logical()
    x = L["x"][:M]
    gu = m.gate_up
    act = kernels.gemm_forward(x.to(device), gu.qweight, gu.scales, gu.qzeros, silu_mul=True)
    x64 = x.double().numpy()
    pre = [x64 @ w4a16.dequantize(*[t.numpy() for t in L[n]], G).astype(np.float64) for n in ("gate", "up")]
    want = pre[0] / (1.0 + np.exp(-pre[0])) * pre[1]
    err = rel_err(act.float().cpu().numpy(), want)
    print(f"M={M}: silu(gate) * up rel_err {err:.3e}")
    assert tuple(act.shape) == (M, I) and err <= TOL


def test_other_activation_and_biased_pair_run_the_plain_fused_gemm(device, mlp):
    _, gate, down, up = mlp
    L = _logical()
    x = L["x"][:16].to(device)
    fused = [t.to(device) for t in L["fused"]]
    # another activation: torch's own gelu(gate) * up on the plain 2I-wide GEMM's output, then down
    m = QuantFusedMLP(gate, down, up, activation=F.gelu)
    assert m.is_fused and not m.silu_mul_epilogue
    v = kernels.gemm_forward(x, *fused).view(16, I // 8, 2, 8)
    gate_y, up_y = v[:, :, 0], v[:, :, 1]                               # (torch works on the [M, I / 8, 2, 8] view, as the module does)
    assert _eq(m(x), down((F.gelu(gate_y) * up_y).reshape(16, I)))
    gate_y, up_y = gate_y.reshape(16, I), up_y.reshape(16, I)
    # the channel order is the one the separate projections compute: gate_y / up_y against two GEMMs (other launches: within the bound)
    assert rel_err(gate_y.float().cpu().numpy(), gate(x).float().cpu().numpy()) <= TOL
    assert rel_err(up_y.float().cpu().numpy(), up(x).float().cpu().numpy()) <= TOL
    # a biased pair: the interleaved bias goes into the plain GEMM, silu in torch
    kind = "gemm" if isinstance(gate, WQLinear_GEMM) else "quick"
    bg, bu = (torch.arange(I, dtype=torch.float32) / I - 0.5).half(), (0.25 - torch.arange(I, dtype=torch.float32) / I).half()
    mb = QuantFusedMLP(_module(kind, "gate", device, bias=bg), down, _module(kind, "up", device, bias=bu))
    assert mb.is_fused and not mb.silu_mul_epilogue
    v = kernels.gemm_forward(x, *fused, bias=packing.interleave8(bg, bu).to(device)).view(16, I // 8, 2, 8)
    assert _eq(mb(x), down((F.silu(v[:, :, 0]) * v[:, :, 1]).reshape(16, I)))


def test_routing_weights_and_leading_dimensions(device, mlp):
    m = mlp[0]
    x = _logical()["x"][:16].to(device)
    y = m(x)
    rw = (torch.arange(16, dtype=torch.float32) / 16).half().reshape(16, 1).to(device)
    assert _eq(m(x, routing_weights=rw), rw * y)
    y3 = m(x.reshape(2, 8, H))
    assert tuple(y3.shape) == (2, 8, H) and _eq(y3.reshape(16, H), y)


@pytest.mark.parametrize("kind", ["quick", "gemm"])
def test_pair_that_cannot_be_fused_runs_as_two_projections(device, kind):
    """in_features = 192 with G = 64 (K % 128 != 0: the projections run on padded copies and have no MI355X order to interleave): the module
    keeps gate_proj and up_proj and runs the reference's two GEMMs.  Bit-equal to the same two launches made by hand, and within the suite's
    bound of the float64 model.  (A pair of 192 OUTPUT channels, whose down_proj would have in_features % 128 != 0, cannot be built into
    runnable modules at all: every GEMM, and both checkpoint bridges, need a multiple of 128 channels per layer.  Such a pair is constructed
    -- tests/test_gate_up_cpu.py -- but has no forward; in_features = 192 is the padded layer an MLP can have.)"""
    K, I_, G_, M = 192, 256, 64, 16
    lg, lu, ld = (tuple(torch.from_numpy(a) for a in exact_layer(k, n, G_, seed)) for k, n, seed in ((K, I_, 71), (K, I_, 72), (I_, 256, 73)))
    gate, up, down = (_module(kind, None, device, logical=l) for l in (lg, lu, ld))
    m = QuantFusedMLP(gate, down, up)
    assert not m.is_fused and m.gate_up is None
    x = (torch.randn(M, K, generator=torch.Generator().manual_seed(74)) * 0.5).half()
    xd = x.to(device)
    act = F.silu(gate(xd)) * up(xd)
    assert _eq(m(xd), down(act))
    pre = [x.double().numpy() @ w4a16.dequantize(*[t.numpy() for t in l], G_).astype(np.float64) for l in (lg, lu)]
    g16, u16 = (p.astype(np.float16).astype(np.float64) for p in pre)         # each projection rounds its output to fp16 before torch multiplies
    err = rel_err(act.float().cpu().numpy(), g16 / (1.0 + np.exp(-g16)) * u16)
    print(f"{kind}: two projections, silu(gate) * up rel_err {err:.3e}")
    assert err <= TOL
