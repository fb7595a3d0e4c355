"""Host-side packing for WQLinear_QUICK (torch ops, any device).

Counterpart of the Python-loop packer in the reference's ``WQLinear_QUICK.from_linear``
(quick/awq/modules/linear/quick.py:76-150), vectorised, and extended with the MI355X order that
the gfx950 kernels consume.  Logical tensors:

    iw [K, N] int (0..15)     s [K/G, N] fp16     z [K/G, N] int (0..15)

"cuda order"   = byte-for-byte the reference's packed tensors / checkpoint format.
"awq gemm"     = the packing of the reference's WQLinear_GEMM (gemm.py:29-63, 108-143), which published AWQ checkpoints
                 use: qweight int32 [K, N/8] and qzeros int32 [K/G, N/8] with nibble i of dword c = channel
                 8c + [0,2,4,6,1,3,5,7][i], scales fp16 [K/G, N] plain.  Tensor order: (qweight, qzeros, scales).
"mi355x order" = same shapes and dtypes, elements permuted for the v_mfma_f32_16x16x32_f16 A-operand
                 fragment (DESIGN.md "Data layout"): tile (n/16, k/128) is 1 KiB contiguous, lane
                 (n%16) + 16*((k%32)/8) owns 16 bytes = the dwords of 4 consecutive k-steps, and inside
                 a dword k-offset j sits at nibble 4*(j%2) + j/2.
"""
import torch

__all__ = ["quantize_intweight", "pack_cuda_order", "unpack_cuda_order", "pack_mi355x", "unpack_mi355x",
           "cuda_to_mi355x", "mi355x_to_cuda", "pack_awq_gemm", "unpack_awq_gemm", "awq_gemm_to_mi355x", "mi355x_to_awq_gemm",
           "awq_gemm_to_cuda_order", "padded_in_features", "interleave8", "interleave_gate_up_mi355x", "split_gate_up_mi355x"]


def quantize_intweight(weight, scales, zeros, group_size):
    """[N, K] fp16 weight + [N, K/G] scales/zeros -> integer weights [K, N] (quick.py:67-81, same fp16
    arithmetic: round((W + z*s) / s)), done for all columns at once instead of one column per Python step."""
    scales = scales.to(torch.float16)
    scale_zeros = (zeros * scales).to(weight.dtype)
    s_full = scales.repeat_interleave(group_size, dim=1)
    q = (weight + scale_zeros.repeat_interleave(group_size, dim=1)) / s_full
    return torch.round(q).to(torch.int32).t().contiguous()


def _arange(n, dev):
    return torch.arange(n, device=dev, dtype=torch.int64)


def _cuda_weight_pos(K, N, dev):
    k = _arange(K, dev)[:, None]
    n = _arange(N, dev)[None, :]
    kt, half, r = k // 32, (k % 32) // 16, k % 16
    l4, hi, odd = (r % 8) // 2, r // 8, r % 2
    bx, ty, chunk, t, j = n // 128, (n // 64) % 2, (n % 64) // 16, (n % 16) // 8, n % 8
    idx = kt * (4 * N) + ((2 * ty + j // 4) * (N // 8) + 16 * bx + 4 * (j % 4) + l4) * 8 + 4 * half + chunk
    nib = 4 * odd + hi + 2 * t
    return idx.expand(K, N), nib.expand(K, N)


def _cuda_slot(N, dev):
    n = _arange(N, dev)
    bx, ty, chunk, t, j = n // 128, (n // 64) % 2, (n % 64) // 16, (n % 16) // 8, n % 8
    return ((2 * ty + j // 4) * (N // 32) + 4 * bx + (j % 4)) * 8 + 2 * chunk + t


def _mi355x_weight_pos(K, N, dev):
    k = _arange(K, dev)[:, None]
    n = _arange(N, dev)[None, :]
    lane = (n % 16) + 16 * ((k % 32) // 8)
    idx = (((n // 16) * (K // 128) + k // 128) * 64 + lane) * 4 + (k % 128) // 32
    j = k % 8
    nib = 4 * (j % 2) + j // 2
    return idx.expand(K, N), nib.expand(K, N)


def _scatter_nibbles(numel, idx, nib, val):
    """OR 4-bit values into a flat int64 accumulator (every nibble slot is hit exactly once, so add == or)."""
    out = torch.zeros(numel, dtype=torch.int64, device=val.device)
    out.scatter_add_(0, idx.reshape(-1), (val.reshape(-1).to(torch.int64) & 15) << (4 * nib.reshape(-1)))
    return _to_i32(out)


def _to_i32(x64):
    return torch.where(x64 >= 2 ** 31, x64 - 2 ** 32, x64).to(torch.int32)


def _as_u32(x32):
    return x32.to(torch.int64) & 0xFFFFFFFF


def _check(K, N, mi355x):
    if N % 128 != 0:
        raise ValueError("OC is not multiple of cta_N = 128")
    if K % 32 != 0:
        raise ValueError("in_features must be a multiple of 32")
    if mi355x and K % 128 != 0:
        raise ValueError("in_features must be a multiple of 128 for the MI355X weight order")


def pack_cuda_order(iw, s, z):
    """-> (qweight int32 [K/4, N/2], scales fp16 [K/G, 2N], qzeros int32 [K/G, N/4]), reference order."""
    K, N = iw.shape
    _check(K, N, False)
    dev = iw.device
    idx, nib = _cuda_weight_pos(K, N, dev)
    qweight = _scatter_nibbles(K * N // 8, idx, nib, iw).reshape(K // 4, N // 2)
    x = _cuda_slot(N, dev)
    NG = s.shape[0]
    qscales = torch.zeros((NG, 2 * N), dtype=torch.float16, device=dev)
    qscales[:, 2 * x] = s.to(torch.float16)
    qscales[:, 2 * x + 1] = s.to(torch.float16)
    zz = z.to(torch.int64) & 15
    qz = torch.zeros((NG, N // 4), dtype=torch.int64, device=dev)
    col = (x // 4)[None, :].expand(NG, N)
    qz.scatter_add_(1, col, (zz << (4 * (x % 4))[None, :]) | (zz << (4 * (x % 4) + 16)[None, :]))
    return qweight, qscales, _to_i32(qz)


def unpack_cuda_order(qweight, qscales, qzeros):
    K, N = qweight.shape[0] * 4, qweight.shape[1] * 2
    _check(K, N, False)
    dev = qweight.device
    idx, nib = _cuda_weight_pos(K, N, dev)
    flat = _as_u32(qweight.reshape(-1))
    iw = ((flat[idx] >> (4 * nib)) & 15).to(torch.uint8)
    x = _cuda_slot(N, dev)
    s = qscales[:, 2 * x].contiguous()
    z = ((_as_u32(qzeros)[:, x // 4] >> (4 * (x % 4))[None, :]) & 15).to(torch.uint8)
    return iw, s, z


def _mi355x_group_word_pos(NG, N, dev):
    """32-bit word of the (scale, zero point) pair of (g, n) in the scales tensor viewed as int32 [NG * N]."""
    g = _arange(NG, dev)[:, None]
    n = _arange(N, dev)[None, :]
    return ((n // 16) * NG + g) * 16 + (n % 16)


def pack_mi355x(iw, s, z):
    """-> (qweight, scales, qzeros) in MI355X order (same shapes / dtypes as the reference buffers).  The scales tensor
    carries one 32-bit word per (group, channel) -- fp16 scale | zero point << 16 -- block-contiguous along K; qzeros
    keeps a plain copy of the zero points that the GEMM kernels do not read (oracle/w4a16.py::pack_mi355x)."""
    K, N = iw.shape
    _check(K, N, True)
    dev = iw.device
    idx, nib = _mi355x_weight_pos(K, N, dev)
    qweight = _scatter_nibbles(K * N // 8, idx, nib, iw).reshape(K // 4, N // 2)
    NG = s.shape[0]
    sbits = s.to(torch.float16).contiguous().view(torch.int16).to(torch.int64) & 0xffff
    words = torch.zeros(NG * N, dtype=torch.int64, device=dev)
    words[_mi355x_group_word_pos(NG, N, dev).reshape(-1)] = (sbits | ((z.to(torch.int64) & 15) << 16)).reshape(-1)
    qscales = _to_i32(words).view(torch.float16).reshape(NG, 2 * N)
    n = _arange(N, dev)
    qz = torch.zeros((NG, N // 4), dtype=torch.int64, device=dev)
    qz.scatter_add_(1, (n // 8)[None, :].expand(NG, N), (z.to(torch.int64) & 15) << (4 * (n % 8))[None, :])
    return qweight, qscales, _to_i32(qz)


def unpack_mi355x(qweight, qscales, qzeros):
    K, N = qweight.shape[0] * 4, qweight.shape[1] * 2
    _check(K, N, True)
    dev = qweight.device
    idx, nib = _mi355x_weight_pos(K, N, dev)
    flat = _as_u32(qweight.reshape(-1))
    iw = ((flat[idx] >> (4 * nib)) & 15).to(torch.uint8)
    NG = qscales.shape[0]
    words = _as_u32(qscales.contiguous().view(torch.int32).reshape(-1))[_mi355x_group_word_pos(NG, N, dev)]
    s = (words & 0xffff).to(torch.int32).to(torch.int16).view(torch.float16)
    z = ((words >> 16) & 15).to(torch.uint8)
    return iw, s, z


def random_mi355x(K, N, G, device, generator=None, zero_point=None, scale_lo=0.005, scale_span=0.02):
    """Random packed tensors in MI355X order (benchmarks, synthetic models): uniform 4-bit weights, scales in
    [scale_lo, scale_lo + scale_span), zero points uniform in 0..15 or the given constant."""
    NG = K // G
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 4, N // 2), dtype=torch.int32, device=device, generator=generator)
    s = (torch.rand((NG, N), device=device, generator=generator) * scale_span + scale_lo).half()
    if zero_point is None:
        z = torch.randint(0, 16, (NG, N), dtype=torch.int64, device=device, generator=generator)
    else:
        z = torch.full((NG, N), int(zero_point), dtype=torch.int64, device=device)
    sbits = s.view(torch.int16).to(torch.int64) & 0xffff
    words = torch.zeros(NG * N, dtype=torch.int64, device=device)
    words[_mi355x_group_word_pos(NG, N, device).reshape(-1)] = (sbits | (z << 16)).reshape(-1)
    n = _arange(N, device)
    qz = torch.zeros((NG, N // 4), dtype=torch.int64, device=device)
    qz.scatter_add_(1, (n // 8)[None, :].expand(NG, N), z << (4 * (n % 8))[None, :])
    return qw, _to_i32(words).view(torch.float16).reshape(NG, 2 * N), _to_i32(qz)


def cuda_to_mi355x(qweight, qscales, qzeros):
    """Reference-order packed tensors -> MI355X order (torch ops; the GPU path uses the HIP repack kernels)."""
    return pack_mi355x(*unpack_cuda_order(qweight, qscales, qzeros))


def mi355x_to_cuda(qweight, qscales, qzeros):
    return pack_cuda_order(*unpack_mi355x(qweight, qscales, qzeros))


# ---------------------------------------------------------------------------------------------- AWQ GEMM packing
_AWQ_ORDER = (0, 2, 4, 6, 1, 3, 5, 7)      # nibble i of a dword holds channel 8c + _AWQ_ORDER[i] (gemm.py:116)


def _pack_awq(a):
    """[R, N] 4-bit values -> int32 [R, N/8] in the AWQ nibble order."""
    R, N = a.shape
    if N % 8 != 0:
        raise ValueError("OC is not multiple of pack_num = 8")
    v = (a.to(torch.int64) & 15).reshape(R, N // 8, 8)[:, :, list(_AWQ_ORDER)]
    return _to_i32((v << (4 * _arange(8, a.device))).sum(dim=2))


def _unpack_awq(q):
    """int32 [R, N/8] -> uint8 [R, N]."""
    nib = (_as_u32(q)[:, :, None] >> (4 * _arange(8, q.device))) & 15        # [R, N/8, 8]: slot i = channel 8c + order[i]
    out = torch.empty_like(nib)
    out[:, :, list(_AWQ_ORDER)] = nib
    return out.reshape(q.shape[0], -1).to(torch.uint8)


def pack_awq_gemm(iw, s, z):
    """Logical (iw [K, N], s [K/G, N], z [K/G, N]) -> (qweight int32 [K, N/8], qzeros int32 [K/G, N/8], scales fp16 [K/G, N]),
    the packing of WQLinear_GEMM (checkpoint order of its three tensors)."""
    return _pack_awq(iw), _pack_awq(z), s.to(torch.float16).contiguous()


def unpack_awq_gemm(qweight, qzeros, scales):
    """-> logical (iw [K, N] uint8, s [K/G, N] fp16, z [K/G, N] uint8)."""
    return _unpack_awq(qweight), scales.to(torch.float16).contiguous(), _unpack_awq(qzeros)


def padded_in_features(K, G):
    """The next multiple of lcm(128, G) (quick_padded_in_features, include/quick_amd.h): the rows of the MI355X-order copy of a layer."""
    import math
    unit = 128 * G // math.gcd(128, G)
    return (K + unit - 1) // unit * unit


def _pad_rows(t, rows):
    if rows == t.shape[0]:
        return t
    return torch.cat([t, torch.zeros((rows - t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)])


def awq_gemm_to_mi355x(qweight, qzeros, scales):
    """GEMM-packing tensors -> (qweight, scales, qzeros) in MI355X order, as the HIP kernel writes them: Kp = padded_in_features(K, G)
    rows, the added rows with weight 0 and the added groups with scale 0 and zero point 0 (Kp == K when K % 128 == 0)."""
    iw, s, z = unpack_awq_gemm(qweight, qzeros, scales)
    K, N = iw.shape
    _check(K, N, False)
    G = K // s.shape[0]
    Kp = padded_in_features(K, G)
    return pack_mi355x(_pad_rows(iw, Kp), _pad_rows(s, Kp // G), _pad_rows(z, Kp // G))


def mi355x_to_awq_gemm(qweight, qscales, qzeros):
    """MI355X-order tensors -> (qweight, qzeros, scales) in the GEMM packing."""
    return pack_awq_gemm(*unpack_mi355x(qweight, qscales, qzeros))


def awq_gemm_to_cuda_order(qweight, qzeros, scales):
    """Checkpoint conversion: GEMM packing -> the QUICK packing (qweight, scales, qzeros) of the same layer."""
    return pack_cuda_order(*unpack_awq_gemm(qweight, qzeros, scales))


# ---------------------------------------------------------------------------------------------- gate / up of the silu_mul epilogue
def interleave8(a, b):
    """[.., I] x 2 -> [.., 2I] with out[16t + i] = a[8t + i], out[16t + 8 + i] = b[8t + i] (i < 8): the channel order of the GEMM's silu_mul
    epilogue (gate and up in blocks of 8)."""
    if a.shape != b.shape or a.shape[-1] % 8 != 0:
        raise ValueError("interleave8: two tensors of the same shape, the last dimension a multiple of 8")
    lead = a.shape[:-1]
    return torch.stack([a.reshape(*lead, -1, 8), b.reshape(*lead, -1, 8)], dim=-2).reshape(*lead, -1)


def _gate_up_dims(qweight, scales, qzeros, fused):
    """(K, I, NG) of MI355X-order tensors of one projection (or of the fused layer), the envelope of the HIP kernels checked."""
    K, I = qweight.shape[0] * 4, qweight.shape[1] * (1 if fused else 2)
    NG = scales.shape[0]
    if K % 128 != 0 or I % 64 != 0:
        raise ValueError("gate / up interleave: in_features must be a multiple of 128 and the intermediate size a multiple of 64")
    width = 2 if fused else 1
    if tuple(scales.shape) != (NG, 2 * I * width) or tuple(qzeros.shape) != (NG, I // 4 * width):
        raise ValueError(f"scales / qzeros must be [{NG}, {2 * I * width}] / [{NG}, {I // 4 * width}], got {tuple(scales.shape)} / {tuple(qzeros.shape)}")
    return K, I, NG


def interleave_gate_up_mi355x(gate, up):
    """MI355X-order (qweight, scales, qzeros) of gate_proj and of up_proj -> those of the layer with channels interleave8(gate, up), in
    packed space: == pack_mi355x of the interleaved logical layers.  Weights are 16-byte pieces [channel tile of 16][k tile][quarter][16],
    scale words [channel tile][group][16]; fused tile T takes half T % 2 of tile T / 2 of either projection, gate's in front of up's
    (quick_interleave_gate_up_mi355x, include/quick_amd.h)."""
    K, I, NG = _gate_up_dims(*gate, fused=False)
    if any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(gate, up)):
        raise ValueError("gate and up must have the same shapes and dtypes")
    qw = torch.stack([t.reshape(I // 16, K // 128, 4, 2, 8, 4) for t in (gate[0], up[0])], dim=4)         # (T', kt, q, T % 2, gate | up, c % 8, dword)
    qw = qw.permute(0, 3, 1, 2, 4, 5, 6).reshape(K // 4, I)
    sc = torch.stack([t.contiguous().view(torch.int32).reshape(I // 16, NG, 2, 8) for t in (gate[1], up[1])], dim=3)   # (T', g, T % 2, gate | up, c % 8)
    sc = sc.permute(0, 2, 1, 3, 4).reshape(NG, 2 * I).view(torch.float16)
    qz = torch.stack([gate[2][:, :I // 8], up[2][:, :I // 8]], dim=2).reshape(NG, I // 4)
    return qw, sc, torch.cat([qz, torch.zeros_like(qz)], dim=1)


def split_gate_up_mi355x(qweight, scales, qzeros):
    """The inverse of interleave_gate_up_mi355x: -> ((qweight, scales, qzeros) of gate, the same of up)."""
    K, I, NG = _gate_up_dims(qweight, scales, qzeros, fused=True)
    qw = qweight.reshape(I // 16, 2, K // 128, 4, 2, 8, 4).permute(4, 0, 2, 3, 1, 5, 6).reshape(2, K // 4, I // 2)
    sc = scales.contiguous().view(torch.int32).reshape(I // 16, 2, NG, 2, 8).permute(3, 0, 2, 1, 4).reshape(2, NG, I).view(torch.float16)
    qz = qzeros[:, :I // 4].reshape(NG, I // 8, 2).permute(2, 0, 1)
    qz = torch.cat([qz, torch.zeros_like(qz)], dim=2)
    return tuple((qw[h].contiguous(), sc[h].contiguous(), qz[h].contiguous()) for h in (0, 1))
