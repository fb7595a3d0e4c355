"""Python face of libquick_amd.so: the functions the reference's ``quick_kernels`` extension exports
(csrc/pybind.cpp:5-8), plus the format bridge.  Device pointers and the current HIP stream come from
torch; the arithmetic is entirely in the HIP library -- there is no CPU / eager fallback.
"""
import ctypes
import weakref

import torch

from . import _lib

KERNEL_AUTO, KERNEL_SKINNY, KERNEL_TILED, KERNEL_WIDE, KERNEL_XK, KERNEL_XW, KERNEL_LEAN, KERNEL_XM = 0, 1, 2, 3, 4, 5, 6, 7
_OK, _INVALID, _WORKSPACE, _LAUNCH, _UNSUPPORTED = 0, 1, 2, 3, 4


def _raise(rc):
    msg = _lib.last_error() or f"libquick_amd error {rc}"
    if rc == _INVALID:
        raise ValueError(msg)          # std::invalid_argument in the reference (gemm_cuda_quick.cu:1479-1484)
    if rc == _UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(msg)


def _expect(t, dtype, name):
    if t.dtype != dtype:               # data_ptr<T>() throws c10::Error -> RuntimeError in the reference
        raise RuntimeError(f"expected scalar type {dtype} for {name} but found {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor: the W4A16 GEMM has no CPU implementation")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _stream():
    return torch.cuda.current_stream().cuda_stream


_WORKSPACES = {}          # (device index, stream handle) -> zero-filled uint8 tensor; insertion order = recency
_WORKSPACES_MAX = 16      # stream handles are recycled by the runtime: keep the few most recently used, drop the rest
_CAPTURED = set()         # keys whose buffer a hipGraph capture has baked into kernel arguments: never evicted
_KEEPALIVE = []           # buffers a capture used and that were outgrown since: a replayed graph still writes into them


def _workspace(device, nbytes):
    """Zero-filled scratch for the in-kernel split-K reduction / K-slice exchange, one per (device, stream), grown on demand.
    The library hands it back zeroed after every launch, so it is allocated and cleared only when it has to grow.  A buffer
    that was used while its stream was being captured is pinned: the graph holds its address (counters and mailboxes that must
    be zero on entry), so it is neither evicted by the LRU cap nor freed when a later, larger request replaces it."""
    key = (device.index, _stream())
    capturing = torch.cuda.is_current_stream_capturing()
    ws = _WORKSPACES.pop(key, None)
    if ws is None or ws.numel() < nbytes:
        if ws is not None and key in _CAPTURED:
            _KEEPALIVE.append(ws)
        ws = torch.zeros(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
    _WORKSPACES[key] = ws                                  # most recently used last
    if capturing:
        _CAPTURED.add(key)
    evictable = [k for k in _WORKSPACES if k not in _CAPTURED]
    while len(evictable) > _WORKSPACES_MAX:
        _WORKSPACES.pop(evictable.pop(0))                  # (in-flight launches keep their buffer alive through the allocator's stream ordering)
    return ws


def can_fuse_rmsnorm(M, K, N, G):
    """True when gemm_forward(..., rmsnorm_weight=...) is available for this shape (small M, x held whole in LDS)."""
    return bool(_lib.load().quick_w4a16_can_fuse_rmsnorm(M, K, N, G))


def plan_describe(M, K, N, G, kernel_id=KERNEL_AUTO, grid_split_k=0):
    """One line saying what a launch of this shape runs (quick_w4a16_plan_describe; host-only, no GPU needed)."""
    import ctypes
    buf = ctypes.create_string_buffer(256)
    rc = _lib.load().quick_w4a16_plan_describe(M, K, N, G, kernel_id, grid_split_k, buf, len(buf))
    if rc != _OK:
        _raise(rc)
    return buf.value.decode()


def _check_gemm(in_feats, kernel, scaling_factors, zeros, bias, residual, out, rmsnorm_weight, silu_mul):
    """The library takes raw pointers: everything it will dereference is checked here (dtype, device, contiguity, shape).
    Returns (M, K, N, G, out) with ``out`` allocated if it was None."""
    _expect(in_feats, torch.float16, "in_feats")
    _expect(kernel, torch.int32, "kernel")
    _expect(scaling_factors, torch.float16, "scaling_factors")
    _expect(zeros, torch.int32, "zeros")
    if in_feats.dim() != 2:
        raise RuntimeError("in_feats must be 2-D [M, K]")
    M, K = in_feats.shape
    N = kernel.shape[1] // 4 * 8                      # gemm_cuda_quick.cu:1468
    if kernel.shape[0] * 4 != K:
        raise ValueError(f"kernel has {kernel.shape[0] * 4} input channels, in_feats has {K}")
    G = K // scaling_factors.shape[0]                 # gemm_cuda_quick.cu:1477
    if tuple(scaling_factors.shape) != (K // G, 2 * N) or tuple(zeros.shape) != (K // G, N // 4):
        raise ValueError(f"scaling_factors / zeros must be [{K // G}, {2 * N}] / [{K // G}, {N // 4}] for K={K} N={N} G={G}, "
                         f"got {tuple(scaling_factors.shape)} / {tuple(zeros.shape)}")
    n_out = N // 2 if silu_mul else N
    for t, shape, name in ((out, (M, n_out), "out"), (bias, (N,), "bias"), (residual, (M, N), "residual"),
                           (rmsnorm_weight, (K,), "rmsnorm_weight")):
        if t is None:
            continue
        _expect(t, torch.float16, name)
        if tuple(t.shape) != shape or t.device != in_feats.device:
            raise ValueError(f"{name} must be a {list(shape)} fp16 tensor on {in_feats.device}, got {list(t.shape)} on {t.device}")
    for t, name in ((kernel, "kernel"), (scaling_factors, "scaling_factors"), (zeros, "zeros")):
        if t.device != in_feats.device:
            raise RuntimeError(f"{name} is on {t.device}, in_feats on {in_feats.device}")
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.float16, device=in_feats.device)
    return M, K, N, G, out


def gemm_forward(in_feats, kernel, scaling_factors, zeros, bias=None, kernel_id=KERNEL_AUTO, grid_split_k=0, residual=None,
                 out=None, rmsnorm_weight=None, rmsnorm_eps=1e-5, silu_mul=False):
    """y [M, N] fp16 = in_feats [M, K] @ dequant(kernel, scaling_factors, zeros) (+ bias) (+ residual), MI355X-order
    weights.  ``out`` (optional, may be ``residual``) receives the result.  ``rmsnorm_weight`` [K] normalises in_feats on
    the way in (see can_fuse_rmsnorm); ``silu_mul`` treats the output channels as gate/up interleaved in blocks of 8 and
    returns silu(gate) * up, [M, N/2]."""
    M, K, N, G, out = _check_gemm(in_feats, kernel, scaling_factors, zeros, bias, residual, out, rmsnorm_weight, silu_mul)
    lib = _lib.load()
    if M == 0:
        return out
    with torch.cuda.device(in_feats.device):          # OptionalCUDAGuard, gemm_cuda_quick.cu:1465
        ws_bytes = lib.quick_w4a16_workspace_bytes_ex(M, K, N, G, kernel_id, grid_split_k)
        ws = _workspace(in_feats.device, ws_bytes) if ws_bytes else None
        fusion = _lib.GemmFusion(bias.data_ptr() if bias is not None else None,
                                 residual.data_ptr() if residual is not None else None,
                                 rmsnorm_weight.data_ptr() if rmsnorm_weight is not None else None, rmsnorm_eps, int(silu_mul))
        rc = lib.quick_w4a16_gemm_f16_fused(
            in_feats.data_ptr(), kernel.data_ptr(), scaling_factors.data_ptr(), zeros.data_ptr(), ctypes.byref(fusion),
            out.data_ptr(),
            ws.data_ptr() if ws is not None else None, ws.numel() if ws is not None else 0, M, K, N, G, kernel_id,
            grid_split_k, _stream())
    if rc != _OK:
        if ws is not None:                                # whatever went wrong, the next launch finds the state it expects: all-zero
            ws.zero_()
        _raise(rc)
    return out


def workspace_check(device=None):
    """Verify that this stream's workspace is all-zero where the library expects it (quick_w4a16_workspace_check: synchronises).
    Raises RuntimeError naming the first dirty byte -- and zeroes the buffer again -- otherwise."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(device):      # (the stream is THAT device's current stream: key and call both)
        stream = torch.cuda.current_stream(device).cuda_stream
        ws = _WORKSPACES.get((device.index, stream))
        if ws is None:
            return True
        rc = _lib.load().quick_w4a16_workspace_check(ws.data_ptr(), ws.numel(), stream)
    if rc != _OK:
        ws.zero_()
        _raise(rc)
    return True


def _tensor_version(t):
    return 0 if t.is_inference() else t._version     # inference tensors have no version counter (and cannot be rewritten in place outside inference mode)


class _Repacked:
    __slots__ = ("refs", "versions", "packed", "stream", "event", "done", "seen")


_REPACK_CACHE = {}     # (data_ptr of qweight, scales, qzeros) -> _Repacked; entries die with the tensors they mirror


def reference_to_mi355x_cached(kernel, scaling_factors, zeros):
    """MI355X-order copies of reference-order packed tensors, made once per tensor triple by the HIP repack kernel.

    This is what lets the reference's own ``WQLinear_QUICK.forward`` (quick/awq/modules/linear/quick.py:158-166), whose
    buffers hold the checkpoint order of ``from_linear`` (quick.py:88-150), call this library unchanged.  The entry is
    keyed on the identity (weak references) and version counters of the three tensors: an in-place rewrite
    (``load_state_dict``, ``copy_``) or a new tensor object invalidates it, and it is dropped when a tensor dies.  Cost: a
    second copy of the layer's packed weights in HBM -- ``quick_amd.WQLinear_QUICK`` avoids it by permuting its own
    buffers in place and calling :func:`gemm_forward` directly.
    """
    tensors = (kernel, scaling_factors, zeros)
    key = tuple(t.data_ptr() for t in tensors)
    versions = tuple(_tensor_version(t) for t in tensors)
    ent = _REPACK_CACHE.get(key)
    if ent is not None and ent.versions == versions and all(r() is t for r, t in zip(ent.refs, tensors)):
        if kernel.is_cuda:
            cur = torch.cuda.current_stream(kernel.device)
            sid = (cur.stream_id, cur.cuda_stream)     # (torch's id AND the raw handle: the runtime recycles handles of destroyed streams)
            if cur != ent.stream:
                # Made on another stream.  Outside a capture: wait for the repack ONCE on the host -- from then on the copy is visible to
                # every stream and later hits cost two comparisons.  Inside a capture nothing may block: the capturing stream
                # waits for the event, on every hit, until a call outside one has synchronised.  Either way the allocator learns once per
                # stream who else reads the copy (record_stream is capture-safe: a graph captured on a side stream is covered -- ADVICE r04).
                if not ent.done:
                    if torch.cuda.is_current_stream_capturing():
                        cur.wait_event(ent.event)
                    else:
                        ent.event.synchronize()
                        ent.done = True
                if sid not in ent.seen:
                    for t in ent.packed:
                        t.record_stream(cur)
                    ent.seen.add(sid)
        return ent.packed
    ent = _Repacked()
    ent.stream = ent.event = None
    ent.done, ent.seen = False, set()
    if kernel.shape[0] * 4 % 128 == 0:
        ent.packed = repack_cuda_to_mi355x(kernel, scaling_factors, zeros)
    else:
        ent.packed = _padded_mi355x(kernel, scaling_factors, zeros)
    ent.versions = versions
    if kernel.is_cuda:
        ent.stream = torch.cuda.current_stream(kernel.device)
        ent.event = torch.cuda.Event()
        ent.event.record(ent.stream)
    drop = lambda _ref, key=key: _REPACK_CACHE.pop(key, None)
    ent.refs = tuple(weakref.ref(t, drop) for t in tensors)
    _REPACK_CACHE[key] = ent
    return ent.packed


def padded_in_features(K, G):
    """The reference accepts in_features % 32 == 0 (csrc/gemm_cuda_quick.cu:1479-1484); the MI355X weight order is made of
    128-k tiles.  A layer in between (only possible with group sizes that are not multiples of 128) runs on a copy padded
    along K to the next multiple of lcm(128, G): weights 0, zero points 0, scales 0 in the added groups -- they contribute
    exactly 0 -- and the activations padded with zeros per call."""
    import math
    unit = 128 * G // math.gcd(128, G)
    return (K + unit - 1) // unit * unit


def _padded_mi355x(kernel, scaling_factors, zeros):
    """MI355X-order tensors of a reference-order layer whose K is not a multiple of 128, once per layer: the HIP repack
    kernel's padded flavour on the GPU, torch ops on CPU tensors (tests)."""
    from . import packing
    if kernel.is_cuda:
        K, N = kernel.shape[0] * 4, kernel.shape[1] * 2
        G = K // scaling_factors.shape[0]
        lib = _lib.load()
        Kp = lib.quick_padded_in_features(K, G)
        if Kp == 0:
            raise ValueError(f"quick_repack_cuda_to_mi355x_padded: invalid shape K={K} N={N} G={G}")
        outs = [torch.empty((Kp // 4, N // 2), dtype=torch.int32, device=kernel.device),
                torch.empty((Kp // G, 2 * N), dtype=torch.float16, device=kernel.device),
                torch.empty((Kp // G, N // 4), dtype=torch.int32, device=kernel.device)]
        with torch.cuda.device(kernel.device):
            rc = lib.quick_repack_cuda_to_mi355x_padded(kernel.data_ptr(), scaling_factors.data_ptr(), zeros.data_ptr(),
                                                        outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), K, N, G, _stream())
        if rc != _OK:
            _raise(rc)
        return tuple(outs)
    iw, s, z = packing.unpack_cuda_order(kernel, scaling_factors, zeros)
    K, G = iw.shape[0], iw.shape[0] // s.shape[0]
    Kp = padded_in_features(K, G)
    pad = lambda t, rows: torch.cat([t, torch.zeros((rows - t.shape[0],) + tuple(t.shape[1:]), dtype=t.dtype, device=t.device)])
    return packing.pack_mi355x(pad(iw, Kp), pad(s, Kp // G), pad(z, Kp // G))


def gemm_forward_cuda_quick(in_feats, kernel, scaling_factors, zeros, split_k_iters):
    """Drop-in for ``quick_kernels.gemm_forward_cuda_quick`` (csrc/gemm_cuda_quick.h:3-8, csrc/pybind.cpp:5-8).

    Same arguments, dtypes, error behaviour and -- like the reference -- the REFERENCE's packed order: ``kernel`` /
    ``scaling_factors`` / ``zeros`` are what ``WQLinear_QUICK.from_linear`` of the reference writes and what its
    checkpoints hold (quick.py:88-150), so the reference's unchanged module can call it.  The MI355X-order copy the HIP
    kernels consume is made on first use and cached (:func:`reference_to_mi355x_cached`).  Return shape follows the
    reference: ``[M, N]`` when ``split_k_iters > 1`` (its ``.sum(0)``), ``[1, M, N]`` otherwise
    (gemm_cuda_quick.cu:1515-1516).  ``split_k_iters`` is a tuning hint for NVIDIA parts; this library chooses its own K
    partitioning and always returns the fully reduced result.
    """
    if split_k_iters < 1:
        raise ValueError("split_k_iters must be >= 1")
    _expect(in_feats, torch.float16, "in_feats")
    _expect(kernel, torch.int32, "kernel")
    _expect(scaling_factors, torch.float16, "scaling_factors")
    _expect(zeros, torch.int32, "zeros")
    if in_feats.dim() != 2:
        raise RuntimeError("in_feats must be 2-D [M, K]")
    K, N = kernel.shape[0] * 4, kernel.shape[1] // 4 * 8       # gemm_cuda_quick.cu:1468
    if in_feats.shape[1] != K:
        raise ValueError(f"kernel has {K} input channels, in_feats has {in_feats.shape[1]}")
    G = K // scaling_factors.shape[0]
    Kp = K if K % 128 == 0 or K % 32 != 0 or G % 32 != 0 or K % G != 0 else padded_in_features(K, G)
    plan_describe(max(int(in_feats.shape[0]), 1), Kp, N, G)   # the reference's shape errors, before any repack
    if Kp != K:                                              # in_features % 128 != 0: the padded copy, zero-padded activations
        in_feats = torch.nn.functional.pad(in_feats, (0, Kp - K))
    out = gemm_forward(in_feats, *reference_to_mi355x_cached(kernel, scaling_factors, zeros))
    return out if split_k_iters > 1 else out.unsqueeze(0)


def _repack(fn_name, qweight, scales, qzeros):
    for t, d, nm in ((qweight, torch.int32, "qweight"), (scales, torch.float16, "scales"), (qzeros, torch.int32, "qzeros")):
        _expect(t, d, nm)
    lib = _lib.load()
    K, N = qweight.shape[0] * 4, qweight.shape[1] * 2
    G = K // scales.shape[0]
    outs = [torch.empty_like(qweight), torch.empty_like(scales), torch.empty_like(qzeros)]
    with torch.cuda.device(qweight.device):
        rc = getattr(lib, fn_name)(qweight.data_ptr(), scales.data_ptr(), qzeros.data_ptr(),
                                   outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), K, N, G, _stream())
    if rc != _OK:
        if rc == _INVALID:
            raise ValueError(f"{fn_name}: invalid shape K={K} N={N} G={G}")
        if rc == _UNSUPPORTED:
            raise NotImplementedError(f"{fn_name}: in_features ({K}) must be a multiple of 128 on MI355X")
        raise RuntimeError(f"{fn_name} failed ({rc})")
    return tuple(outs)


def repack_cuda_to_mi355x(qweight, scales, qzeros):
    """Reference-order packed tensors (a QUICK checkpoint) -> MI355X order, on the GPU."""
    return _repack("quick_repack_cuda_to_mi355x", qweight, scales, qzeros)


def repack_mi355x_to_cuda(qweight, scales, qzeros):
    return _repack("quick_repack_mi355x_to_cuda", qweight, scales, qzeros)


def _awq_gemm_dims(rows, n8, groups, what):
    """(K, N, G) of a GEMM-packing layer from its tensor shapes; the library answers the shape rules itself."""
    if groups <= 0 or rows % groups != 0:
        raise ValueError(f"{what}: {rows} input channels do not divide into {groups} groups")
    return rows, n8 * 8, rows // groups


def repack_awq_gemm_to_mi355x(qweight, qzeros, scales):
    """AWQ GEMM-packing tensors (a ``WQLinear_GEMM`` checkpoint: qweight int32 [K, N/8], qzeros int32 [K/G, N/8], scales fp16
    [K/G, N]) -> (qweight, scales, qzeros) in MI355X order, on the GPU.  The outputs have ``padded_in_features(K, G)`` rows'
    worth of weights and groups (== K when K % 128 == 0); what lies beyond K contributes exactly 0."""
    fn_name = "quick_repack_awq_gemm_to_mi355x"
    for t, d, nm in ((qweight, torch.int32, "qweight"), (qzeros, torch.int32, "qzeros"), (scales, torch.float16, "scales")):
        _expect(t, d, nm)
    K, N, G = _awq_gemm_dims(qweight.shape[0], qweight.shape[1], scales.shape[0], fn_name)
    if tuple(qzeros.shape) != (K // G, N // 8) or tuple(scales.shape) != (K // G, N):
        raise ValueError(f"{fn_name}: qzeros / scales must be [{K // G}, {N // 8}] / [{K // G}, {N}] for K={K} N={N} G={G}, "
                         f"got {tuple(qzeros.shape)} / {tuple(scales.shape)}")
    lib = _lib.load()
    Kp = lib.quick_padded_in_features(K, G) or K      # (0: a shape the call below refuses before it touches the outputs)
    dev = qweight.device
    outs = [torch.empty((Kp // 4, N // 2), dtype=torch.int32, device=dev),
            torch.empty((Kp // G, 2 * N), dtype=torch.float16, device=dev),
            torch.empty((Kp // G, N // 4), dtype=torch.int32, device=dev)]
    with torch.cuda.device(dev):
        rc = lib.quick_repack_awq_gemm_to_mi355x(qweight.data_ptr(), qzeros.data_ptr(), scales.data_ptr(),
                                                 outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), K, N, G, _stream())
    if rc != _OK:
        _raise(rc)
    return tuple(outs)


def repack_mi355x_to_awq_gemm(qweight, scales, qzeros, in_features=None):
    """MI355X-order tensors -> (qweight, qzeros, scales) in the AWQ GEMM packing, on the GPU.  in_features % 128 == 0: a padded copy
    (``in_features``, the layer's own, smaller than the tensors' rows) is never turned back -- NotImplementedError."""
    fn_name = "quick_repack_mi355x_to_awq_gemm"
    for t, d, nm in ((qweight, torch.int32, "qweight"), (scales, torch.float16, "scales"), (qzeros, torch.int32, "qzeros")):
        _expect(t, d, nm)
    K, N, G = _awq_gemm_dims(qweight.shape[0] * 4, qweight.shape[1] // 4, scales.shape[0], fn_name)
    if in_features is not None and in_features != K:
        if in_features % 128 == 0:
            raise ValueError(f"{fn_name}: the tensors hold {K} input channels, not {in_features}")
        K = in_features                                # (the library refuses it before it touches a tensor)
    NG = scales.shape[0]
    if tuple(scales.shape) != (NG, 2 * N) or tuple(qzeros.shape) != (NG, N // 4):
        raise ValueError(f"{fn_name}: scales / qzeros must be [{NG}, {2 * N}] / [{NG}, {N // 4}] for N={N} G={G}, "
                         f"got {tuple(scales.shape)} / {tuple(qzeros.shape)}")
    dev = qweight.device
    outs = [torch.empty((K, N // 8), dtype=torch.int32, device=dev),
            torch.empty((K // G, N // 8), dtype=torch.int32, device=dev),
            torch.empty((K // G, N), dtype=torch.float16, device=dev)]
    with torch.cuda.device(dev):
        rc = _lib.load().quick_repack_mi355x_to_awq_gemm(qweight.data_ptr(), scales.data_ptr(), qzeros.data_ptr(),
                                                         outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), K, N, G, _stream())
    if rc != _OK:
        _raise(rc)
    return tuple(outs)


def gate_up_shape_check(K, I, G):
    """The shape rules of the gate / up interleave (include/quick_amd.h), answered by the library without a GPU: NotImplementedError with
    its sentence outside the envelope (K % 128, I % 64), ValueError for a shape that is no layer at all."""
    rc = _lib.load().quick_interleave_gate_up_mi355x(*([None] * 9), K, I, G, None)
    if rc != _OK and "null tensor pointer" not in _lib.last_error():      # (the rules come first; with them met, the pointers are all it can object to)
        _raise(rc)


def _gate_up_triple(t, I, width, what):
    """dtype, device, contiguity and shape of one MI355X-order (qweight, scales, qzeros) of `width` * I channels; -> (K, NG)."""
    qweight, scales, qzeros = t
    for x, d, nm in ((qweight, torch.int32, "qweight"), (scales, torch.float16, "scales"), (qzeros, torch.int32, "qzeros")):
        _expect(x, d, f"{what} {nm}")
        if x.dim() != 2 or x.device != qweight.device:
            raise ValueError(f"{what} {nm} must be a 2-D tensor on {qweight.device}")
    K, NG = qweight.shape[0] * 4, scales.shape[0]
    want = ((K // 4, I // 2 * width), (NG, 2 * I * width), (NG, I // 4 * width))
    if tuple(tuple(x.shape) for x in t) != want:
        raise ValueError(f"{what}: qweight / scales / qzeros must be {' / '.join(str(list(w)) for w in want)}, got "
                         f"{' / '.join(str(list(x.shape)) for x in t)}")
    return K, NG


def _gate_up_call(fn_name, tensors, K, I, NG):
    """``tensors``: the nine of the C signature, in its order."""
    if NG <= 0 or K % NG != 0:
        raise ValueError(f"{fn_name}: {K} input channels do not divide into {NG} groups")
    with torch.cuda.device(tensors[0].device):
        rc = getattr(_lib.load(), fn_name)(*[x.data_ptr() for x in tensors], K, I, K // NG, _stream())
    if rc != _OK:
        _raise(rc)


def _empty_gate_up(K, I, NG, width, dev):
    return (torch.empty((K // 4, I // 2 * width), dtype=torch.int32, device=dev),
            torch.empty((NG, 2 * I * width), dtype=torch.float16, device=dev),
            torch.empty((NG, I // 4 * width), dtype=torch.int32, device=dev))


def interleave_gate_up_mi355x(gate, up, out=None):
    """MI355X-order (qweight, scales, qzeros) of gate_proj and of up_proj -> those of the [K, 2I] layer whose output channels interleave
    gate and up in blocks of 8, which ``gemm_forward(..., silu_mul=True)`` reads; one HIP launch.  ``out`` (optional): the three tensors
    to write, which must not share memory with the inputs."""
    fn_name = "quick_interleave_gate_up_mi355x"
    gate, up = tuple(gate), tuple(up)
    I = gate[0].shape[1] * 2
    K, NG = _gate_up_triple(gate, I, 1, "gate")
    if _gate_up_triple(up, I, 1, "up") != (K, NG) or up[0].device != gate[0].device:
        raise ValueError(f"{fn_name}: gate and up must be layers of the same shape on the same device")
    if out is None:
        out = _empty_gate_up(K, I, NG, 2, gate[0].device)
    elif _gate_up_triple(tuple(out), I, 2, "out") != (K, NG) or out[0].device != gate[0].device:
        raise ValueError(f"{fn_name}: out must be the fused layer of the same K and groups on the same device")
    _gate_up_call(fn_name, gate + up + tuple(out), K, I, NG)
    return tuple(out)


def split_gate_up_mi355x(qweight, scales, qzeros, out=None):
    """The inverse of interleave_gate_up_mi355x (saving): -> ((qweight, scales, qzeros) of gate, the same of up).  ``out``: the two
    triples to write."""
    fn_name = "quick_split_gate_up_mi355x"
    fused = (qweight, scales, qzeros)
    I = qweight.shape[1]
    K, NG = _gate_up_triple(fused, I, 2, "fused")
    if out is None:
        out = (_empty_gate_up(K, I, NG, 1, qweight.device), _empty_gate_up(K, I, NG, 1, qweight.device))
    gate, up = tuple(out[0]), tuple(out[1])
    for t, what in ((gate, "out gate"), (up, "out up")):
        if _gate_up_triple(t, I, 1, what) != (K, NG) or t[0].device != qweight.device:
            raise ValueError(f"{fn_name}: {what} must be a projection of the same K and groups on the same device")
    _gate_up_call(fn_name, fused + gate + up, K, I, NG)
    return gate, up


def dequantize_mi355x(qweight, scales, qzeros):
    """Dense fp16 [K, N] = fp16((w - z) * s) from MI355X-order tensors (parity aid)."""
    lib = _lib.load()
    K, N = qweight.shape[0] * 4, qweight.shape[1] * 2
    G = K // scales.shape[0]
    out = torch.empty((K, N), dtype=torch.float16, device=qweight.device)
    with torch.cuda.device(qweight.device):
        rc = lib.quick_dequantize_mi355x_f16(qweight.data_ptr(), scales.data_ptr(), qzeros.data_ptr(), out.data_ptr(),
                                             K, N, G, _stream())
    if rc != _OK:
        _raise(rc)
    return out


# ---------------------------------------------------------------------------------------------- decode-step glue
def rmsnorm(x, weight, eps=1e-5, out=None):
    """RMSNorm over the last dimension (fp16, H % 8 == 0)."""
    lib = _lib.load()
    H = x.shape[-1]
    out = torch.empty_like(x) if out is None else out
    rc = lib.quick_rmsnorm_f16(x.data_ptr(), weight.data_ptr(), out.data_ptr(), x.numel() // H, H, eps, _stream())
    if rc != _OK:
        raise RuntimeError(f"quick_rmsnorm_f16 failed ({rc})")
    return out


def rope_kv_append(qkv, cos_table, sin_table, pos, q_out, k_cache, v_cache, n_heads, n_kv_heads, head_dim):
    """Decode step: rotate q/k of the fused qkv GEMM output [B, (nh + 2 nkv) D], append k/v to the caches at *pos."""
    lib = _lib.load()
    rc = lib.quick_rope_kv_append_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos.data_ptr(), q_out.data_ptr(),
                                      k_cache.data_ptr(), v_cache.data_ptr(), qkv.shape[0], n_heads, n_kv_heads, head_dim,
                                      k_cache.shape[2], _stream())
    if rc != _OK:
        raise RuntimeError(f"quick_rope_kv_append_f16 failed ({rc})")
    return q_out


def _per_sequence_pos(pos, batch, like, name):
    """The position argument of a per-sequence launch: a device int64 tensor of exactly `batch` elements, on the device of `like`.
    Anything else is a ValueError before the library is called (the kernels index it by the sequence)."""
    if not isinstance(pos, torch.Tensor) or pos.dtype != torch.int64:
        raise ValueError(f"per_sequence: {name} must be an int64 tensor, got {getattr(pos, 'dtype', type(pos).__name__)}")
    if pos.numel() != batch or not pos.is_contiguous():
        raise ValueError(f"per_sequence: {name} must hold exactly one contiguous position per sequence ({batch}), it holds {pos.numel()}")
    if not pos.is_cuda or pos.device != like.device:
        raise ValueError(f"per_sequence: {name} must be a GPU tensor on the device of the caches ({like.device}), it is on {pos.device}")


_BYTE_DTYPES = (torch.float8_e4m3fn, torch.uint8)


def _byte_caches(k_cache, v_cache):
    """True when the caches are one-byte (OCP e4m3fn; a uint8 view of the same bytes is accepted): the launch is then the fp8 one.  A
    pair of unequal kinds is a RuntimeError; fp16 caches (False) take the path they always took."""
    kb, vb = k_cache.dtype in _BYTE_DTYPES, v_cache.dtype in _BYTE_DTYPES
    if kb != vb:
        raise RuntimeError(f"k_cache and v_cache must be of one kind, got {k_cache.dtype} and {v_cache.dtype}")
    if kb:
        for t, name in ((k_cache, "k_cache"), (v_cache, "v_cache")):
            if not t.is_cuda or not t.is_contiguous() or t.dim() != 4:
                raise RuntimeError(f"{name} must be a contiguous 4-D GPU tensor [batch, n_kv_heads, cache_len, head_dim]")
    return kb


def _window(window, table_rows, k_cache, v_cache, cos_table, who):
    """The (window, ring_rows, table_rows) ints of a windowed launch (quick_*_win_f16): fp16 ring caches [B, nkv, ring_rows, D];
    ``table_rows`` defaults to the rows of ``cos_table``.  Byte caches with a window are a ValueError (out of scope)."""
    if k_cache.dtype in _BYTE_DTYPES or v_cache.dtype in _BYTE_DTYPES:
        raise ValueError(f"{who}: a sliding window over one-byte (fp8) caches is not supported; use fp16 caches or window=None")
    for t, name in ((k_cache, "k_cache"), (v_cache, "v_cache")):
        _expect(t, torch.float16, name)
        if t.dim() != 4 or not t.is_contiguous() or t.shape != k_cache.shape:
            raise ValueError(f"{who}: {name} must be a contiguous ring cache [batch, n_kv_heads, ring_rows, head_dim] of k_cache's shape")
    if table_rows is None:
        if cos_table is None:
            raise ValueError(f"{who}: window needs table_rows (the exclusive bound on positions; there is no RoPE table to take it from)")
        table_rows = cos_table.shape[0]
    return int(window), k_cache.shape[2], int(table_rows)


def _paged(block_table, page_size, table_rows, k_pool, v_pool, cos_table, batch, window, k_scale, v_scale, who):
    """The (num_pages, page_size, max_pages, table_rows) ints of a paged launch (quick_*_paged_f16): fp16 pools
    [num_pages, n_kv_heads, page_size, head_dim] and a device int32 block table [batch, max_pages]; ``table_rows`` defaults to the rows of
    ``cos_table``.  Combined with a window, one-byte caches or fp8 scales: a ValueError (out of scope)."""
    if window is not None:
        raise ValueError(f"{who}: block_table and window together are not supported (a windowed paged cache is out of scope)")
    if k_pool.dtype in _BYTE_DTYPES or v_pool.dtype in _BYTE_DTYPES:
        raise ValueError(f"{who}: a block_table over one-byte (fp8) pools is not supported; use fp16 pools")
    if k_scale != 1.0 or v_scale != 1.0:
        raise ValueError(f"{who}: k_scale / v_scale belong to one-byte caches and cannot be combined with block_table")
    if page_size is None:
        raise ValueError(f"{who}: block_table needs page_size")
    for t, name in ((k_pool, "k_cache"), (v_pool, "v_cache")):
        if t.dim() != 4 or not t.is_contiguous() or t.shape != k_pool.shape or t.shape[2] != int(page_size):
            raise ValueError(f"{who}: {name} must be a contiguous pool [num_pages, n_kv_heads, page_size = {page_size}, head_dim] of "
                             f"k_cache's shape, got {list(t.shape)}")
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or block_table.dim() != 2 \
            or block_table.shape[0] != batch or not block_table.is_contiguous():
        raise ValueError(f"{who}: block_table must be a contiguous int32 tensor [batch = {batch}, max_pages]")
    if not block_table.is_cuda or block_table.device != k_pool.device:
        raise ValueError(f"{who}: block_table must be a GPU tensor on the device of the pools ({k_pool.device}), it is on {block_table.device}")
    if table_rows is None:
        if cos_table is None:
            raise ValueError(f"{who}: block_table needs table_rows (the exclusive bound on positions; there is no RoPE table to take it from)")
        table_rows = cos_table.shape[0]
    for t, name in ((k_pool, "k_cache"), (v_pool, "v_cache")):
        _expect(t, torch.float16, name)
    return k_pool.shape[0], int(page_size), block_table.shape[1], int(table_rows)


def rope_kv_write(qkv, cos_table, sin_table, pos0, q_out, k_cache, v_cache, tokens, n_heads, n_kv_heads, head_dim, per_sequence=False,
                  k_scale=1.0, v_scale=1.0, window=None, table_rows=None, block_table=None, page_size=None):
    """Prefill: qkv [B * T, (nh + 2 nkv) D] -> rotated q in q_out [B, nh, T, D], rotated k and v into the caches at
    positions *pos0 .. *pos0 + T - 1.  ``per_sequence``: pos0 is a device int64 [B] and sequence b starts at pos0[b]
    (quick_rope_kv_write_seq_f16); a sequence whose start lies outside 0 .. L - T is skipped.  One-byte caches
    (``torch.float8_e4m3fn``, or ``uint8`` holding the same bytes) are written by quick_rope_kv_write_fp8 as
    ``attention.quantize_kv`` of the rows the fp16 launch would store, with ``k_scale`` / ``v_scale``; q_out is the same, bit for bit.
    ``window`` (fp16 caches only): the caches are rings of ``k_cache.shape[2]`` rows and the token at position j is stored at row
    j % ring_rows (quick_rope_kv_write_win_f16); ``table_rows`` bounds the positions (default: the rows of ``cos_table``).
    ``block_table`` (device int32 [B, max_pages], with ``page_size``; fp16 only): the caches are page pools
    [num_pages, nkv, page_size, D] and the token at position j of sequence b is stored at pool row
    (block_table[b][j // page_size], kvh, j % page_size) (quick_rope_kv_write_paged_f16); a row whose entry names no page is dropped."""
    if block_table is not None:
        B = qkv.shape[0] // tokens
        pages, psize, max_pages, table_rows = _paged(block_table, page_size, table_rows, k_cache, v_cache, cos_table, B, window, k_scale,
                                                     v_scale, "rope_kv_write")
        if per_sequence:
            _per_sequence_pos(pos0, B, k_cache, "pos0")
        rc = _lib.load().quick_rope_kv_write_paged_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos0.data_ptr(),
                                                       q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), block_table.data_ptr(), B,
                                                       tokens, n_heads, n_kv_heads, head_dim, pages, psize, max_pages, table_rows,
                                                       int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return q_out
    if window is not None:
        _, ring, table_rows = _window(window, table_rows, k_cache, v_cache, cos_table, "rope_kv_write")
        if per_sequence:
            _per_sequence_pos(pos0, qkv.shape[0] // tokens, k_cache, "pos0")
        rc = _lib.load().quick_rope_kv_write_win_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos0.data_ptr(),
                                                     q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), qkv.shape[0] // tokens,
                                                     tokens, n_heads, n_kv_heads, head_dim, ring, table_rows, int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return q_out
    if _byte_caches(k_cache, v_cache):
        if per_sequence:
            _per_sequence_pos(pos0, qkv.shape[0] // tokens, k_cache, "pos0")
        rc = _lib.load().quick_rope_kv_write_fp8(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos0.data_ptr(),
                                                 q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), qkv.shape[0] // tokens, tokens,
                                                 n_heads, n_kv_heads, head_dim, k_cache.shape[2], k_scale, v_scale, int(per_sequence),
                                                 _stream())
        if rc != _OK:
            _raise(rc)
        return q_out
    if per_sequence:
        _per_sequence_pos(pos0, qkv.shape[0] // tokens, k_cache, "pos0")
        rc = _lib.load().quick_rope_kv_write_seq_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos0.data_ptr(),
                                                     q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), qkv.shape[0] // tokens,
                                                     tokens, n_heads, n_kv_heads, head_dim, k_cache.shape[2], _stream())
        if rc != _OK:
            raise RuntimeError(f"quick_rope_kv_write_seq_f16 failed ({rc})")
        return q_out
    lib = _lib.load()
    rc = lib.quick_rope_kv_write_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos0.data_ptr(), q_out.data_ptr(),
                                     k_cache.data_ptr(), v_cache.data_ptr(), qkv.shape[0] // tokens, tokens, n_heads, n_kv_heads,
                                     head_dim, k_cache.shape[2], _stream())
    if rc != _OK:
        raise RuntimeError(f"quick_rope_kv_write_f16 failed ({rc})")
    return q_out


def prefill_attention(q, k_cache, v_cache, pos0, out, n_heads, n_kv_heads, head_dim, per_sequence=False, k_scale=1.0, v_scale=1.0,
                      window=None, table_rows=None, block_table=None, page_size=None):
    """Causal attention of T new tokens over the cache (quick_prefill_attention_f16): q [B, nh, T, D] as rope_kv_write leaves it, caches
    [B, nkv, L, D] with rows *pos0 .. *pos0 + T - 1 written, pos0 a device int64 -> out [B * T, nh * D] (row b * T + t).  Query t attends
    cache rows 0 .. *pos0 + t; no host read, no mask tensor.  ``per_sequence``: pos0 is a device int64 [B] and query t of sequence b
    attends rows 0 .. pos0[b] + t (quick_prefill_attention_seq_f16); a sequence whose start lies outside 0 .. L - T is skipped.
    One-byte caches run quick_prefill_attention_fp8 with ``k_scale`` / ``v_scale`` (see rope_kv_write).
    ``window`` (fp16 ring caches, see rope_kv_write): query t attends positions max(0, pos0 + t - window + 1) .. pos0 + t
    (quick_prefill_attention_win_f16).  ``table_rows``, the exclusive bound on positions, must be given with it; on a ring that can wrap
    (ring_rows < table_rows) a chunk needs window + T - 1 <= ring_rows.
    ``block_table`` (with ``page_size`` and ``table_rows``; fp16 page pools, see rope_kv_write): query t attends positions
    0 .. pos0 + t, each 32-row tile fetched through the table (quick_prefill_attention_paged_f16); the pool is never written."""
    if per_sequence:
        _per_sequence_pos(pos0, q.shape[0], k_cache, "pos0")
    if block_table is not None:
        pages, psize, max_pages, table_rows = _paged(block_table, page_size, table_rows, k_cache, v_cache, None, q.shape[0], window,
                                                     k_scale, v_scale, "prefill_attention")
        for t, name in ((q, "q"), (out, "out")):
            _expect(t, torch.float16, name)
        _expect(pos0, torch.int64, "pos0")
        rc = _lib.load().quick_prefill_attention_paged_f16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos0.data_ptr(),
                                                           out.data_ptr(), block_table.data_ptr(), q.shape[0], q.shape[2], n_heads,
                                                           n_kv_heads, head_dim, pages, psize, max_pages, table_rows, head_dim ** -0.5,
                                                           int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return out
    if window is not None:
        window, ring, table_rows = _window(window, table_rows, k_cache, v_cache, None, "prefill_attention")
        for t, name in ((q, "q"), (out, "out")):
            _expect(t, torch.float16, name)
        _expect(pos0, torch.int64, "pos0")
        rc = _lib.load().quick_prefill_attention_win_f16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos0.data_ptr(),
                                                         out.data_ptr(), q.shape[0], q.shape[2], n_heads, n_kv_heads, head_dim, ring,
                                                         window, table_rows, head_dim ** -0.5, int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return out
    if _byte_caches(k_cache, v_cache):
        for t, name in ((q, "q"), (out, "out")):
            _expect(t, torch.float16, name)
        _expect(pos0, torch.int64, "pos0")
        rc = _lib.load().quick_prefill_attention_fp8(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos0.data_ptr(), out.data_ptr(),
                                                     q.shape[0], q.shape[2], n_heads, n_kv_heads, head_dim, k_cache.shape[2],
                                                     head_dim ** -0.5, k_scale, v_scale, int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return out
    for t, name in ((q, "q"), (k_cache, "k_cache"), (v_cache, "v_cache"), (out, "out")):
        _expect(t, torch.float16, name)
    if per_sequence:
        rc = _lib.load().quick_prefill_attention_seq_f16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos0.data_ptr(),
                                                         out.data_ptr(), q.shape[0], q.shape[2], n_heads, n_kv_heads, head_dim,
                                                         k_cache.shape[2], head_dim ** -0.5, _stream())
        if rc != _OK:
            _raise(rc)
        return out
    _expect(pos0, torch.int64, "pos0")
    lib = _lib.load()
    rc = lib.quick_prefill_attention_f16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos0.data_ptr(), out.data_ptr(),
                                         q.shape[0], q.shape[2], n_heads, n_kv_heads, head_dim, k_cache.shape[2], head_dim ** -0.5,
                                         _stream())
    if rc != _OK:
        _raise(rc)
    return out


def prefill_attention_describe(batch, tokens, n_heads, n_kv_heads, head_dim, cache_len):
    """One line describing prefill_attention's launch for this shape (quick_prefill_attention_describe; host-only, no GPU needed)."""
    buf = ctypes.create_string_buffer(128)
    rc = _lib.load().quick_prefill_attention_describe(batch, tokens, n_heads, n_kv_heads, head_dim, cache_len, buf, len(buf))
    if rc != _OK:
        _raise(rc)
    return buf.value.decode()


def decode_attention(q, k_cache, v_cache, pos, out, n_heads, n_kv_heads, head_dim):
    """Single-query attention over cache positions 0..*pos; q [B, nh, D] -> out [B, nh * D]."""
    lib = _lib.load()
    rc = lib.quick_decode_attention_f16(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), pos.data_ptr(), out.data_ptr(),
                                        q.shape[0], n_heads, n_kv_heads, head_dim, k_cache.shape[2], head_dim ** -0.5, _stream())
    if rc != _OK:
        raise RuntimeError(f"quick_decode_attention_f16 failed ({rc})")
    return out


def rope_attention(qkv, cos_table, sin_table, pos, k_cache, v_cache, out, n_heads, n_kv_heads, head_dim, per_sequence=False,
                   k_scale=1.0, v_scale=1.0, window=None, table_rows=None, block_table=None, page_size=None):
    """rope_kv_append + decode_attention in one launch: qkv [B, (nh + 2 nkv) D] -> out [B, nh * D].  ``per_sequence``: pos is a device
    int64 [B]; sequence b rotates with table row pos[b], appends at cache row pos[b] and attends rows 0 .. pos[b]
    (quick_decode_rope_attention_seq_f16); a sequence whose position lies outside 0 .. L - 1 is skipped.  One-byte caches run
    quick_decode_rope_attention_fp8 with ``k_scale`` / ``v_scale``: the new token is appended as bytes and attended in that form.
    ``window`` (fp16 ring caches, see rope_kv_write): the token is appended at row pos % ring_rows and attends positions
    max(0, pos - window + 1) .. pos (quick_decode_rope_attention_win_f16).
    ``block_table`` (with ``page_size``; fp16 page pools, see rope_kv_write): the token is appended at its page and row and attends
    positions 0 .. pos, one table read per 16-row chunk (quick_decode_rope_attention_paged_f16)."""
    if block_table is not None:
        pages, psize, max_pages, table_rows = _paged(block_table, page_size, table_rows, k_cache, v_cache, cos_table, qkv.shape[0], window,
                                                     k_scale, v_scale, "rope_attention")
        if per_sequence:
            _per_sequence_pos(pos, qkv.shape[0], k_cache, "pos")
        rc = _lib.load().quick_decode_rope_attention_paged_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos.data_ptr(),
                                                               k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(),
                                                               block_table.data_ptr(), qkv.shape[0], n_heads, n_kv_heads, head_dim, pages,
                                                               psize, max_pages, table_rows, head_dim ** -0.5, int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return out
    if window is not None:
        window, ring, table_rows = _window(window, table_rows, k_cache, v_cache, cos_table, "rope_attention")
        if per_sequence:
            _per_sequence_pos(pos, qkv.shape[0], k_cache, "pos")
        rc = _lib.load().quick_decode_rope_attention_win_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos.data_ptr(),
                                                             k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), qkv.shape[0], n_heads,
                                                             n_kv_heads, head_dim, ring, window, table_rows, head_dim ** -0.5,
                                                             int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return out
    if _byte_caches(k_cache, v_cache):
        if per_sequence:
            _per_sequence_pos(pos, qkv.shape[0], k_cache, "pos")
        rc = _lib.load().quick_decode_rope_attention_fp8(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos.data_ptr(),
                                                         k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), qkv.shape[0], n_heads,
                                                         n_kv_heads, head_dim, k_cache.shape[2], head_dim ** -0.5, k_scale, v_scale,
                                                         int(per_sequence), _stream())
        if rc != _OK:
            _raise(rc)
        return out
    if per_sequence:
        _per_sequence_pos(pos, qkv.shape[0], k_cache, "pos")
        rc = _lib.load().quick_decode_rope_attention_seq_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos.data_ptr(),
                                                             k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), qkv.shape[0],
                                                             n_heads, n_kv_heads, head_dim, k_cache.shape[2], head_dim ** -0.5, _stream())
        if rc != _OK:
            raise RuntimeError(f"quick_decode_rope_attention_seq_f16 failed ({rc})")
        return out
    lib = _lib.load()
    rc = lib.quick_decode_rope_attention_f16(qkv.data_ptr(), cos_table.data_ptr(), sin_table.data_ptr(), pos.data_ptr(),
                                             k_cache.data_ptr(), v_cache.data_ptr(), out.data_ptr(), qkv.shape[0], n_heads,
                                             n_kv_heads, head_dim, k_cache.shape[2], head_dim ** -0.5, _stream())
    if rc != _OK:
        raise RuntimeError(f"quick_decode_rope_attention_f16 failed ({rc})")
    return out


def attention_describe(batch, n_heads, n_kv_heads, head_dim, cache_len, kv_cache_dtype="fp16"):
    """One line saying which kernel rope_attention runs for this shape (quick_decode_rope_attention_describe; host-only, no GPU needed).
    ``kv_cache_dtype="fp8_e4m3"``: the launch over one-byte caches (quick_decode_rope_attention_fp8_describe)."""
    if kv_cache_dtype not in ("fp16", "fp8_e4m3"):
        raise ValueError(f"attention_describe: kv_cache_dtype must be 'fp16' or 'fp8_e4m3', got {kv_cache_dtype!r}")
    buf = ctypes.create_string_buffer(128)
    fn = _lib.load().quick_decode_rope_attention_fp8_describe if kv_cache_dtype == "fp8_e4m3" else _lib.load().quick_decode_rope_attention_describe
    rc = fn(batch, n_heads, n_kv_heads, head_dim, cache_len, buf, len(buf))
    if rc != _OK:
        _raise(rc)
    return buf.value.decode()


def window_attention_describe(batch, tokens, n_heads, n_kv_heads, head_dim, ring_rows, window, table_rows):
    """One line describing the windowed attention launch for this shape (quick_attention_win_describe; host-only): tokens == 1 the
    decode launch, more tokens the prefill launch."""
    buf = ctypes.create_string_buffer(160)
    rc = _lib.load().quick_attention_win_describe(batch, tokens, n_heads, n_kv_heads, head_dim, ring_rows, window, table_rows, buf, len(buf))
    if rc != _OK:
        _raise(rc)
    return buf.value.decode()


def paged_attention_describe(batch, tokens, n_heads, n_kv_heads, head_dim, num_pages, page_size, max_pages, table_rows):
    """One line describing the paged attention launch for this shape (quick_attention_paged_describe; host-only): tokens == 1 the
    decode launch, more tokens the prefill launch."""
    buf = ctypes.create_string_buffer(160)
    rc = _lib.load().quick_attention_paged_describe(batch, tokens, n_heads, n_kv_heads, head_dim, num_pages, page_size, max_pages,
                                                    table_rows, buf, len(buf))
    if rc != _OK:
        _raise(rc)
    return buf.value.decode()


_LM_WS = {}


def lm_head_argmax(x, weight, norm_weight=None, eps=1e-5, want_hidden=False, want_logits=False):
    """Greedy next token of a decode step: argmax(RMSNorm(x) @ weight.T) in two launches (quick_lm_head_argmax_f16); x [B, H] fp16,
    weight [V, H] fp16, B <= 4.  Returns (next_token [B] int64, hidden [B, H] or None, logits [B, V] or None).  Raises
    NotImplementedError where the kernel has no build (the caller then runs torch)."""
    B, H = x.shape
    V = weight.shape[0]
    lib = _lib.load()
    key = (x.device.index, _stream(), B)   # per stream: two streams must not share the partial-key buffer
    if key not in _LM_WS:
        _LM_WS[key] = torch.empty(lib.quick_lm_head_workspace_bytes(B), dtype=torch.uint8, device=x.device)
    ws = _LM_WS[key]
    tok = torch.empty(B, dtype=torch.int64, device=x.device)
    hidden = torch.empty_like(x) if want_hidden else None
    logits = torch.empty((B, V), dtype=torch.float16, device=x.device) if want_logits else None
    rc = lib.quick_lm_head_argmax_f16(x.data_ptr(), norm_weight.data_ptr() if norm_weight is not None else None, eps, weight.data_ptr(),
                                      hidden.data_ptr() if hidden is not None else None,
                                      logits.data_ptr() if logits is not None else None, tok.data_ptr(), ws.data_ptr(), ws.numel(),
                                      B, V, H, _stream())
    if rc == 4:
        raise NotImplementedError("quick_lm_head_argmax_f16: batch <= 4, hidden % 512 == 0")
    if rc != _OK:
        raise RuntimeError(f"quick_lm_head_argmax_f16 failed ({rc})")
    return tok, hidden, logits


def prefetch(t, workgroups=0, stream=None):
    """Measurement aid: pull tensor `t` through HBM into the memory-side cache on `stream` (default: the current one); quick_prefetch."""
    st = _stream() if stream is None else stream.cuda_stream
    rc = _lib.load().quick_prefetch(t.data_ptr(), t.numel() * t.element_size(), workgroups, st)
    if rc != _OK:
        raise RuntimeError(f"quick_prefetch failed ({rc})")


def silu_mul(gate_up, out=None):
    """silu(gate) * up for the fused gate_up GEMM output [M, 2 I] (gate/up interleaved in blocks of 8) -> [M, I]."""
    lib = _lib.load()
    M, I = gate_up.shape[0], gate_up.shape[1] // 2
    out = torch.empty((M, I), dtype=torch.float16, device=gate_up.device) if out is None else out
    rc = lib.quick_silu_mul_f16(gate_up.data_ptr(), out.data_ptr(), M, I, _stream())
    if rc != _OK:
        raise RuntimeError(f"quick_silu_mul_f16 failed ({rc})")
    return out
