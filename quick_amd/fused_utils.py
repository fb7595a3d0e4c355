"""Packed-space concatenation of QUICK layers along the output dimension.

Counterpart of ``QUICK_cat`` / ``fuse_qkv_quick`` (quick/awq/utils/fused_utils.py:97-159), generalised to
layers of *different* widths (GQA: q 4096 / k 1024 / v 1024), which the reference rejects with
``ValueError("All input layers must have the same shape")`` (fused_utils.py:138-142) although its packed
format concatenates cleanly whenever every width is a multiple of 128: per (k-tile, quarter) segment the
128-channel blocks of the layers simply follow each other (closed form in SURVEY.md section 8(a)).
"""
from typing import Optional, Tuple

import torch

from . import kernels, packing
from .linear import WQLinear_QUICK
from .linear_gemm import WQLinear_GEMM


def QUICK_cat(*input_layers: torch.Tensor, options: str, reshape_dims: Optional[Tuple[int, int]] = None) -> torch.Tensor:
    """Concatenate reference-order packed tensors along N.  ``options`` in {'qweight', 'qzeros', 'scales'}.

    Same call signature as the reference.  ``reshape_dims``, when given, is applied to every input as in the
    reference (and therefore requires equal shapes); by default each input [H, W] is viewed as
    qweight -> (H/2, 2W), qzeros / scales -> (4H, W/4), which is what lets unequal widths through.
    """
    if len(input_layers) < 2:
        raise ValueError("At least two input layers are required")
    H = input_layers[0].shape[0]
    for layer in input_layers[1:]:
        if layer.shape[0] != H:
            raise ValueError("All input layers must have the same number of rows")
    if options not in ("qweight", "qzeros", "scales"):
        raise ValueError("Unknown options provided or invalid reshape dimensions")
    gran = {"qweight": 64, "qzeros": 32, "scales": 256}[options]      # columns per 128 output channels
    for layer in input_layers:
        if layer.shape[1] % gran != 0:
            raise ValueError("every layer must hold a multiple of 128 output channels")
    if reshape_dims is not None:
        parts = [layer.reshape(*reshape_dims) for layer in input_layers]
    elif options == "qweight":
        parts = [layer.reshape(H // 2, layer.shape[1] * 2) for layer in input_layers]
    else:
        parts = [layer.reshape(H * 4, layer.shape[1] // 4) for layer in input_layers]
    return torch.cat(parts, dim=1).reshape(H, -1)


def fuse_qkv_quick(module, q_proj, k_proj, v_proj):
    """One WQLinear_QUICK computing [q | k | v] (fused_utils.py:97-117); accepts unequal widths."""
    dev = q_proj.qweight.device if module is None else next(iter(module.state_dict().values())).device
    qkv_layer = WQLinear_QUICK(
        q_proj.w_bit, q_proj.group_size, q_proj.in_features,
        q_proj.out_features + k_proj.out_features + v_proj.out_features,
        q_proj.bias is not None, dev, q_proj.k_split_1, q_proj.k_split_2)
    packed = [p.reference_order() for p in (q_proj, k_proj, v_proj)]
    qkv_layer._set_packed(
        QUICK_cat(*[p[0] for p in packed], options="qweight").to(dev),
        QUICK_cat(*[p[1] for p in packed], options="scales").to(dev),
        QUICK_cat(*[p[2] for p in packed], options="qzeros").to(dev),
        prepared=False)
    qkv_layer.bias = torch.cat([q_proj.bias, k_proj.bias, v_proj.bias], dim=0) if q_proj.bias is not None else None
    return qkv_layer


def fuse_qkv_gemm(module, q_proj, k_proj, v_proj):
    """One WQLinear_GEMM computing [q | k | v]: the GEMM packing concatenates along dim 1 (eight channels per dword, every width a
    multiple of 8), so unequal widths are fine.  Works on ``state_dict``-order tensors, whatever the three modules hold now."""
    dev = q_proj.qweight.device if module is None else next(iter(module.state_dict().values())).device
    qkv_layer = WQLinear_GEMM(
        q_proj.w_bit, q_proj.group_size, q_proj.in_features,
        q_proj.out_features + k_proj.out_features + v_proj.out_features, q_proj.bias is not None, dev)
    packed = [p.awq_gemm_order() for p in (q_proj, k_proj, v_proj)]
    qkv_layer._set_packed(*[torch.cat([p[i] for p in packed], dim=1).to(dev) for i in range(3)], prepared=False)
    qkv_layer.bias = torch.cat([q_proj.bias, k_proj.bias, v_proj.bias], dim=0).to(dev) if q_proj.bias is not None else None
    return qkv_layer


# ---------------------------------------------------------------------------------------------- gate_proj + up_proj
def _mi355x_order(layer):
    """(qweight, scales, qzeros) of a WQLinear_QUICK / WQLinear_GEMM in MI355X order, by the path the module has for it; the module
    is left as it is (a prepared one hands out its own buffers)."""
    if layer.is_prepared:
        return layer.qweight, layer.scales, layer.qzeros
    if isinstance(layer, WQLinear_GEMM):
        return layer._to_mi355x(layer.qweight, layer.qzeros, layer.scales)
    if layer.qweight.is_cuda:
        return kernels.repack_cuda_to_mi355x(layer.qweight.contiguous(), layer.scales.contiguous(), layer.qzeros.contiguous())
    return packing.cuda_to_mi355x(layer.qweight, layer.scales, layer.qzeros)


def fuse_gate_up(gate_proj, up_proj):
    """One prepared WQLinear_QUICK of 2I output channels that interleave gate_proj's and up_proj's in blocks of 8 -- the layer
    ``kernels.gemm_forward(..., silu_mul=True)`` turns into silu(gate) * up in one launch (the intent of the reference's QuantFusedMLP,
    quick/awq/modules/fused/mlp.py:52-71).  The sources are WQLinear_QUICK or WQLinear_GEMM modules, prepared or not, on the GPU (one
    HIP launch interleaves them) or on the CPU (packing.interleave_gate_up_mi355x); the result shares no storage with them.
    ValueError: the two differ in in_features, out_features, group_size or bias presence.  NotImplementedError: in_features is not a
    multiple of 128 (a padded layer has no MI355X order of its own) or the width is outside the envelope."""
    for p in (gate_proj, up_proj):
        if not isinstance(p, (WQLinear_QUICK, WQLinear_GEMM)):
            raise TypeError(f"fuse_gate_up takes quick_amd.WQLinear_QUICK / WQLinear_GEMM modules, not {type(p).__name__}")
    for name in ("in_features", "out_features", "group_size", "w_bit"):
        if getattr(gate_proj, name) != getattr(up_proj, name):
            raise ValueError(f"gate_proj and up_proj differ in {name}: {getattr(gate_proj, name)} and {getattr(up_proj, name)}")
    if (gate_proj.bias is None) != (up_proj.bias is None):
        raise ValueError("gate_proj and up_proj differ in bias presence")
    dev = gate_proj.qweight.device
    if up_proj.qweight.device != dev:
        raise ValueError(f"gate_proj is on {dev}, up_proj on {up_proj.qweight.device}")
    K, I, G = gate_proj.in_features, gate_proj.out_features, gate_proj.group_size
    kernels.gate_up_shape_check(K, I, G)
    if I % 128 != 0:       # (inside the kernels' envelope, I % 64 == 0, but neither packing can hold one such projection)
        raise NotImplementedError(f"fuse_gate_up: a projection of {I} output channels has no MI355X order of its own (OC must be a multiple of 128)")
    gate, up = _mi355x_order(gate_proj), _mi355x_order(up_proj)
    fused = kernels.interleave_gate_up_mi355x(gate, up) if dev.type == "cuda" else packing.interleave_gate_up_mi355x(gate, up)
    has_bias = gate_proj.bias is not None
    # (device "meta": the constructor's buffers are placeholders, every one of them is replaced below)
    layer = WQLinear_QUICK(gate_proj.w_bit, G, K, 2 * I, has_bias, "meta", getattr(gate_proj, "k_split_1", 2), getattr(gate_proj, "k_split_2", 8))
    layer._set_packed(*fused, prepared=True)
    if has_bias:
        layer.bias = packing.interleave8(gate_proj.bias, up_proj.bias)
    return layer


def split_gate_up(layer, kind="quick"):
    """(gate_proj, up_proj) of a layer fuse_gate_up made -- the way back, for saving: prepared WQLinear_QUICK (``kind="quick"``) or
    WQLinear_GEMM (``"gemm"``) modules whose ``state_dict()`` tensors equal, bit for bit, those of the modules that were fused."""
    if kind not in ("quick", "gemm"):
        raise ValueError('kind must be "quick" or "gemm"')
    K, I, G = layer.in_features, layer.out_features // 2, layer.group_size
    kernels.gate_up_shape_check(K, I, G)
    fused = _mi355x_order(layer)
    if fused[0].is_cuda:
        parts = kernels.split_gate_up_mi355x(*[t.contiguous() for t in fused])
    else:
        parts = packing.split_gate_up_mi355x(*fused)
    bias = None if layer.bias is None else layer.bias.reshape(I // 8, 2, 8)
    out = []
    for h, (qw, sc, qz) in enumerate(parts):        # (device "meta": placeholders, all replaced)
        if kind == "quick":
            m = WQLinear_QUICK(layer.w_bit, G, K, I, bias is not None, "meta", layer.k_split_1, layer.k_split_2)
            m._set_packed(qw, sc, qz, prepared=True)
        else:
            m = WQLinear_GEMM(layer.w_bit, G, K, I, bias is not None, "meta")
            m._set_packed(qw, qz, sc, prepared=True)
        if bias is not None:
            m.bias = bias[:, h].reshape(I)
        out.append(m)
    return tuple(out)
