"""``QuantFusedMLP`` for MI355X: the constructor, attributes and ``forward(x, routing_weights=None)`` of the reference's module
(quick/awq/modules/fused/mlp.py:14-90), running gate_proj and up_proj as ONE W4A16 GEMM whose epilogue writes silu(gate) * up.

The reference keeps the two projections' buffers and launches two GEMMs plus an elementwise pass.  Here the constructor interleaves the
two layers' output channels in blocks of 8 (``fused_utils.fuse_gate_up``: one HIP launch on the GPU) into the child ``gate_up``, a
prepared ``WQLinear_QUICK`` of 2I channels, and drops its references to the sources -- the caller's own references are all that keeps
their memory.  ``unfuse()`` is the way back for saving.  Where the pair cannot be fused (in_features % 128 != 0: a padded layer has no
MI355X order of its own; a width outside the kernels' envelope) the module keeps ``gate_proj`` and ``up_proj`` and runs them as the
reference does, so construction never fails for a layer the reference accepts.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import kernels
from .fused_utils import fuse_gate_up, split_gate_up
from .linear_gemm import WQLinear_GEMM


class QuantFusedMLP(nn.Module):
    def __init__(self, gate_proj, down_proj, up_proj, activation=F.silu):
        super().__init__()
        self.in_features = gate_proj.in_features
        self.intermediate_size = gate_proj.out_features
        self.out_features = down_proj.out_features
        self.w_bit = gate_proj.w_bit
        self._kind = "gemm" if isinstance(gate_proj, WQLinear_GEMM) else "quick"      # what unfuse() hands back by default
        try:
            self.gate_up = fuse_gate_up(gate_proj, up_proj)
        except NotImplementedError:      # (a mismatched pair is a ValueError, raised before the envelope is looked at)
            self.gate_up = None
            self.gate_proj, self.up_proj = gate_proj, up_proj
        self.down_proj = down_proj
        self.activation = activation

    @property
    def is_fused(self):
        """True when gate_proj and up_proj live interleaved in the child ``gate_up``."""
        return self.gate_up is not None

    @property
    def silu_mul_epilogue(self):
        """True when forward() takes silu(gate) * up from the GEMM's epilogue: a fused pair, ``F.silu``, no bias.  Otherwise a fused pair
        runs one plain GEMM of width 2I (bias included) and the activation in torch."""
        return self.is_fused and self.activation is F.silu and self.gate_up.bias is None

    @torch.no_grad()
    def forward(self, x, routing_weights=None):
        I = self.intermediate_size
        out_shape = x.shape[:-1] + (I,)
        x = x.reshape(-1, x.shape[-1])
        if not self.is_fused:
            act = self.activation(self.gate_proj(x)) * self.up_proj(x)
        else:
            input_dtype = x.dtype
            x = x.to(torch.float16).contiguous()
            gu = self.gate_up
            if not gu.is_prepared:          # (rewritten from outside, e.g. load_state_dict: reference order again)
                gu.prepare()
            if self.silu_mul_epilogue:
                act = kernels.gemm_forward(x, gu.qweight, gu.scales, gu.qzeros, silu_mul=True)
            else:
                y = kernels.gemm_forward(x, gu.qweight, gu.scales, gu.qzeros, bias=gu.bias).view(-1, I // 8, 2, 8)
                act = (self.activation(y[:, :, 0]) * y[:, :, 1]).reshape(-1, I)
            if input_dtype != torch.float16:
                act = act.to(input_dtype)
        x = self.down_proj(act.reshape(out_shape))
        if routing_weights is not None:
            x = routing_weights * x
        return x

    def unfuse(self, kind=None):
        """(gate_proj, up_proj) as separate modules (``fused_utils.split_gate_up``): ``kind`` "quick" or "gemm", by default what the
        module was built from.  Their ``state_dict()`` tensors equal those of the modules given to the constructor bit for bit."""
        if not self.is_fused:
            return self.gate_proj, self.up_proj
        return split_gate_up(self.gate_up, kind or self._kind)


class QuantLlamaMLP(QuantFusedMLP):
    """Kept, like the reference's, for backward compatibility; use ``QuantFusedMLP``."""

    def __init__(self, gate_proj, down_proj, up_proj):
        super().__init__(gate_proj, down_proj, up_proj)
