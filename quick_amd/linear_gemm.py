"""``WQLinear_GEMM`` for MI355X: the operator published AWQ checkpoints are saved from, with the constructor, ``from_linear``,
buffer names, shapes, dtypes and ``extra_repr`` of the reference's (quick/awq/modules/linear/gemm.py:13-63, 189-197), running on
the same HIP GEMM as ``WQLinear_QUICK``.

Layout contract (the mirror of linear.py's)
-------------------------------------------
* ``state_dict()`` / ``load_state_dict()`` always speak the GEMM packing and its shapes: qweight int32 [K, N/8], qzeros int32
  [K/G, N/8] (nibble i of dword c = channel 8c + [0,2,4,6,1,3,5,7][i]), scales fp16 [K/G, N].
* In memory, after :meth:`prepare` (run lazily by the first ``forward``), the three buffers hold the same bits in MI355X order,
  whose shapes differ: qweight [K/4, N/2], scales [K/G, 2N], qzeros [K/G, N/4].  The conversion is a permutation -- lossless both
  ways -- done by one HIP repack launch per layer on the GPU and by ``packing`` on CPU tensors.
* in_features % 128 != 0 (only with group sizes that are not multiples of 128): the MI355X order cannot tile the layer, and a
  padded copy is never turned back.  The buffers keep the GEMM packing, and ``forward`` runs on a zero-padded MI355X-order copy
  held beside them -- made once, dropped when the buffers are rewritten -- with ``x`` zero-padded to the same width.
"""
import torch
import torch.nn as nn

from . import kernels, packing
from .linear import _Layout


class _PaddedCopy:
    """The MI355X-order copy of a layer whose in_features the order cannot tile, and the key of the buffers it was made from.  Not
    state: copies and pickles of the module start without it."""
    __slots__ = ("key", "packed")

    def __init__(self, key=None, packed=None):
        self.key, self.packed = key, packed

    def __deepcopy__(self, memo):
        return _PaddedCopy()

    def __reduce__(self):
        return (_PaddedCopy, ())


class WQLinear_GEMM(nn.Module):
    def __init__(self, w_bit, group_size, in_features, out_features, bias, dev):
        super().__init__()
        if w_bit not in [4]:
            raise NotImplementedError("Only 4-bit are supported for now.")
        self.in_features = in_features
        self.out_features = out_features
        self.w_bit = w_bit
        self.group_size = group_size if group_size != -1 else in_features
        assert self.in_features % self.group_size == 0
        assert out_features % (32 // self.w_bit) == 0
        pack = 32 // self.w_bit
        self.register_buffer("qweight", torch.zeros((in_features, out_features // pack), dtype=torch.int32, device=dev))
        self.register_buffer("qzeros", torch.zeros((in_features // self.group_size, out_features // pack), dtype=torch.int32, device=dev))
        self.register_buffer("scales", torch.zeros((in_features // self.group_size, out_features), dtype=torch.float16, device=dev))
        if bias:
            self.register_buffer("bias", torch.zeros((out_features), dtype=torch.float16, device=dev))
        else:
            self.bias = None
        self._layout = _Layout()
        self._padded = _PaddedCopy()

    # ---------------------------------------------------------------- layout tracking
    def _key(self):
        return tuple((t.data_ptr(), 0 if t.is_inference() else t._version, t.device) for t in (self.qweight, self.qzeros, self.scales))

    @property
    def is_prepared(self):
        """True when the buffers currently hold MI355X order (and its shapes)."""
        lay = self._layout
        if not lay.prepared:
            return False
        if lay.key is None:                 # a copy / unpickled module: same bits in new storages
            lay.key = self._key()
        elif lay.key != self._key():        # rewritten from outside: GEMM packing again
            lay.prepared, lay.key = False, None
        return lay.prepared

    def _set_packed(self, qweight, qzeros, scales, prepared):
        self.qweight, self.qzeros, self.scales = qweight, qzeros, scales
        self._layout = _Layout(prepared, self._key() if prepared else None)
        self._padded = _PaddedCopy()

    @staticmethod
    def _to_mi355x(qweight, qzeros, scales):
        if qweight.is_cuda:
            return kernels.repack_awq_gemm_to_mi355x(qweight.contiguous(), qzeros.contiguous(), scales.contiguous())
        return packing.awq_gemm_to_mi355x(qweight, qzeros, scales)

    def prepare(self):
        """Permute GEMM-packing buffers into MI355X order (one HIP repack launch on the GPU)."""
        if self.is_prepared or self.in_features % 128 != 0:   # (K % 128 != 0: stays in the GEMM packing, see forward)
            return self
        qw, sc, qz = self._to_mi355x(self.qweight, self.qzeros, self.scales)
        self._set_packed(qw, qz, sc, prepared=True)
        return self

    def awq_gemm_order(self):
        """(qweight, qzeros, scales) in the GEMM packing, whatever the buffers hold now."""
        if not self.is_prepared:
            return self.qweight, self.qzeros, self.scales
        if self.qweight.is_cuda:
            return kernels.repack_mi355x_to_awq_gemm(self.qweight, self.scales, self.qzeros)
        return packing.mi355x_to_awq_gemm(self.qweight, self.scales, self.qzeros)

    def _padded_mi355x(self):
        """The zero-padded MI355X-order copy of a layer with in_features % 128 != 0, made once per content of the buffers."""
        key = self._key()
        if self._padded.packed is None or self._padded.key != key:
            self._padded = _PaddedCopy(key, self._to_mi355x(self.qweight, self.qzeros, self.scales))
        return self._padded.packed

    def _apply(self, fn, *args, **kwargs):
        was = self.is_prepared
        super()._apply(fn, *args, **kwargs)
        self._layout = _Layout(was, self._key() if was else None)   # .to()/.cuda() move bits, they do not reorder them
        self._padded = _PaddedCopy()
        return self

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        # Checkpoints hold the GEMM packing, whose SHAPES differ from the prepared buffers': a prepared module goes back to GEMM-packing
        # buffers first (also on a partial load: the orders must not mix), so that nn.Module's shape checks pass and its in-place copies
        # land in the right packing.  The load itself marks the module unprepared (see WQLinear_QUICK._load_from_state_dict for why the
        # version counters are not left to notice it).
        if any(prefix + n in state_dict for n in ("qweight", "scales", "qzeros")):
            if self.is_prepared:
                self._set_packed(*self.awq_gemm_order(), prepared=False)
            self._layout = _Layout(False)
            self._padded = _PaddedCopy()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        super()._save_to_state_dict(destination, prefix, keep_vars)
        if self.is_prepared:
            qw, qz, sc = self.awq_gemm_order()
            destination[prefix + "qweight"], destination[prefix + "qzeros"], destination[prefix + "scales"] = qw, qz, sc

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_linear(cls, linear, w_bit, group_size, init_only=False, scales=None, zeros=None):
        """``scales`` / ``zeros`` are [K/G, N] as in the reference's WQLinear_GEMM.from_linear (gemm.py:65-145) -- the transpose of what
        WQLinear_QUICK.from_linear takes."""
        awq_linear = cls(w_bit, group_size, linear.in_features, linear.out_features, linear.bias is not None, linear.weight.device)
        if init_only:  # just prepare for loading sd
            return awq_linear
        assert scales is not None and zeros is not None
        if linear.bias is not None:
            awq_linear.bias = linear.bias.clone().half()
        intweight = packing.quantize_intweight(linear.weight.data, scales.t(), zeros.t(), awq_linear.group_size)   # [K, N]
        awq_linear._set_packed(*packing.pack_awq_gemm(intweight, scales.half(), zeros.to(torch.int32)), prepared=False)
        return awq_linear

    # ---------------------------------------------------------------- forward
    @torch.no_grad()
    def forward(self, x):
        out_shape = x.shape[:-1] + (self.out_features,)
        input_dtype = x.dtype
        if input_dtype != torch.float16:
            x = x.half()
        x = x.reshape(-1, x.shape[-1])
        if self.in_features % 128 != 0:
            qweight, scales, qzeros = self._padded_mi355x()
            x = torch.nn.functional.pad(x, (0, qweight.shape[0] * 4 - self.in_features))
        else:
            if not self.is_prepared:
                self.prepare()
            qweight, scales, qzeros = self.qweight, self.scales, self.qzeros
        out = kernels.gemm_forward(x.contiguous(), qweight, scales, qzeros, bias=self.bias)
        if input_dtype != torch.float16:
            out = out.to(dtype=input_dtype)
        return out.reshape(out_shape)

    def extra_repr(self) -> str:
        return "in_features={}, out_features={}, bias={}, w_bit={}, group_size={}".format(
            self.in_features, self.out_features, self.bias is not None, self.w_bit, self.group_size)
