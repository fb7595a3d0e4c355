"""``QuantAttentionFused`` for MI355X: the constructor, attributes and ``forward`` triple of the reference's module
(quick/awq/modules/fused/attn.py:100-245) on the HIP kernels of this package.  The module sits between the fused ``qkv_proj``
(``fuse_qkv_quick`` / ``fuse_qkv_gemm``) and ``o_proj`` and owns the KV cache and the position.

    one token  (T == 1)  qkv_proj | kernels.rope_attention (RoPE + cache append + single-query attention, one launch)    | o_proj
    T > 1, any start_pos qkv_proj | kernels.rope_kv_write (RoPE + cache write) | kernels.prefill_attention (causal, MFMA) | o_proj

No step reads a device value on the host and none builds a mask: the position the kernels use is a device int64 the module advances on
the device (``start_pos`` mirrors it on the host), so a forward can be captured in a graph, and a chunk of T > 1 tokens on top of a
non-empty cache (second chat turn, chunked prefill, speculative verify) attends the whole cache.

Envelope: inference, fp16, head_dim 128, rotate-half RoPE (HF convention, the reference's ``is_neox=True``).  Where the reference rolls
its cache, this module refuses: ``start_pos + T`` must not exceed ``max_seq_len`` -- the rows of the RoPE tables.

``sliding_window=W`` (opt-in; fp16 caches) makes the attention banded: the query at position p attends positions max(0, p - W + 1) .. p,
and the caches become RINGS of ``ring_rows(W, prefill_chunk, max_seq_len)`` rows in which position j lives in row ``ring_slot(j, rows)``.
Cache memory and the decode sweep are then bounded by the window, not by the context.  Keys keep the RoPE of their own absolute position
(the reference's ``roll_kv_n_steps`` shifts ``start_pos`` and so re-labels the cached keys; that is not copied).  A prompt goes in
chunks of at most ``prefill_chunk`` tokens: a chunk is written before it is attended, and with W + T - 1 <= rows the rows it
overwrites hold positions in front of every window of the chunk.  ``window_attention_reference`` restates the result in float64.

``per_sequence=True`` (a keyword of this package, not of the reference) gives every sequence of the batch its own position: ``pos`` is
int64 [batch], ``forward(..., new_tokens=...)`` says how many of the T rows of each sequence are real (right-padded), and
``reset(slots=[...])`` frees single slots.  The launches are the per-sequence forms of the same kernels; each sequence's workgroups sweep
its own length.  ``start_pos`` is then a host-side UPPER BOUND on the largest position, not the position.

``kv_cache_dtype="fp8_e4m3"`` (opt-in, the default stays ``"fp16"``) keeps the caches in one byte per element, OCP e4m3fn, with one scale
per cache: ``k_scale`` and ``v_scale``, host floats and constants of a captured graph.  ``quantize_kv`` / ``dequantize_kv`` below are the
format, restated in torch: the kernels store ``quantize_kv`` of the fp16 rows the fp16 module would store and attend their
``dequantize_kv`` -- the new token of a decode step included, so step p attends what step p + 1 reads.

``page_size=P, num_pages=N`` (opt-in; fp16, full attention) makes the cache PAGED: two pools ``[N, n_kv_heads, P, 128]`` and an int32
block table ``[batch, ceil(max_seq_len / P)]`` in which ``block_table[b][i]`` names the pool page of positions i P .. i P + P - 1 of
sequence b (-1: none).  A sequence holds ceil(length / P) pages, taken from a host-side ``PageAllocator`` as it grows and given back by
``reset``: memory is charged for the tokens alive, not for batch * max_seq_len.  ``paged_slot`` / ``gather_pages`` / ``scatter_pages``
restate the mapping in torch; the results are those of the linear module bit for bit.
"""
import math
import os

import torch
import torch.nn as nn

from . import kernels

HEAD_DIM = 128
KV_CACHE_DTYPES = {"fp16": torch.float16, "fp8_e4m3": torch.float8_e4m3fn}
FP8_MAX = 448.0


def _check_scale(scale, name):
    scale = float(scale)
    if not math.isfinite(scale) or scale <= 0.0:
        raise ValueError(f"{name} must be finite and positive, got {scale}")
    return scale


def _check_kv_cache(who, kv_cache_dtype, k_scale, v_scale):
    if kv_cache_dtype not in KV_CACHE_DTYPES:
        raise ValueError(f"{who}: kv_cache_dtype must be one of {sorted(KV_CACHE_DTYPES)}, got {kv_cache_dtype!r}")
    return KV_CACHE_DTYPES[kv_cache_dtype], _check_scale(k_scale, who + ": k_scale"), _check_scale(v_scale, who + ": v_scale")


def quantize_kv(x, scale):
    """The stored byte of the one-byte KV cache, as ``torch.float8_e4m3fn``: rne_e4m3(clamp(float(x) * inv, -448, 448)) with
    inv = 1.0f / scale in fp32.  ``x`` is the fp16 value the fp16 cache would hold; CPU or GPU.  The clamp is explicit (+-448.0001 and
    +-65504 saturate to +-448), ties go to the even code, NaN stays NaN."""
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(_check_scale(scale, "scale"), dtype=torch.float32)   # one fp32 division
    y = x.to(torch.float32) * inv.item()
    return torch.clamp(y, -FP8_MAX, FP8_MAX).to(torch.float8_e4m3fn)   # (clamp lets NaN through)


def dequantize_kv(b, scale):
    """float32(byte) * scale: the value the kernels attend.  ``b`` is ``torch.float8_e4m3fn`` or a ``uint8`` view of the same bytes."""
    if b.dtype == torch.uint8:
        b = b.view(torch.float8_e4m3fn)
    return b.to(torch.float32) * torch.tensor(_check_scale(scale, "scale"), dtype=torch.float32).item()


def ring_rows(window, prefill_chunk, max_seq_len):
    """Rows of the ring caches of a sliding window: min(max_seq_len, window + prefill_chunk - 1).  window + T - 1 rows let a chunk of
    T <= prefill_chunk tokens be written before it is attended without overwriting a row it attends; max_seq_len rows never wrap."""
    window, prefill_chunk, max_seq_len = int(window), int(prefill_chunk), int(max_seq_len)
    if window < 1 or prefill_chunk < 1 or max_seq_len < 1:
        raise ValueError(f"ring_rows: window, prefill_chunk and max_seq_len must be at least 1, got {window}, {prefill_chunk}, {max_seq_len}")
    return min(max_seq_len, window + prefill_chunk - 1)


def ring_slot(pos, ring_rows):
    """The cache row of position ``pos`` (an int, or an integer tensor of positions) in a ring of ``ring_rows`` rows: pos % ring_rows."""
    if int(ring_rows) < 1:
        raise ValueError(f"ring_slot: ring_rows must be at least 1, got {ring_rows}")
    return pos % int(ring_rows)


def window_attention_reference(q, k_ring, v_ring, pos0, window):
    """float64 banded-causal softmax(q K^T / sqrt(D)) V, the restatement of the windowed launches: q [B, nh, T, D] (rotated, as
    rope_kv_write leaves it), ring caches [B, nkv, R, D] in which position j lives in row ring_slot(j, R) and positions
    max(0, pos0 - window + 1) .. pos0 + T - 1 are present, pos0 an int or one int per sequence.  Query t attends positions
    max(0, pos0 + t - window + 1) .. pos0 + t: those rows are gathered out of the ring, and no other row is looked at.  Returns the
    kernels' row order, [B * T, nh * D], in float64.  CPU or GPU tensors."""
    B, nh, T, Dh = q.shape
    nkv, R = k_ring.shape[1], k_ring.shape[2]
    window = int(window)
    if window < 1 or nh % nkv != 0:
        raise ValueError("window_attention_reference: window must be at least 1 and n_heads a multiple of n_kv_heads")
    starts = [int(pos0)] * B if not isinstance(pos0, (list, tuple, torch.Tensor)) else [int(p) for p in pos0]
    if len(starts) != B or min(starts) < 0:
        raise ValueError(f"window_attention_reference: pos0 must be one non-negative position, or one per sequence ({B})")
    out = torch.empty((B, T, nh, Dh), dtype=torch.float64, device=q.device)
    scale = Dh ** -0.5
    for b, p0 in enumerate(starts):
        lo = max(0, p0 - window + 1)
        if p0 + T - lo > R:
            raise ValueError(f"window_attention_reference: positions {lo} .. {p0 + T - 1} do not fit a ring of {R} rows")
        span = torch.arange(lo, p0 + T, device=q.device)                                       # the positions any query of b attends
        K = k_ring[b][:, ring_slot(span, R)].double()                                          # [nkv, n, D]
        V = v_ring[b][:, ring_slot(span, R)].double()
        qp = p0 + torch.arange(T, device=q.device)[:, None]
        vis = (span[None, :] <= qp) & (span[None, :] > qp - window)                            # [T, n]
        s = torch.einsum("kgtd,knd->kgtn", q[b].double().view(nkv, nh // nkv, T, Dh), K) * scale
        P = torch.softmax(torch.where(vis, s, torch.full_like(s, float("-inf"))), -1)
        P = torch.where(vis, P, torch.zeros_like(P))                                           # (an exact 0: 0 * V stays 0)
        out[b] = torch.einsum("kgtn,knd->kgtd", P, V).reshape(nh, T, Dh).transpose(0, 1)
    return out.reshape(B * T, nh * Dh)


PAGE_SIZES = (32, 64, 128, 256)


def _check_page_size(page_size, who):
    if page_size not in PAGE_SIZES or int(page_size) != page_size:
        raise ValueError(f"{who}: page_size must be one of {PAGE_SIZES}, got {page_size!r}")
    return int(page_size)


def paged_slot(pos, block_table_row, page_size):
    """(page, row) of position ``pos`` (an int, or an integer tensor of positions) of the sequence whose block table row is
    ``block_table_row``: (block_table_row[pos // page_size], pos % page_size)."""
    P = _check_page_size(page_size, "paged_slot")
    col = pos // P
    if isinstance(col, torch.Tensor):
        return block_table_row[col.to(block_table_row.device)].long(), pos % P
    return int(block_table_row[col]), pos % P


def gather_pages(pool, block_table_row, length):
    """Positions 0 .. length - 1 of one sequence out of a pool [num_pages, nkv, P, D], as a linear [nkv, length, D] tensor; no page
    behind the last needed column of ``block_table_row`` is looked at."""
    P = pool.shape[2]
    pos = torch.arange(int(length), device=pool.device)
    page, row = paged_slot(pos, block_table_row, P)
    return pool[page, :, row].transpose(0, 1).contiguous()


def scatter_pages(pool, block_table_row, linear):
    """The inverse of gather_pages (for building fixtures): rows 0 .. length - 1 of ``linear`` [nkv, length, D] into their pool rows,
    in place; every other pool row keeps what it holds.  Returns ``pool``."""
    P = pool.shape[2]
    pos = torch.arange(linear.shape[1], device=pool.device)
    page, row = paged_slot(pos, block_table_row, P)
    pool[page, :, row] = linear.transpose(0, 1).to(pool.dtype)
    return pool


class PageAllocator:
    """A host-side free list over pages 0 .. num_pages - 1.  ``take(n)`` is all-or-nothing; ``give(pages)`` returns pages for reuse."""

    def __init__(self, num_pages):
        if int(num_pages) != num_pages or num_pages < 1:
            raise ValueError(f"PageAllocator: num_pages must be a whole number >= 1, got {num_pages!r}")
        self.num_pages = int(num_pages)
        self._free = list(range(self.num_pages - 1, -1, -1))     # (a stack: page 0 goes out first, a page given back is reused first)

    @property
    def free(self):
        return len(self._free)

    def take(self, n):
        n = int(n)
        if n < 0:
            raise ValueError(f"PageAllocator: cannot take {n} pages")
        if n > len(self._free):
            raise RuntimeError(f"PageAllocator: out of pages: {len(self._free)} of {self.num_pages} are free, {n} were asked for")
        return [self._free.pop() for _ in range(n)]

    def give(self, pages):
        pages = [int(p) for p in pages]
        held = set(self._free)
        if len(set(pages)) != len(pages) or any(p < 0 or p >= self.num_pages or p in held for p in pages):
            raise ValueError(f"PageAllocator: give({pages}): pages must be distinct, inside 0 .. {self.num_pages - 1} and not free already")
        self._free.extend(reversed(pages))


class QuantAttentionFused(nn.Module):
    def __init__(self, hidden_size, n_heads, n_kv_heads, qkv_layer, o_proj, dev, max_seq_len, use_alibi=False, attention_shapes=None,
                 rope_theta=10000, per_sequence=False, kv_cache_dtype="fp16", k_scale=1.0, v_scale=1.0, sliding_window=None,
                 prefill_chunk=512, page_size=None, num_pages=None):
        super().__init__()
        _, k_scale, v_scale = _check_kv_cache("QuantAttentionFused", kv_cache_dtype, k_scale, v_scale)
        if prefill_chunk is None or int(prefill_chunk) != prefill_chunk or prefill_chunk < 1:
            raise ValueError(f"QuantAttentionFused: prefill_chunk must be a whole number >= 1, got {prefill_chunk!r}")
        if sliding_window is not None:
            if int(sliding_window) != sliding_window or sliding_window < 1:
                raise ValueError(f"QuantAttentionFused: sliding_window must be a whole number >= 1 (or None), got {sliding_window!r}")
            if kv_cache_dtype != "fp16":
                raise ValueError("QuantAttentionFused: sliding_window needs kv_cache_dtype='fp16' (a window over one-byte caches is not supported)")
        if page_size is not None:
            page_size = _check_page_size(page_size, "QuantAttentionFused")
            if sliding_window is not None:
                raise ValueError("QuantAttentionFused: page_size with sliding_window is not supported (a windowed paged cache is out of scope)")
            if kv_cache_dtype != "fp16":
                raise ValueError("QuantAttentionFused: page_size needs kv_cache_dtype='fp16' (a paged one-byte cache is out of scope)")
            if num_pages is None or int(num_pages) != num_pages or num_pages < 1:
                raise ValueError(f"QuantAttentionFused: page_size needs num_pages, a whole number >= 1, got {num_pages!r}")
        elif num_pages is not None:
            raise ValueError("QuantAttentionFused: num_pages needs page_size")
        if use_alibi:
            raise ValueError("QuantAttentionFused: use_alibi=True is not supported (the kernels rotate q and k, they add no ALiBi bias)")
        if attention_shapes is not None:
            raise ValueError("QuantAttentionFused: custom attention_shapes are not supported (the kernels take [q | k | v] of the fused qkv layer)")
        if n_heads <= 0 or n_kv_heads <= 0 or n_heads % n_kv_heads != 0:
            raise ValueError(f"QuantAttentionFused: n_heads ({n_heads}) must be a positive multiple of n_kv_heads ({n_kv_heads})")
        if hidden_size % n_heads != 0 or hidden_size // n_heads != HEAD_DIM:
            raise ValueError(f"QuantAttentionFused: head_dim must be {HEAD_DIM}, hidden_size // n_heads is {hidden_size // n_heads}")
        width = (n_heads + 2 * n_kv_heads) * HEAD_DIM
        if qkv_layer.out_features != width or qkv_layer.in_features != hidden_size:
            raise ValueError(f"QuantAttentionFused: qkv_layer must map {hidden_size} to (n_heads + 2 n_kv_heads) * {HEAD_DIM} = {width} "
                             f"channels, it maps {qkv_layer.in_features} to {qkv_layer.out_features}")
        if o_proj.in_features != hidden_size:
            raise ValueError(f"QuantAttentionFused: o_proj must take {hidden_size} channels, it takes {o_proj.in_features}")
        if max_seq_len <= 0:
            raise ValueError("QuantAttentionFused: max_seq_len must be positive")
        self.hidden_size = hidden_size
        self.n_heads = n_heads
        self.n_kv_heads = n_kv_heads
        self.n_kv_groups = n_heads // n_kv_heads
        self.head_dim = HEAD_DIM
        self.qkv_proj = qkv_layer
        self.o_proj = o_proj
        self.start_pos = 0
        self.use_alibi = False
        self.cache_batch_size = int(os.getenv("AWQ_BATCH_SIZE", "1"))
        self.max_seq_len = max_seq_len
        self.is_hf_transformers = False
        self.rope_theta = rope_theta
        self.rotary_dim = HEAD_DIM
        self.is_neox = True
        # state, not parameters: plain attributes, absent from state_dict()
        dev = torch.device(dev)
        inv = 1.0 / (rope_theta ** (torch.arange(0, HEAD_DIM, 2, device=dev).float() / HEAD_DIM))
        ang = torch.outer(torch.arange(max_seq_len, device=dev).float(), inv)
        self.cos = torch.cat((ang.cos(), ang.cos()), -1).half()
        self.sin = torch.cat((ang.sin(), ang.sin()), -1).half()
        self.per_sequence = bool(per_sequence)
        self.kv_cache_dtype, self.k_scale, self.v_scale = kv_cache_dtype, k_scale, v_scale
        self.sliding_window = None if sliding_window is None else int(sliding_window)
        self.prefill_chunk = int(prefill_chunk)
        # rows per sequence and KV head: the whole context, or a ring bounded by the window (max_seq_len stays the position bound)
        self.cache_rows = max_seq_len if sliding_window is None else ring_rows(sliding_window, prefill_chunk, max_seq_len)
        # paged: the pools stand in k_cache / v_cache ([num_pages, nkv, P, D]); the block table, the allocator and the bounds come with them
        self.page_size = page_size
        self.num_pages = None if page_size is None else int(num_pages)
        self.pos = torch.zeros(1, dtype=torch.int64, device=dev)
        self._allocate(self.cache_batch_size, dev)

    def _allocate(self, batch, dev):
        shape = (batch, self.n_kv_heads, self.cache_rows, HEAD_DIM)
        if self.page_size is not None:
            shape = (self.num_pages, self.n_kv_heads, self.page_size, HEAD_DIM)
            self.max_pages = -(-self.max_seq_len // self.page_size)
            self._table_host = torch.full((batch, self.max_pages), -1, dtype=torch.int32)
            self.block_table = self._table_host.to(dev)
            self.allocator = PageAllocator(self.num_pages)
            self._pages = [[] for _ in range(batch)]             # the pages of every sequence, in position order
            self._len_bound = [0] * batch                        # host-side upper bound of every sequence's length
        self.k_cache = torch.zeros(shape, dtype=KV_CACHE_DTYPES[self.kv_cache_dtype], device=dev)
        self.v_cache = torch.zeros(shape, dtype=KV_CACHE_DTYPES[self.kv_cache_dtype], device=dev)
        self.cache_batch_size = batch
        if self.per_sequence:                                   # one position per sequence, re-made with the caches
            self.pos = torch.zeros(batch, dtype=torch.int64, device=dev)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        for name in ("cos", "sin", "k_cache", "v_cache"):       # (.to() / .cuda() move the state along with the projections)
            t = getattr(self, name)
            if t.dtype == torch.float8_e4m3fn:                  # a byte cache moves as bytes: fn may be a dtype cast (.half())
                setattr(self, name, fn(t.view(torch.uint8)).to(torch.uint8).view(torch.float8_e4m3fn))
            else:
                setattr(self, name, fn(t).half())
        self.pos = fn(self.pos).to(torch.int64)
        if self.page_size is not None:
            self.block_table = fn(self.block_table).to(torch.int32)
        return self

    # ------------------------------------------------------------------------------------------ paged cache: host-side bookkeeping
    @property
    def k_pool(self):
        return self.k_cache

    @property
    def v_pool(self):
        return self.v_cache

    @property
    def free_pages(self):
        """Pages of the pool no sequence holds."""
        self._need_pages("free_pages")
        return self.allocator.free

    def _need_pages(self, what):
        if self.page_size is None:
            raise ValueError(f"QuantAttentionFused: {what} needs a paged cache (page_size=...)")

    @staticmethod
    def _capturing():
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def _push_table(self):
        self.block_table.copy_(self._table_host)                 # in place, at the same address: a captured graph reads the new table

    def reserve(self, lengths):
        """Make sure sequence b holds the pages of positions 0 .. lengths[b] - 1 (an int: every sequence) -- what ``forward`` does for the
        tokens it is given, done ahead of time: a captured step allocates nothing, so call this before the capture and between replays.
        All or nothing: RuntimeError when the pool has too few free pages, and then nothing has changed.  Never gives pages back."""
        self._need_pages("reserve")
        B = self.cache_batch_size
        lengths = [int(lengths)] * B if not isinstance(lengths, (list, tuple, torch.Tensor)) else [int(n) for n in lengths]
        if len(lengths) != B or any(n < 0 or n > self.max_seq_len for n in lengths):
            raise ValueError(f"QuantAttentionFused: reserve: one length in 0 .. max_seq_len = {self.max_seq_len} per sequence ({B}), got {lengths}")
        need = [max(0, -(-n // self.page_size) - len(held)) for n, held in zip(lengths, self._pages)]
        if not any(need):
            return
        if self._capturing():
            raise RuntimeError(f"QuantAttentionFused: {sum(need)} pages are missing while a stream is capturing, and a captured step "
                               "allocates nothing: call reserve(lengths) before the capture (and between replays)")
        try:
            got = self.allocator.take(sum(need))
        except RuntimeError as e:
            raise RuntimeError(f"QuantAttentionFused: the page pool is exhausted ({e}); free slots with reset(slots=...) or build the "
                               "module with more num_pages") from None
        for b, n in enumerate(need):
            mine, got = got[:n], got[n:]
            self._table_host[b, len(self._pages[b]):len(self._pages[b]) + n] = torch.tensor(mine, dtype=torch.int32)
            self._pages[b] += mine
        self._push_table()

    def _release(self, slots):
        for b in slots:
            self.allocator.give(self._pages[b])
            self._pages[b] = []
            self._len_bound[b] = 0
            self._table_host[b] = -1
        self._push_table()

    def reset(self, slots=None):
        """Back to position 0 (the cache rows are overwritten as the positions are).  ``slots`` (``per_sequence=True`` only): the indices
        of the sequences to restart -- a finished slot takes a new request while the others go on; ``start_pos`` is then recomputed as
        the largest remaining position (one host read, here and nowhere in ``forward``)."""
        if slots is None:
            self.start_pos = 0
            self.pos.zero_()
            if self.page_size is not None:                      # every page goes back, every table row to -1
                self._release(range(self.cache_batch_size))
            return
        if not self.per_sequence:
            raise ValueError("QuantAttentionFused: reset(slots=...) needs per_sequence=True (this module keeps one position for the batch)")
        slots = [int(i) for i in slots]
        if any(i < 0 or i >= self.cache_batch_size for i in slots):
            raise ValueError(f"QuantAttentionFused: reset(slots={slots}): slots are 0 .. {self.cache_batch_size - 1}")
        if slots:
            self.pos[torch.tensor(slots, dtype=torch.int64, device=self.pos.device)] = 0
        if self.page_size is not None:                          # (the host read below makes the other slots' bounds exact again)
            self._release(sorted(set(slots)))
            self._len_bound = [int(p) for p in self.pos.tolist()]
        self.start_pos = int(self.pos.max())

    def _new_tokens(self, new_tokens, B, T):
        """-> (device int64 [B] to add to pos, or None for T everywhere; what start_pos advances by).  A list, a tuple or a CPU tensor
        is checked here, on the host; a device tensor is taken as it is (its values are never read on the host)."""
        if new_tokens is None:
            return None, T
        if isinstance(new_tokens, torch.Tensor) and new_tokens.is_cuda:
            if new_tokens.dtype != torch.int64 or new_tokens.numel() != B or not new_tokens.is_contiguous():
                raise ValueError(f"QuantAttentionFused: a device new_tokens must be a contiguous int64 tensor of {B} elements")
            return new_tokens.view(B), T
        counts = new_tokens.tolist() if isinstance(new_tokens, torch.Tensor) else list(new_tokens)
        if len(counts) != B:
            raise ValueError(f"QuantAttentionFused: new_tokens has {len(counts)} entries, the batch has {B} sequences")
        if any(int(c) != c or c < 0 or c > T for c in counts):
            raise ValueError(f"QuantAttentionFused: new_tokens must be whole numbers in 0 .. T = {T} (right-padded rows), got {counts}")
        counts = [int(c) for c in counts]
        return torch.tensor(counts, dtype=torch.int64), max(counts)

    @torch.no_grad()
    def forward(self, hidden_states, attention_mask=None, *args, new_tokens=None, **kwargs):
        """hidden_states [B, T, hidden] fp16 -> (attn_output [B, T, hidden], attention_weight [B, T, hidden] = the attention output in
        front of o_proj, past_key_value = [torch.zeros(1, 1, start_pos, 1)]), the reference's triple.

        The module applies causal masking itself: ``attention_mask`` is accepted and IGNORED, as the reference's single-token path
        ignores it.  A batch size other than the cache's reallocates the caches and
        restarts at position 0, as the reference does.  ValueError where ``start_pos + T`` would exceed ``max_seq_len`` (the
        reference rolls its cache and re-labels the cached keys; this module refuses at the last row of its RoPE tables -- with
        ``sliding_window`` the caches are rings bounded by the window, and that is the only limit on the context).

        ``sliding_window=W``: query at position p attends positions max(0, p - W + 1) .. p; all four paths run the windowed launches.
        On a ring smaller than ``max_seq_len`` a forward takes at most ``prefill_chunk`` tokens (ValueError otherwise): feed a longer
        prompt in chunks.  In ``per_sequence`` mode the padded rows of a chunk are written too and land behind the sequence's new
        position, which in a wrapped ring are its OLDEST rows: the padding of a chunk counts toward T in W + T - 1 <= rows, and
        ``prefill_chunk`` bounds T with its padding.

        Ragged batches need ``per_sequence=True``: ``new_tokens`` [B] says how many of the T rows of each sequence are real tokens
        (0 .. T, RIGHT-padded; None: T for all).  A list, a tuple or a CPU tensor is validated on the host (ValueError); a device int64
        [B] tensor is used as it is, without a host read, so the step can be captured in a graph.  Sequence b's rows go to cache rows
        pos[b] .. pos[b] + T - 1 and ``pos += new_tokens`` afterwards: its padding rows lie behind its new position, where the kernels
        never read, and the next forward overwrites them; the OUTPUT rows of padding are unspecified.  ``new_tokens[b] == 0`` is an
        idle step, the position stays.  ``start_pos`` advances by max(new_tokens) where the counts are known on the host and by T
        otherwise: an upper bound on the largest position, which the overflow check and ``past_key_value`` use -- a padded chunk needs
        room for its padding.  ``attention_mask`` stays ignored in this mode too, and LEFT-padded batches are out of scope."""
        B, T, _ = hidden_states.shape
        if new_tokens is not None and not self.per_sequence:
            raise ValueError("QuantAttentionFused: new_tokens needs per_sequence=True (this module keeps one position for the batch)")
        if B != self.cache_batch_size:
            self._allocate(B, self.k_cache.device)
            self.reset()
        if self.is_hf_transformers and "past_key_value" in kwargs and kwargs["past_key_value"] is None:
            self.reset()                    # (the first step of a new generate())
        if self.start_pos + T > self.max_seq_len:
            raise ValueError(f"QuantAttentionFused: start_pos + tokens = {self.start_pos} + {T} exceeds max_seq_len = {self.max_seq_len}; "
                             "the cache does not roll, call reset() or build the module with a larger max_seq_len"
                             + ("; a padded chunk needs room for its padding (all T rows of every sequence are written), and start_pos "
                                "is an upper bound on the positions" if self.per_sequence else ""))
        if self.sliding_window is not None and self.cache_rows < self.max_seq_len and T > self.prefill_chunk:
            raise ValueError(f"QuantAttentionFused: {T} tokens in one forward on a ring of {self.cache_rows} rows (sliding_window = "
                             f"{self.sliding_window}): feed the prompt in chunks of at most prefill_chunk = {self.prefill_chunk} tokens"
                             + (" (padding included)" if self.per_sequence else ""))
        step, advance = self._new_tokens(new_tokens, B, T) if self.per_sequence else (None, T)
        if not hidden_states.is_cuda:
            raise RuntimeError("hidden_states must be a GPU tensor: the attention kernels have no CPU implementation")
        nh, nkv = self.n_heads, self.n_kv_heads
        ks = {} if self.kv_cache_dtype == "fp16" else dict(k_scale=self.k_scale, v_scale=self.v_scale)   # byte caches: the fp8 launches
        if self.sliding_window is not None:                                                              # ring caches: the windowed launches
            ks = dict(window=self.sliding_window, table_rows=self.max_seq_len)
        if self.page_size is not None:                                                                   # page pools: the paged launches
            # the pages of every sequence's bound plus its new tokens, before any launch; exact where the counts are host integers
            counts = [T] * B if step is None or step.is_cuda else step.tolist()
            grown = [min(n + c, self.max_seq_len) for n, c in zip(self._len_bound, counts)]
            self.reserve(grown)
            self._len_bound = grown
            ks = dict(block_table=self.block_table, page_size=self.page_size, table_rows=self.max_seq_len)
        qkv = self.qkv_proj(hidden_states.reshape(B * T, self.hidden_size).contiguous())
        att = torch.empty((B * T, nh * HEAD_DIM), dtype=torch.float16, device=qkv.device)
        if self.per_sequence:
            if T == 1:
                kernels.rope_attention(qkv, self.cos, self.sin, self.pos, self.k_cache, self.v_cache, att, nh, nkv, HEAD_DIM, per_sequence=True, **ks)
            else:
                q = torch.empty((B, nh, T, HEAD_DIM), dtype=torch.float16, device=qkv.device)
                kernels.rope_kv_write(qkv, self.cos, self.sin, self.pos, q, self.k_cache, self.v_cache, T, nh, nkv, HEAD_DIM, per_sequence=True, **ks)
                kernels.prefill_attention(q, self.k_cache, self.v_cache, self.pos, att, nh, nkv, HEAD_DIM, per_sequence=True, **ks)
            attn_output = self.o_proj(att).view(B, T, -1)
            if step is None:
                self.pos.add_(T)
            else:
                self.pos.add_(step.to(self.pos.device, non_blocking=True))
            self.start_pos += advance
            return attn_output, att.view(B, T, nh * HEAD_DIM), [torch.zeros(1, 1, self.start_pos, 1)]
        if T == 1:
            kernels.rope_attention(qkv, self.cos, self.sin, self.pos, self.k_cache, self.v_cache, att, nh, nkv, HEAD_DIM, **ks)
        else:
            q = torch.empty((B, nh, T, HEAD_DIM), dtype=torch.float16, device=qkv.device)
            kernels.rope_kv_write(qkv, self.cos, self.sin, self.pos, q, self.k_cache, self.v_cache, T, nh, nkv, HEAD_DIM, **ks)
            kernels.prefill_attention(q, self.k_cache, self.v_cache, self.pos, att, nh, nkv, HEAD_DIM, **ks)
        attn_output = self.o_proj(att).view(B, T, -1)
        self.pos.add_(T)
        self.start_pos += T
        return attn_output, att.view(B, T, nh * HEAD_DIM), [torch.zeros(1, 1, self.start_pos, 1)]
