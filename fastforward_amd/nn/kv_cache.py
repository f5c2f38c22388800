"""A preallocated, quantized KV cache for a decode loop (no counterpart in the reference, which never decodes).

``QuantizedKVCache`` owns two int8 buffers ``[B, H, S_max, E]`` and the lengths of its sequences as an int32 tensor ON THE DEVICE.
``append`` advances the lengths with an ordinary ``add_`` and quantizes the new K / V rows into place in one launch
(``ops.kv_append``); ``attend`` is one ``ops.kv_decode`` call that reads the lengths on the device. Nothing reads a length on the host
and no shape moves from step to step, so ``append`` + ``attend`` can be captured once in a ``torch.cuda.graph`` and replayed while the
sequences grow, each at its own length. ``is_causal`` is bottom-right: the L new queries sit at the END of the cache.

``composed_append`` / ``composed_attend`` run the same semantics from existing pieces (torch ops for the rotation, the quantizer
modules, an indexed copy per batch, ``scaled_dot_product_attention`` per batch on the slices with a bottom-right bool mask). They read
the lengths on the host: they are the chain the kernels are tested against and what the class runs on host tensors or with a library
that lacks the entry points, not a fast path.

``PagedQuantizedKVCache`` keeps the same codes in fixed-size pages of two pools behind a per-sequence block table on the device
(``ops.kv_paged_append`` / ``ops.kv_paged_decode``, include/ffq_kv_paged.h): a sequence owns only the pages it uses, a finished one
gives them back without a copy, and sequences can share the pages of a common prefix. Its page bookkeeping is host code that runs
outside a captured step; ``composed_paged_append`` / ``composed_paged_attend`` gather the pages into a dense view and run the chain above.

``DynamicQuantizedKVCache`` is the dense cache with two ``DynamicLinearQuantizer``s: every appended row gets its own
``(scale, offset)``, computed on the device from the row's min / max and kept in an fp32 store ``[B, H, S_max, 4]`` beside the codes
(``ops.kv_token_append`` / ``ops.kv_token_decode``, include/ffq_kv_token.h), so nothing is calibrated ahead of serving.
``composed_token_append`` / ``composed_token_attend`` are its chain from the quantizer modules themselves.

``PagedDynamicQuantizedKVCache`` is both: the pages and the bookkeeping of ``PagedQuantizedKVCache`` (``_PagedBase`` states them once)
with two ``DynamicLinearQuantizer``s, every row's ``(scale, offset)`` kept in a third pool ``[num_pages, H, P, 4]`` of the same pages
(``ops.kv_paged_token_append`` / ``ops.kv_paged_token_decode``, include/ffq_kv_paged_token.h), so a shared prefix page shares its
parameters. ``composed_paged_token_append`` / ``composed_paged_token_attend`` gather the pages and run the dense per-row chain.
"""

from __future__ import annotations

from typing import Any, Sequence

import torch

from fastforward_amd import _native, ops
from fastforward_amd.nn.dynamic_linear_quantizer import DynamicLinearQuantizer
from fastforward_amd.nn.linear_quantizer import LinearQuantizer
from fastforward_amd.quantization.affine import AffineQuantizationFunction, StaticAffineQuantParams
from fastforward_amd.quantization.function import QuantizationContext
from fastforward_amd.quantized_tensor import QuantizedTensor

LAYOUTS = ("bhse", "bshe")
_VALUES = (torch.bfloat16, torch.float16)
Rope = tuple[torch.Tensor, torch.Tensor]


def _kernels():
    from fastforward_amd import fused_sdpa_decode  # (imports this package's modules: resolved at call time)

    return fused_sdpa_decode.KERNELS


def _quantizer_params(quantizer: Any, what: str) -> tuple[torch.Tensor, torch.Tensor | None, float]:
    """(scale, offset, bits) of a quantizer the append kernel reproduces, else ValueError: the ``_fused`` rule of the attention
    kernels (a plain, initialised, per-tensor, static ``LinearQuantizer`` with fp32 parameters) with an int8 container and 2..8 bits."""
    if not isinstance(quantizer, LinearQuantizer):
        raise ValueError(f"QuantizedKVCache: the {what} quantizer must be a LinearQuantizer, got {type(quantizer).__name__}")
    with torch.no_grad():  # (a cache serves inference: parameters that could take a gradient are no reason to decline)
        fused = _kernels()._fused(quantizer)
    if not fused or quantizer.quantized_dtype != torch.int8 or not 2 <= fused[2] <= 8:
        raise ValueError(
            f"QuantizedKVCache: the {what} quantizer must be an initialised per-tensor static LinearQuantizer with fp32 parameters, "
            "quantized_dtype=torch.int8 and an integral bit-width in 2..8"
        )
    return fused[0].detach(), None if fused[1] is None else fused[1].detach(), float(fused[2])


def _rotate(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """``x * cos + rotate_half(x) * sin`` in x's dtype, every step rounded (x [..., L, E], cos / sin [L, E])."""
    half = x.shape[-1] // 2
    rotated = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
    return x * cos + rotated * sin


def _bottom_right(L: int, S: int, device: torch.device) -> torch.Tensor:
    """bool [L, S]: row l sees key <= l + (S - L)."""
    rows = torch.arange(L, device=device).unsqueeze(1)
    return torch.arange(S, device=device).unsqueeze(0) <= rows + (S - L)


def composed_append(k_cache: torch.Tensor, v_cache: torch.Tensor, lengths: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                    key_quantizer: LinearQuantizer, value_quantizer: LinearQuantizer, rope: Rope | None = None) -> None:
    """``ops.kv_append`` from existing pieces. `lengths` already counts the L new rows; it is read on the host."""
    L, S_max = key.shape[2], k_cache.shape[2]
    with torch.no_grad():
        for b, n in enumerate(lengths.tolist()):
            rows = [l for l in range(L) if 0 <= n - L + l < S_max]
            if not rows:
                continue
            at = torch.tensor([n - L + l for l in rows], device=key.device)
            take = torch.tensor(rows, device=key.device)
            k_rows, v_rows = key[b].index_select(1, take), value[b].index_select(1, take)
            if rope is not None:
                k_rows = _rotate(k_rows, rope[0].index_select(0, at), rope[1].index_select(0, at))
            k_cache[b].index_copy_(1, at, key_quantizer(k_rows.contiguous()).raw_data)
            v_cache[b].index_copy_(1, at, value_quantizer(v_rows.contiguous()).raw_data)


def composed_attend(query: Any, k_cache: torch.Tensor, v_cache: torch.Tensor, lengths: torch.Tensor, key_quantizer: LinearQuantizer,
                    value_quantizer: LinearQuantizer, dtype: torch.dtype, is_causal: bool = True, scale: float | None = None,
                    output_quantizer: Any = None) -> torch.Tensor:
    """``ops.kv_decode`` from existing pieces: per batch, ``scaled_dot_product_attention`` over the ``[:, :, :S_b]`` slices with a
    bottom-right bool mask; exact zeros for a sequence without keys. `lengths` is read on the host."""
    from fastforward_amd.nn import functional as F

    B, H, L, E = query.shape
    HKV, S_max = k_cache.shape[1], k_cache.shape[2]
    out = torch.zeros((B, H, L, E), dtype=dtype, device=k_cache.device)
    extra = {} if output_quantizer is None else dict(output_quantizer=output_quantizer)
    with torch.no_grad():
        for b, n in enumerate(lengths.tolist()):
            S = min(max(n, 0), S_max)
            if S == 0:
                continue
            keys = key_quantizer.wrap_codes(k_cache[b:b + 1, :, :S], dtype)
            values = value_quantizer.wrap_codes(v_cache[b:b + 1, :, :S], dtype)
            mask = _bottom_right(L, S, k_cache.device) if is_causal else None
            got = F.scaled_dot_product_attention(query[b:b + 1], keys, values, attn_mask=mask, scale=scale, enable_gqa=H != HKV,
                                                 strict_quantization=False, **extra)
            out[b] = (got.dequantize() if isinstance(got, QuantizedTensor) else got)[0].to(dtype)
    return out


class _CacheBase:
    """What the two caches share: the data dtype, the head size and the two quantizers, the choice between the kernels and the composed
    chain, the checks of ``append``, and the whole of ``attend``. A subclass allocates its buffers and ``lengths`` (int32 ``[B]``),
    names its two entry points in ``_SYMBOLS`` and supplies the two calls that differ (``_native_attend``, ``_composed_attend``)."""

    _SYMBOLS: tuple[str, str]

    def _quantizer_rule(self, quantizer: Any, what: str) -> tuple:
        """What the class's append call takes for one quantizer, else ValueError: the per-tensor static rule unless a subclass has its own."""
        return _quantizer_params(quantizer, what)

    def __init__(self, dtype: torch.dtype, head_dim: int, key_quantizer: Any, value_quantizer: Any) -> None:
        name = type(self).__name__
        if dtype not in _VALUES:
            raise ValueError(f"{name}: the data dtype is bf16 or fp16, got {dtype}")
        if head_dim not in (64, 128):
            raise ValueError(f"{name}: head_dim must be 64 or 128, got {head_dim}")
        self.head_dim = head_dim
        self._quantizer_rule(key_quantizer, "key")
        self._quantizer_rule(value_quantizer, "value")
        self.key_quantizer, self.value_quantizer, self.dtype = key_quantizer, value_quantizer, dtype

    def _native(self, *tensors: torch.Tensor) -> bool:
        lib = _native.library()
        return all(t.is_cuda for t in (*tensors, self.lengths)) and all(getattr(lib, name, None) is not None for name in self._SYMBOLS)

    def _new_rows(self, key: torch.Tensor, value: torch.Tensor, store: torch.Tensor, rows: str):
        """``append``'s checks of key / value against `store` (the K cache or pool; `rows` is how the class words what it takes), then
        ``lengths += L``. Returns the two quantizers' ``(scale, offset, bits)``."""
        name = type(self).__name__
        if key.dim() != 4 or tuple(key.shape) != tuple(value.shape) or (key.shape[0], key.shape[1], key.shape[3]) != (self.lengths.shape[0], store.shape[1], store.shape[3]):
            raise ValueError(f"{name}.append: key / value are {rows}, got {tuple(key.shape)}, {tuple(value.shape)}")
        if key.dtype != self.dtype or value.dtype != self.dtype:
            raise ValueError(f"{name}.append: the new rows are plain {self.dtype} values, got {key.dtype}, {value.dtype}")
        params = self._quantizer_rule(self.key_quantizer, "key"), self._quantizer_rule(self.value_quantizer, "value")
        self.lengths.add_(key.shape[2])
        return params

    def attend(self, query: Any, is_causal: bool = True, scale: float | None = None, output_quantizer: Any = None, splits: int = 0,
               plan_len: int | None = None) -> torch.Tensor:
        """Attention of query ``[B, H_q, L, E]`` (plain, or per-tensor codes in an int8 or value-dtype container) over every sequence's
        own keys; ``H_q`` is a multiple of the cache's heads (GQA). ``is_causal`` is bottom-right. `output_quantizer`: None, a stub, or
        one the decode kernels fuse (then the result is A2 of its codes in the data dtype). ``splits`` / ``plan_len``: ``ops.kv_decode``
        (``ops.kv_paged_decode`` over pages: the same operands, refusals and bits)."""
        kernels = _kernels()
        if isinstance(query, QuantizedTensor):
            if kernels._codes_dtype(query, ("int8", "value")) != self.dtype:
                raise ValueError(f"{type(self).__name__}.attend: a quantized query holds per-tensor codes of the cache's dtype in an int8 or value-dtype container")
        elif type(query) is not torch.Tensor or query.dtype != self.dtype:
            raise ValueError(f"{type(self).__name__}.attend: the query is plain {self.dtype} or per-tensor codes of it")
        with torch.no_grad():
            fused = kernels._fused(output_quantizer)
        if fused is False:
            raise ValueError(f"{type(self).__name__}.attend: the output quantizer is not one the decode kernels fuse")
        raw, q_dequant = kernels._dequant(query)
        if not self._native(raw):
            return self._composed_attend(query, is_causal=is_causal, scale=scale, output_quantizer=output_quantizer if fused else None)
        k_params, v_params = self._quantizer_rule(self.key_quantizer, "key"), self._quantizer_rule(self.value_quantizer, "value")
        return self._native_attend(raw, is_causal, scale, fused or None, (q_dequant, k_params[:2], v_params[:2]), splits, plan_len)


class QuantizedKVCache(_CacheBase):
    """int8 K / V codes for `batch` sequences of up to `max_len` positions, quantized by two per-tensor static quantizers.

    ``layout="bhse"`` allocates ``[B, H, S_max, E]``; ``"bshe"`` allocates ``[B, S_max, H, E]`` (a position's heads side by side, the
    projection's own order) and works on its ``transpose(1, 2)`` view. ``k_cache`` / ``v_cache`` are always ``[B, H, S_max, E]`` views,
    ``lengths`` is int32 ``[B]``."""

    def __init__(self, batch: int, kv_heads: int, max_len: int, head_dim: int, key_quantizer: LinearQuantizer, value_quantizer: LinearQuantizer,
                 dtype: torch.dtype = torch.bfloat16, device: torch.device | str = "cuda", layout: str = "bhse") -> None:
        if layout not in LAYOUTS:
            raise ValueError(f"QuantizedKVCache: layout is one of {LAYOUTS}, got {layout!r}")
        if min(batch, kv_heads, max_len) < 1:
            raise ValueError(f"QuantizedKVCache: batch, kv_heads and max_len are positive, got {batch}, {kv_heads}, {max_len}")
        super().__init__(dtype, head_dim, key_quantizer, value_quantizer)
        self.layout, self.max_len = layout, max_len
        shape = (batch, kv_heads, max_len, head_dim) if layout == "bhse" else (batch, max_len, kv_heads, head_dim)
        buffers = [torch.zeros(shape, dtype=torch.int8, device=device) for _ in range(2)]
        self.k_cache, self.v_cache = (t if layout == "bhse" else t.transpose(1, 2) for t in buffers)
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)

    _SYMBOLS = ("ffq_kv_append", "ffq_kv_decode")

    def reset(self, lengths: torch.Tensor | Sequence[int] | None = None) -> None:
        """Every sequence back to length 0, or to `lengths` (the codes stay where they are: positions below a length are the cache)."""
        if lengths is None:
            self.lengths.zero_()
        else:
            self.lengths.copy_(torch.as_tensor(lengths, dtype=torch.int32).reshape(self.lengths.shape))

    def append(self, key: torch.Tensor, value: torch.Tensor, rope: Rope | None = None) -> None:
        """Quantize key / value ``[B, H, L, E]`` (plain values in the cache's dtype) to the end of every sequence: ``lengths += L``, then
        row l of batch b goes to position ``lengths[b] - L + l``; rows outside ``[0, max_len)`` are dropped. ``rope=(cos, sin)``,
        ``[P >= max_len, E]`` tables in the data dtype: K is rotated with the row of its position first."""
        k_params, v_params = self._new_rows(key, value, self.k_cache, f"[B, H, L, E] rows of a {tuple(self.k_cache.shape)} cache")
        if self._native(key, value):
            ops.kv_append(key.detach(), value.detach(), self.k_cache, self.v_cache, self.lengths, k_params, v_params, rope=rope)
        else:
            composed_append(self.k_cache, self.v_cache, self.lengths, key.detach(), value.detach(), self.key_quantizer, self.value_quantizer, rope)

    def _native_attend(self, raw, is_causal, scale, output_quantizer, dequant, splits, plan_len) -> torch.Tensor:
        return ops.kv_decode(raw, self.k_cache, self.v_cache, self.lengths, is_causal, scale, output_quantizer, dequant, self.dtype, splits, plan_len)

    def _composed_attend(self, query: Any, **how: Any) -> torch.Tensor:
        return composed_attend(query, self.k_cache, self.v_cache, self.lengths, self.key_quantizer, self.value_quantizer, self.dtype, **how)

    def keys(self, length: int) -> QuantizedTensor:
        """The first `length` positions of every sequence's keys as the QuantizedTensor the key quantizer would have returned."""
        return self.key_quantizer.wrap_codes(self.k_cache[:, :, :length], self.dtype)

    def values(self, length: int) -> QuantizedTensor:
        return self.value_quantizer.wrap_codes(self.v_cache[:, :, :length], self.dtype)


# ---- the same cache in pages ---------------------------------------------------------------------------------------------------------------
PAGED_LAYOUTS = ("phse", "pshe")


def gather_pages(pool: torch.Tensor, block_table: torch.Tensor) -> torch.Tensor:
    """The dense ``[B, H, max_pages * P, E]`` codes a block table ``[B, max_pages]`` describes in a pool ``[num_pages, H, P, E]``: a
    host-driven gather (the table is read on the host); the rows of an entry outside ``[0, num_pages)`` are zeros. A parameter pool
    ``[num_pages, H, P, 4]`` gathers the same way."""
    num_pages, H, P, E = pool.shape
    table = block_table.cpu().long()
    valid = (table >= 0) & (table < num_pages)
    pages = pool[table.clamp(0, num_pages - 1).to(pool.device)]                            # [B, max_pages, H, P, E]
    pages = torch.where(valid.to(pool.device)[:, :, None, None, None], pages, torch.zeros_like(pages))  # (a float pool may hold NaN)
    return pages.permute(0, 2, 1, 3, 4).reshape(table.shape[0], H, table.shape[1] * P, E)


def _in_use(block_table: torch.Tensor, lengths: torch.Tensor, P: int, num_pages: int) -> list[list[int]]:
    """The table entries every sequence's length reaches, read on the host; ValueError where one lies outside the pool."""
    rows = block_table.cpu().tolist()
    out = []
    for b, n in enumerate(lengths.tolist()):
        used = rows[b][:-(-min(max(n, 0), len(rows[b]) * P) // P)]
        if any(not 0 <= page < num_pages for page in used):
            raise ValueError(f"the composed paged route: sequence {b} of length {n} reaches a page that was never reserved ({used})")
        out.append(used)
    return out


def _scatter_touched(pools: Sequence[torch.Tensor], dense: Sequence[torch.Tensor], block_table: torch.Tensor, lengths: torch.Tensor, L: int) -> None:
    """The pages the L new rows of every sequence touched, copied from the gathered `dense` views back into their `pools` (a page
    outside the pool is skipped). `lengths` already counts the rows; it and the table are read on the host."""
    num_pages, P = pools[0].shape[0], pools[0].shape[2]
    rows = block_table.cpu().tolist()
    for b, n in enumerate(lengths.tolist()):
        first, last = max(n - L, 0), min(n, len(rows[b]) * P)
        for slot in range(first // P, -(-last // P) if last > first else 0):
            page = rows[b][slot]
            if 0 <= page < num_pages:
                for pool, view in zip(pools, dense):
                    pool[page].copy_(view[b, :, slot * P:(slot + 1) * P])


def composed_paged_append(k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, lengths: torch.Tensor, key: torch.Tensor,
                          value: torch.Tensor, key_quantizer: LinearQuantizer, value_quantizer: LinearQuantizer, rope: Rope | None = None) -> None:
    """``ops.kv_paged_append`` from existing pieces: the pages gathered into a dense ``[B, H, C, E]`` view, :func:`composed_append` on
    it, and the pages the new rows touched scattered back (a row whose page lies outside the pool is dropped). `lengths` already counts
    the L new rows; it and the table are read on the host."""
    k_dense, v_dense = gather_pages(k_pool, block_table), gather_pages(v_pool, block_table)
    composed_append(k_dense, v_dense, lengths, key, value, key_quantizer, value_quantizer, rope)
    _scatter_touched((k_pool, v_pool), (k_dense, v_dense), block_table, lengths, key.shape[2])


def composed_paged_attend(query: Any, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, lengths: torch.Tensor,
                          key_quantizer: LinearQuantizer, value_quantizer: LinearQuantizer, dtype: torch.dtype, is_causal: bool = True,
                          scale: float | None = None, output_quantizer: Any = None) -> torch.Tensor:
    """``ops.kv_paged_decode`` from existing pieces: :func:`composed_attend` on the gathered dense view. It reads the table on the host
    and refuses (ValueError) a sequence whose length reaches a page outside the pool, which the kernel masks."""
    _in_use(block_table, lengths, k_pool.shape[2], k_pool.shape[0])
    return composed_attend(query, gather_pages(k_pool, block_table), gather_pages(v_pool, block_table), lengths, key_quantizer, value_quantizer,
                           dtype, is_causal=is_causal, scale=scale, output_quantizer=output_quantizer)


class _PagedBase(_CacheBase):
    """What the two paged caches share: the geometry checks, the two int8 pools (``"phse"`` allocates ``[num_pages, H, P, E]``,
    ``"pshe"`` ``[num_pages, P, H, E]`` seen through ``transpose(1, 2)``), ``block_table``, ``lengths`` and the host-side page
    bookkeeping (``reserve``, ``release``, ``share_prefix``, ``pages``, ``free_pages``, reference counts), stated once. Messages carry
    the subclass's own name."""

    def __init__(self, num_pages: int, page_size: int, kv_heads: int, head_dim: int, key_quantizer: Any, value_quantizer: Any, batch: int,
                 max_pages_per_seq: int, dtype: torch.dtype, device: torch.device | str, layout: str) -> None:
        name = type(self).__name__
        if layout not in PAGED_LAYOUTS:
            raise ValueError(f"{name}: layout is one of {PAGED_LAYOUTS}, got {layout!r}")
        if not 16 <= page_size <= 256 or page_size & (page_size - 1):
            raise ValueError(f"{name}: page_size is a power of two in 16..256, got {page_size}")
        if min(num_pages, kv_heads, batch, max_pages_per_seq) < 1 or max_pages_per_seq * page_size >= 1 << 30:
            raise ValueError(f"{name}: num_pages, kv_heads, batch and max_pages_per_seq are positive and a sequence stays below 2^30 positions, "
                             f"got {num_pages}, {kv_heads}, {batch}, {max_pages_per_seq}")
        super().__init__(dtype, head_dim, key_quantizer, value_quantizer)
        self.layout, self.page_size, self.num_pages = layout, page_size, num_pages
        self.capacity = max_pages_per_seq * page_size  # positions a sequence can address
        self.k_pool, self.v_pool = (self._pool(kv_heads, head_dim, torch.int8, device) for _ in range(2))
        self.block_table = torch.full((batch, max_pages_per_seq), -1, dtype=torch.int32, device=device)
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)
        # the host's view of the table: the pages of every sequence in order, how many sequences hold each page, and the free pages
        self._pages: list[list[int]] = [[] for _ in range(batch)]
        self._refs = [0] * num_pages
        self._free = list(range(num_pages - 1, -1, -1))  # (a stack: page 0 goes out first)

    def _pool(self, kv_heads: int, width: int, dtype: torch.dtype, device: torch.device | str) -> torch.Tensor:
        """A zeroed pool ``[num_pages, H, P, width]`` view in the cache's layout."""
        shape = (self.num_pages, kv_heads, self.page_size, width) if self.layout == "phse" else (self.num_pages, self.page_size, kv_heads, width)
        t = torch.zeros(shape, dtype=dtype, device=device)
        return t if self.layout == "phse" else t.transpose(1, 2)

    # ---- host-side page bookkeeping (never inside a captured region)
    @property
    def free_pages(self) -> int:
        return len(self._free)

    def pages(self, seq: int) -> tuple[int, ...]:
        """The pool pages of sequence `seq`, in order (the host's copy of its table row)."""
        return tuple(self._pages[seq])

    def _write_row(self, seq: int) -> None:
        row = self._pages[seq] + [-1] * (self.block_table.shape[1] - len(self._pages[seq]))
        self.block_table[seq].copy_(torch.tensor(row, dtype=torch.int32))

    def reserve(self, seq: int, n_positions: int) -> None:
        """Take pages from the free list until sequence `seq` can hold `n_positions`; RuntimeError (and nothing taken) when the pool
        cannot give them, ValueError beyond the sequence's capacity."""
        name = type(self).__name__
        if not 0 <= n_positions <= self.capacity:
            raise ValueError(f"{name}.reserve: a sequence holds 0..{self.capacity} positions, got {n_positions}")
        need = -(-n_positions // self.page_size) - len(self._pages[seq])
        if need <= 0:
            return
        if need > len(self._free):
            raise RuntimeError(f"{name}.reserve: the pool is exhausted ({need} pages wanted, {len(self._free)} free)")
        for _ in range(need):
            page = self._free.pop()
            self._refs[page] = 1
            self._pages[seq].append(page)
        self._write_row(seq)

    def release(self, seq: int) -> None:
        """Give the pages of sequence `seq` back (a shared page once its last holder lets go), its table row to -1, its length to 0."""
        for page in reversed(self._pages[seq]):
            self._refs[page] -= 1
            if self._refs[page] == 0:
                self._free.append(page)
        self._pages[seq] = []
        self._write_row(seq)
        self.lengths[seq:seq + 1].zero_()

    def share_prefix(self, src: int, dst: int, n_positions: int) -> None:
        """Point the first ``n_positions // page_size`` whole pages of `dst` (which holds no page yet) at `src`'s pages, reference
        counted, and set ``lengths[dst]`` to that many positions. A partial last page is not shared: `dst` appends those rows itself."""
        name = type(self).__name__
        whole = n_positions // self.page_size
        if src == dst or self._pages[dst]:
            raise ValueError(f"{name}.share_prefix: the receiving sequence is another one and holds no page yet (release it first)")
        if not 0 <= whole <= len(self._pages[src]):
            raise ValueError(f"{name}.share_prefix: sequence {src} holds {len(self._pages[src])} pages, {whole} wanted")
        self._pages[dst] = self._pages[src][:whole]
        for page in self._pages[dst]:
            self._refs[page] += 1
        self._write_row(dst)
        self.lengths[dst:dst + 1].fill_(whole * self.page_size)


class PagedQuantizedKVCache(_PagedBase):
    """:class:`QuantizedKVCache` with the codes in fixed-size pages: two int8 pools of `num_pages` pages of `page_size` positions
    shared by `batch` sequences, each of which addresses up to `max_pages_per_seq` of them through its row of ``block_table``
    (int32 ``[batch, max_pages_per_seq]`` on the device, -1 where no page is assigned). A sequence owns only the pages it uses, a
    finished sequence's pages go back to the free list without a copy, and two sequences can share the pages of a common prefix.

    ``layout="phse"`` allocates ``[num_pages, H, P, E]``; ``"pshe"`` allocates ``[num_pages, P, H, E]`` (a position's heads side by
    side) and works on its ``transpose(1, 2)`` view. ``k_pool`` / ``v_pool`` are always ``[num_pages, H, P, E]`` views.

    ``append`` and ``attend`` are one launch each (``ops.kv_paged_append`` / ``ops.kv_paged_decode``) and read neither a length nor
    the table on the host, so a step can be captured in a graph and replayed. The page bookkeeping — ``reserve``, ``release``,
    ``share_prefix`` — is host code that writes the table with one small copy: call it OUTSIDE a captured region, ahead of the step
    that needs the page. A position whose page was never reserved is dropped by ``append`` and masked by ``attend``."""

    def __init__(self, num_pages: int, page_size: int, kv_heads: int, head_dim: int, key_quantizer: LinearQuantizer,
                 value_quantizer: LinearQuantizer, batch: int, max_pages_per_seq: int, dtype: torch.dtype = torch.bfloat16,
                 device: torch.device | str = "cuda", layout: str = "phse") -> None:
        super().__init__(num_pages, page_size, kv_heads, head_dim, key_quantizer, value_quantizer, batch, max_pages_per_seq, dtype, device, layout)

    # ---- the device side
    _SYMBOLS = ("ffq_kv_paged_append", "ffq_kv_paged_decode")

    def append(self, key: torch.Tensor, value: torch.Tensor, rope: Rope | None = None) -> None:
        """:meth:`QuantizedKVCache.append` into pages: ``lengths += L``, then row l of batch b goes to position ``lengths[b] - L + l``
        of its sequence; rows outside ``[0, capacity)`` or on a page never reserved are dropped. The rotary tables need `capacity` rows."""
        k_params, v_params = self._new_rows(key, value, self.k_pool, f"[{self.lengths.shape[0]}, {self.k_pool.shape[1]}, L, {self.k_pool.shape[3]}] rows")
        if self._native(key, value):
            ops.kv_paged_append(key.detach(), value.detach(), self.k_pool, self.v_pool, self.lengths, self.block_table, k_params, v_params, rope=rope)
        else:
            composed_paged_append(self.k_pool, self.v_pool, self.block_table, self.lengths, key.detach(), value.detach(), self.key_quantizer,
                                  self.value_quantizer, rope)

    def _native_attend(self, raw, is_causal, scale, output_quantizer, dequant, splits, plan_len) -> torch.Tensor:
        return ops.kv_paged_decode(raw, self.k_pool, self.v_pool, self.lengths, self.block_table, is_causal, scale, output_quantizer, dequant, self.dtype,
                                   splits, plan_len)

    def _composed_attend(self, query: Any, **how: Any) -> torch.Tensor:
        return composed_paged_attend(query, self.k_pool, self.v_pool, self.block_table, self.lengths, self.key_quantizer, self.value_quantizer,
                                     self.dtype, **how)

    def dense(self, seq: int | None = None) -> tuple[torch.Tensor, torch.Tensor]:
        """The K and V codes gathered into dense ``[B, H, capacity, E]`` tensors (``[H, capacity, E]`` for one sequence), zeros where no
        page is assigned: a host-driven gather for tests and debugging, not a fast path."""
        table = self.block_table if seq is None else self.block_table[seq:seq + 1]
        k, v = gather_pages(self.k_pool, table), gather_pages(self.v_pool, table)
        return (k, v) if seq is None else (k[0], v[0])


# ---- the same cache with a dynamic quantizer per row ---------------------------------------------------------------------------------------
def _dynamic_spec(quantizer: Any, what: str, head_dim: int, name: str = "DynamicQuantizedKVCache") -> tuple[float, bool]:
    """(bits, symmetric) of a dynamic quantizer the per-row append kernels reproduce, else ValueError under the class's `name`."""
    if not isinstance(quantizer, DynamicLinearQuantizer):
        raise ValueError(f"{name}: the {what} quantizer must be a DynamicLinearQuantizer, got {type(quantizer).__name__}")
    bits = quantizer.num_bits
    probe = torch.Size((2, 3, 5, head_dim))
    try:
        tile = quantizer.granularity.tile_size(probe)
    except Exception:  # (a granularity that does not take a 4-D tensor at all)
        tile = None
    if (quantizer.quantized_dtype != torch.int8 or not isinstance(bits, (int, float)) or bits != int(bits) or not 2 <= bits <= 8
            or quantizer.parameter_inference_fn is not None or isinstance(tile, str) or tile is None or tuple(tile) != (1, 1, 1, head_dim)
            or (quantizer.symmetric and quantizer.allow_one_sided)):
        raise ValueError(
            f"{name}: the {what} quantizer must be a DynamicLinearQuantizer with quantized_dtype=torch.int8, an integral bit-width in 2..8, no "
            f"parameter_inference_fn, a granularity of one tile per row ((1, 1, 1, {head_dim}) of [B, H, L, E]: PerChannel((0, 1, 2)) or PerTile), "
            "and asymmetric or symmetric with allow_one_sided=False"
        )
    return float(bits), bool(quantizer.symmetric)


def _wrap_rows(codes: torch.Tensor, scale: torch.Tensor, offset: torch.Tensor, quantizer: DynamicLinearQuantizer, dtype: torch.dtype) -> QuantizedTensor:
    """The QuantizedTensor `quantizer` returns for rows whose codes [B, H, n, E] and per-row parameters [B, H, n] are given."""
    static = StaticAffineQuantParams(scale=scale.reshape(-1).contiguous(), offset=offset.reshape(-1).contiguous(), num_bits=quantizer.num_bits,
                                     granularity=quantizer.granularity, quantized_dtype=quantizer.quantized_dtype, dequantize_dtype=dtype)
    return QuantizedTensor(codes, QuantizationContext(AffineQuantizationFunction, static))


def composed_token_append(k_cache: torch.Tensor, v_cache: torch.Tensor, params: torch.Tensor, lengths: torch.Tensor, key: torch.Tensor,
                          value: torch.Tensor, key_quantizer: DynamicLinearQuantizer, value_quantizer: DynamicLinearQuantizer,
                          rope: Rope | None = None) -> None:
    """``ops.kv_token_append`` from existing pieces: per batch the rows that land inside the cache, rotated with torch ops, quantized by
    the dynamic quantizer modules themselves, codes and per-row parameters copied to their positions. `lengths` already counts the L new
    rows; it is read on the host."""
    L, S_max = key.shape[2], k_cache.shape[2]
    with torch.no_grad():
        for b, n in enumerate(lengths.tolist()):
            rows = [l for l in range(L) if 0 <= n - L + l < S_max]
            if not rows:
                continue
            at = torch.tensor([n - L + l for l in rows], device=key.device)
            take = torch.tensor(rows, device=key.device)
            k_rows, v_rows = key[b:b + 1].index_select(2, take), value[b:b + 1].index_select(2, take)
            if rope is not None:
                k_rows = _rotate(k_rows, rope[0].index_select(0, at), rope[1].index_select(0, at))
            for first, (cache, quantizer, data) in enumerate(((k_cache, key_quantizer, k_rows), (v_cache, value_quantizer, v_rows))):
                quantized = quantizer(data.contiguous())
                args = quantized.quant_args()
                cache[b].index_copy_(1, at, quantized.raw_data[0])
                shape = (cache.shape[1], len(rows))
                offset = torch.zeros(shape, device=key.device) if args.offset is None else args.offset.float().reshape(shape)
                params[b, :, :, 2 * first].index_copy_(1, at, args.scale.float().reshape(shape))
                params[b, :, :, 2 * first + 1].index_copy_(1, at, offset)


def composed_token_attend(query: Any, k_cache: torch.Tensor, v_cache: torch.Tensor, params: torch.Tensor, lengths: torch.Tensor,
                          key_quantizer: DynamicLinearQuantizer, value_quantizer: DynamicLinearQuantizer, dtype: torch.dtype, is_causal: bool = True,
                          scale: float | None = None, output_quantizer: Any = None) -> torch.Tensor:
    """``ops.kv_token_decode`` from existing pieces: per batch, ``scaled_dot_product_attention`` over the ``[:, :, :S_b]`` slices wrapped
    with their per-row parameters, with a bottom-right bool mask; exact zeros for a sequence without keys. `lengths` is read on the host."""
    from fastforward_amd.nn import functional as F

    B, H, L, E = query.shape
    HKV, S_max = k_cache.shape[1], k_cache.shape[2]
    out = torch.zeros((B, H, L, E), dtype=dtype, device=k_cache.device)
    extra = {} if output_quantizer is None else dict(output_quantizer=output_quantizer)
    with torch.no_grad():
        for b, n in enumerate(lengths.tolist()):
            S = min(max(n, 0), S_max)
            if S == 0:
                continue
            rows = params[b:b + 1, :, :S]
            keys = _wrap_rows(k_cache[b:b + 1, :, :S], rows[..., 0], rows[..., 1], key_quantizer, dtype)
            values = _wrap_rows(v_cache[b:b + 1, :, :S], rows[..., 2], rows[..., 3], value_quantizer, dtype)
            mask = _bottom_right(L, S, k_cache.device) if is_causal else None
            got = F.scaled_dot_product_attention(query[b:b + 1], keys, values, attn_mask=mask, scale=scale, enable_gqa=H != HKV,
                                                 strict_quantization=False, **extra)
            out[b] = (got.dequantize() if isinstance(got, QuantizedTensor) else got)[0].to(dtype)
    return out


class DynamicQuantizedKVCache(_CacheBase):
    """:class:`QuantizedKVCache` with two ``DynamicLinearQuantizer``s: int8 K / V codes for `batch` sequences of up to `max_len`
    positions, every (sequence, head, position) row quantized with its own ``(scale, offset)`` from the row's min / max when it is
    appended. ``params`` is the fp32 ``[B, H, S_max, 4]`` view of ``(k_scale, k_offset, v_scale, v_offset)`` per position (``"bshe"``
    allocates ``[B, S_max, H, 4]``, like the codes). The quantizers hold ``quantized_dtype=torch.int8``, an integral bit-width in 2..8, no
    ``parameter_inference_fn``, a granularity of one tile per row (``PerChannel((0, 1, 2))`` or ``PerTile((1, 1, 1, E))``), and are
    asymmetric, or symmetric with ``allow_one_sided=False``. ``append`` and ``attend`` are one launch each and read nothing on the host."""

    _SYMBOLS = ("ffq_kv_token_append", "ffq_kv_token_decode")

    def __init__(self, batch: int, kv_heads: int, max_len: int, head_dim: int, key_quantizer: DynamicLinearQuantizer,
                 value_quantizer: DynamicLinearQuantizer, dtype: torch.dtype = torch.bfloat16, device: torch.device | str = "cuda",
                 layout: str = "bhse") -> None:
        if layout not in LAYOUTS:
            raise ValueError(f"DynamicQuantizedKVCache: layout is one of {LAYOUTS}, got {layout!r}")
        if min(batch, kv_heads, max_len) < 1:
            raise ValueError(f"DynamicQuantizedKVCache: batch, kv_heads and max_len are positive, got {batch}, {kv_heads}, {max_len}")
        super().__init__(dtype, head_dim, key_quantizer, value_quantizer)
        self.layout, self.max_len = layout, max_len
        lead = (batch, kv_heads, max_len) if layout == "bhse" else (batch, max_len, kv_heads)
        buffers = [torch.zeros((*lead, head_dim), dtype=torch.int8, device=device) for _ in range(2)]
        buffers.append(torch.zeros((*lead, 4), dtype=torch.float32, device=device))
        self.k_cache, self.v_cache, self.params = (t if layout == "bhse" else t.transpose(1, 2) for t in buffers)
        self.lengths = torch.zeros(batch, dtype=torch.int32, device=device)

    def _quantizer_rule(self, quantizer: Any, what: str) -> tuple[float, bool]:
        return _dynamic_spec(quantizer, what, self.head_dim)

    def reset(self, lengths: torch.Tensor | Sequence[int] | None = None) -> None:
        """Every sequence back to length 0, or to `lengths` (codes and parameters stay where they are)."""
        QuantizedKVCache.reset(self, lengths)  # type: ignore[arg-type]

    def append(self, key: torch.Tensor, value: torch.Tensor, rope: Rope | None = None) -> None:
        """:meth:`QuantizedKVCache.append` with every row's own parameters: ``lengths += L``, then row l of batch b goes to position
        ``lengths[b] - L + l`` with the codes and the ``(scale, offset)`` its dynamic quantizer gives that row (K rotated first with
        ``rope``); rows outside ``[0, max_len)`` are dropped and their parameters stay as they were."""
        k_spec, v_spec = self._new_rows(key, value, self.k_cache, f"[B, H, L, E] rows of a {tuple(self.k_cache.shape)} cache")
        if self._native(key, value):
            ops.kv_token_append(key.detach(), value.detach(), self.k_cache, self.v_cache, self.params, self.lengths, k_spec, v_spec, rope=rope)
        else:
            composed_token_append(self.k_cache, self.v_cache, self.params, self.lengths, key.detach(), value.detach(), self.key_quantizer,
                                  self.value_quantizer, rope)

    def _native_attend(self, raw, is_causal, scale, output_quantizer, dequant, splits, plan_len) -> torch.Tensor:
        return ops.kv_token_decode(raw, self.k_cache, self.v_cache, self.params, self.lengths, is_causal, scale, output_quantizer, dequant[0], self.dtype,
                                   splits, plan_len)

    def _composed_attend(self, query: Any, **how: Any) -> torch.Tensor:
        return composed_token_attend(query, self.k_cache, self.v_cache, self.params, self.lengths, self.key_quantizer, self.value_quantizer,
                                     self.dtype, **how)

    def keys(self, length: int) -> QuantizedTensor:
        """The first `length` positions of every sequence's keys as the QuantizedTensor the key quantizer would have returned for those
        rows: the codes with one (scale, offset) per row."""
        rows = self.params[:, :, :length]
        return _wrap_rows(self.k_cache[:, :, :length], rows[..., 0], rows[..., 1], self.key_quantizer, self.dtype)

    def values(self, length: int) -> QuantizedTensor:
        rows = self.params[:, :, :length]
        return _wrap_rows(self.v_cache[:, :, :length], rows[..., 2], rows[..., 3], self.value_quantizer, self.dtype)


# ---- both: pages and a dynamic quantizer per row -------------------------------------------------------------------------------------------
def composed_paged_token_append(k_pool: torch.Tensor, v_pool: torch.Tensor, param_pool: torch.Tensor, block_table: torch.Tensor, lengths: torch.Tensor,
                                key: torch.Tensor, value: torch.Tensor, key_quantizer: DynamicLinearQuantizer, value_quantizer: DynamicLinearQuantizer,
                                rope: Rope | None = None) -> None:
    """``ops.kv_paged_token_append`` from existing pieces: the three pools gathered into dense views, :func:`composed_token_append` on
    them, and the pages the new rows touched scattered back (a row whose page lies outside the pool is dropped, its parameters too).
    `lengths` already counts the L new rows; it and the table are read on the host."""
    dense = [gather_pages(pool, block_table) for pool in (k_pool, v_pool, param_pool)]
    composed_token_append(*dense, lengths, key, value, key_quantizer, value_quantizer, rope)
    _scatter_touched((k_pool, v_pool, param_pool), dense, block_table, lengths, key.shape[2])


def composed_paged_token_attend(query: Any, k_pool: torch.Tensor, v_pool: torch.Tensor, param_pool: torch.Tensor, block_table: torch.Tensor,
                                lengths: torch.Tensor, key_quantizer: DynamicLinearQuantizer, value_quantizer: DynamicLinearQuantizer,
                                dtype: torch.dtype, is_causal: bool = True, scale: float | None = None, output_quantizer: Any = None) -> torch.Tensor:
    """``ops.kv_paged_token_decode`` from existing pieces: :func:`composed_token_attend` on the gathered dense views. It reads the table
    on the host and refuses (ValueError) a sequence whose length reaches a page outside the pool, which the kernel masks."""
    _in_use(block_table, lengths, k_pool.shape[2], k_pool.shape[0])
    return composed_token_attend(query, *(gather_pages(pool, block_table) for pool in (k_pool, v_pool, param_pool)), lengths, key_quantizer,
                                 value_quantizer, dtype, is_causal=is_causal, scale=scale, output_quantizer=output_quantizer)


class PagedDynamicQuantizedKVCache(_PagedBase):
    """:class:`PagedQuantizedKVCache` with the two ``DynamicLinearQuantizer``s of :class:`DynamicQuantizedKVCache`: int8 K / V codes in
    pages behind ``block_table``, every (sequence, head, position) row quantized with its own ``(scale, offset)`` when it is appended.
    ``param_pool`` is the fp32 ``[num_pages, H, P, 4]`` view of ``(k_scale, k_offset, v_scale, v_offset)`` per row of every page
    (``"pshe"`` allocates ``[num_pages, P, H, 4]``, like the codes): a page shared by two sequences shares its parameters. The quantizer
    rule is :class:`DynamicQuantizedKVCache`'s, the pages and the bookkeeping (``reserve``, ``release``, ``share_prefix``, outside a
    captured region) are :class:`PagedQuantizedKVCache`'s. ``append`` and ``attend`` are one launch each
    (``ops.kv_paged_token_append`` / ``ops.kv_paged_token_decode``) and read nothing on the host."""

    _SYMBOLS = ("ffq_kv_paged_token_append", "ffq_kv_paged_token_decode")

    def __init__(self, num_pages: int, page_size: int, kv_heads: int, head_dim: int, key_quantizer: DynamicLinearQuantizer,
                 value_quantizer: DynamicLinearQuantizer, batch: int, max_pages_per_seq: int, dtype: torch.dtype = torch.bfloat16,
                 device: torch.device | str = "cuda", layout: str = "phse") -> None:
        super().__init__(num_pages, page_size, kv_heads, head_dim, key_quantizer, value_quantizer, batch, max_pages_per_seq, dtype, device, layout)
        self.param_pool = self._pool(kv_heads, 4, torch.float32, device)

    def _quantizer_rule(self, quantizer: Any, what: str) -> tuple[float, bool]:
        return _dynamic_spec(quantizer, what, self.head_dim, type(self).__name__)

    def append(self, key: torch.Tensor, value: torch.Tensor, rope: Rope | None = None) -> None:
        """:meth:`DynamicQuantizedKVCache.append` into pages: ``lengths += L``, then row l of batch b goes to position
        ``lengths[b] - L + l`` of its sequence with its own codes and ``(scale, offset)``; rows outside ``[0, capacity)`` or on a page
        never reserved are dropped, their parameters included. The rotary tables need `capacity` rows."""
        k_spec, v_spec = self._new_rows(key, value, self.k_pool, f"[{self.lengths.shape[0]}, {self.k_pool.shape[1]}, L, {self.k_pool.shape[3]}] rows")
        if self._native(key, value):
            ops.kv_paged_token_append(key.detach(), value.detach(), self.k_pool, self.v_pool, self.param_pool, self.lengths, self.block_table, k_spec,
                                      v_spec, rope=rope)
        else:
            composed_paged_token_append(self.k_pool, self.v_pool, self.param_pool, self.block_table, self.lengths, key.detach(), value.detach(),
                                        self.key_quantizer, self.value_quantizer, rope)

    def _native_attend(self, raw, is_causal, scale, output_quantizer, dequant, splits, plan_len) -> torch.Tensor:
        return ops.kv_paged_token_decode(raw, self.k_pool, self.v_pool, self.param_pool, self.lengths, self.block_table, is_causal, scale,
                                         output_quantizer, dequant[0], self.dtype, splits, plan_len)

    def _composed_attend(self, query: Any, **how: Any) -> torch.Tensor:
        return composed_paged_token_attend(query, self.k_pool, self.v_pool, self.param_pool, self.block_table, self.lengths, self.key_quantizer,
                                           self.value_quantizer, self.dtype, **how)

    def dense(self, seq: int | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """The K and V codes and the parameters gathered into dense ``[B, H, capacity, E | 4]`` tensors (``[H, capacity, E | 4]`` for one
        sequence), zeros where no page is assigned: a host-driven gather for tests and debugging, not a fast path."""
        table = self.block_table if seq is None else self.block_table[seq:seq + 1]
        k, v, params = (gather_pages(pool, table) for pool in (self.k_pool, self.v_pool, self.param_pool))
        return (k, v, params) if seq is None else (k[0], v[0], params[0])
