"""Guard bands around every buffer a C-ABI call touches: the memory contract of ``include/ffq.h`` as assertions.

``check_call(fn, inputs)`` runs ``fn(*inputs)`` three times: as it is, and twice with every tensor the call touches carved from an
:class:`Arena` (inputs copied in; the package's own outputs, workspaces, ticket and extrema words captured by :func:`capture`)
whose guards and fresh bodies hold poison A (0xFF: NaN as a float, -1 as an integer), then poison B (0x7F: a huge finite float,
+127 as a code). :func:`verdict` then checks

  I1  every guard byte of every arena buffer is unchanged (a store before or past any operand);
  I2  every input body is bit-identical to before (declared in-place operands: equal to the unguarded run's final state);
  I3  the A and B results equal each other and the unguarded result (an element no lane wrote, a result that depends on
      workspace contents or on bytes outside an operand, differs between A and B);
  I4  ticket words are zero and extrema words {0xFFFFFFFF, 0, 0, 0} after the call;
  I5  the workspace handed to the library is exactly as long as the size the library was told, and that size is what a
      ``*_workspace_bytes`` / ``*_slab_bytes`` query returned (I1 on its trailing guard then covers the query).

Honesty: a :class:`Recorder` stands between the package and the library (installed with ``conftest.use_backend``; its ``path``
differs from the shipped library's, so calls take the ctypes route, where Python allocates) and notes every pointer argument,
those inside ``ffq_fanout`` / ``ffq_cat_inputs`` / ``ffq_rows_batch`` / quantizer-slot arrays included. A pointer other than the
stream that is not inside an arena body, or a returned tensor whose storage is not an arena buffer, FAILS the case.

What this cannot see: an out-of-bounds READ whose value is discarded."""

from __future__ import annotations

import contextlib
import ctypes

from dataclasses import dataclass, field

import torch

from conftest import use_backend
from fastforward_amd import _cabi, _native
from fastforward_amd.ops import _base
from helpers import same_with_nan

GUARD = 512  # bytes before a body, and at least as many after it
ALIGN = 512  # what the device's caching allocator gives every block: the kernels branch on alignment
POISON_A, POISON_B = 0xFF, 0x7F
EXTREMA_IDLE = (-1, 0, 0, 0)  # {0xFFFFFFFF, 0, 0, 0} as int32

# the real functions, bound before any patch
_empty, _zeros, _full, _empty_like, _zeros_like = torch.empty, torch.zeros, torch.full, torch.empty_like, torch.zeros_like
_new_empty, _contiguous, _clone, _to = torch.Tensor.new_empty, torch.Tensor.contiguous, torch.Tensor.clone, torch.Tensor.to


@dataclass
class Block:
    chunk: torch.Tensor  # the flat uint8 buffer this block is carved from
    start: int  # body offset inside the chunk
    nbytes: int
    end: int  # end of the trailing guard (the next block's leading guard starts here)
    kind: str  # "input" | "fresh" | "copy"
    label: str

    @property
    def pointer(self) -> int:
        return self.chunk.data_ptr() + self.start

    def body(self) -> torch.Tensor:
        return self.chunk[self.start:self.start + self.nbytes]

    def guards(self) -> tuple[torch.Tensor, torch.Tensor]:
        return self.chunk[self.start - GUARD:self.start], self.chunk[self.start + self.nbytes:self.end]


class Arena:
    """Flat uint8 buffers, poison-filled, from which bodies are carved: ``[guard >= 512][body][guard >= 512] ...``. A body starts on a
    512-byte boundary (plus `misalign`, for an input that was a view at an offset); its trailing guard starts at the first byte after
    it. Bodies are never reused."""

    def __init__(self, poison: int, chunk_bytes: int = 1 << 22) -> None:
        self.poison, self.chunk_bytes = poison, chunk_bytes
        self.blocks: list[Block] = []
        self._open: dict[torch.device, tuple[torch.Tensor, int]] = {}  # device -> (chunk, first free offset)
        self.chunks: list[torch.Tensor] = []

    def carve(self, nbytes: int, device: torch.device, kind: str, label: str = "", misalign: int = 0) -> Block:
        device = torch.device(device)
        need = GUARD + ALIGN + misalign + nbytes + GUARD + ALIGN
        have = self._open.get(device)
        if have is None or have[1] + need > have[0].numel():
            chunk = _full((max(self.chunk_bytes, need) + ALIGN,), self.poison, dtype=torch.uint8, device=device)
            self.chunks.append(chunk)
            have = (chunk, 0)
        chunk, free = have
        base = chunk.data_ptr()
        start = free + GUARD
        start += (-(base + start)) % ALIGN + misalign
        end = start + nbytes + GUARD
        end += (-(base + end)) % ALIGN  # (the pad belongs to the trailing guard: nothing sits between body and guard)
        assert end <= chunk.numel() and (base + start - misalign) % ALIGN == 0
        self._open[device] = (chunk, end)
        block = Block(chunk, start, nbytes, end, kind, label)
        self.blocks.append(block)
        return block

    def like(self, t: torch.Tensor, kind: str, label: str = "") -> torch.Tensor:
        """A tensor of `t`'s shape, strides and dtype on `t`'s device whose storage is a fresh body (holding poison)."""
        span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) if t.numel() else 0
        block = self.carve(span * t.element_size(), t.device, kind, label or f"{kind} {tuple(t.shape)} {t.dtype}")
        return block.body().view(t.dtype).as_strided(t.shape, t.stride())

    def adopt(self, t: torch.Tensor, label: str = "") -> torch.Tensor:
        """A copy of input `t` inside the arena: the same shape, strides and values (the bytes between the elements of a strided view
        too), at `t`'s own remainder mod 512 on the device."""
        span = 1 + sum((n - 1) * st for n, st in zip(t.shape, t.stride())) if t.numel() else 0
        misalign = t.data_ptr() % ALIGN if t.is_cuda else t.data_ptr() % 16
        block = self.carve(span * t.element_size(), t.device, "input", label or f"input {tuple(t.shape)} {t.dtype}", misalign)
        flat = block.body().view(t.dtype)
        if span:
            flat.copy_(t.detach().as_strided((span,), (1,)))
        return flat.as_strided(t.shape, t.stride())

    def find(self, pointer: int) -> Block | None:
        for b in self.blocks:
            if b.pointer <= pointer < b.pointer + max(b.nbytes, 1):
                return b
        return None

    def owns(self, t: torch.Tensor) -> bool:
        return t.numel() == 0 or self.find(t.data_ptr()) is not None

    def touched_guards(self) -> list[str]:
        """I1: the blocks one of whose guard bytes no longer holds the poison (one device round trip per chunk unless something is wrong)."""
        bad = []
        for chunk in self.chunks:
            wrong = chunk != self.poison
            for b in self.blocks:
                if b.chunk is chunk:
                    wrong[b.start:b.start + b.nbytes] = False
            if not bool(wrong.any()):
                continue
            for b in self.blocks:
                if b.chunk is not chunk:
                    continue
                for side, g in zip(("before", "after"), b.guards()):
                    hit = (g != self.poison).nonzero().flatten()
                    if hit.numel():
                        at = int(hit[0]) - GUARD if side == "before" else int(hit[0])
                        bad.append(f"{b.label}: guard byte {at:+d} {side} the body was written ({hit.numel()} bytes changed)")
        return bad


# ---- scoped allocator capture ---------------------------------------------------------------------------------------------------
_PATCHED = False


@contextlib.contextmanager
def capture(arena: Arena):
    """Inside the block the package's own allocations come from `arena`: ``torch.empty / empty_like / zeros / zeros_like / full``
    and ``Tensor.new_empty`` (fresh bodies keep the poison; zeros and full keep their fill), and the copies ``.contiguous()``,
    ``.clone()`` (``_dense``) and ``.to()`` make. ``_base._TICKETS`` / ``_EXTREMA_WORDS`` start empty, so the cached
    words are re-made inside the arena; both are put back on exit. Test code only: nothing in the package knows."""
    global _PATCHED
    assert not _PATCHED, "capture() does not nest"

    def fresh(real):
        def make(*args, **kwargs):
            t = real(*args, **kwargs)
            return arena.like(t, "fresh") if isinstance(t, torch.Tensor) and t.numel() else t
        return make

    def copied(real):
        def make(*args, **kwargs):
            t = real(*args, **kwargs)
            if not isinstance(t, torch.Tensor) or arena.owns(t):
                return t
            home = arena.like(t, "copy")
            home.copy_(t)
            return home
        return make

    module = {"empty": fresh(_empty), "empty_like": fresh(_empty_like), "zeros": copied(_zeros), "zeros_like": copied(_zeros_like), "full": copied(_full)}
    # Beyond the allocation functions, the three tensor methods with which the package makes a COPY that it then hands to the library:
    #   contiguous  every ops module (``data.detach().contiguous()``, ``_base._flat``): a strided operand
    #   clone       ``_base._dense``: a misaligned or strided operand of the entry points that take 16-byte aligned buffers only
    #   to          ``.to(torch.float32)`` of half-precision parameters (gemm, wq, conv, modules, packing, producers, sdpa) and
    #               ``.to(torch.int8)`` of the GGUF writers' codes
    # Each returns its operand itself when there is nothing to copy, and that one already lives in the arena. Drop one of them and
    # the honesty condition fails the cases whose operands need that copy.
    method = {"new_empty": fresh(_new_empty), "contiguous": copied(_contiguous), "clone": copied(_clone), "to": copied(_to)}
    real_module = {k: getattr(torch, k) for k in module}
    real_method = {k: getattr(torch.Tensor, k) for k in method}
    tickets, words = dict(_base._TICKETS), dict(_base._EXTREMA_WORDS)
    _base._TICKETS.clear()
    _base._EXTREMA_WORDS.clear()
    for k, v in module.items():
        setattr(torch, k, v)
    for k, v in method.items():
        setattr(torch.Tensor, k, v)
    _PATCHED = True
    scratch = {"tickets": _base._TICKETS, "extrema": _base._EXTREMA_WORDS}
    try:
        yield scratch
    finally:
        _PATCHED = False
        for k, v in real_module.items():
            setattr(torch, k, v)
        for k, v in real_method.items():
            setattr(torch.Tensor, k, v)
        scratch["tickets"], scratch["extrema"] = dict(_base._TICKETS), dict(_base._EXTREMA_WORDS)
        _base._TICKETS.clear()
        _base._TICKETS.update(tickets)
        _base._EXTREMA_WORDS.clear()
        _base._EXTREMA_WORDS.update(words)


# ---- recording proxy library ----------------------------------------------------------------------------------------------------
@dataclass
class Call:
    name: str
    pointers: list[int]  # every non-null pointer argument but the stream, struct members included
    workspaces: list[tuple[int | None, int]]  # (pointer, size_t) pairs: a void* directly followed by a size_t
    result: int


def _pointers_in(obj) -> list[int]:
    """Every non-null ``void*`` held by a ctypes argument: an address, a byref / pointer to a struct, a struct, an array."""
    if obj is None:
        return []
    if isinstance(obj, int):
        return [obj] if obj else []
    if isinstance(obj, ctypes.c_void_p):
        return [obj.value] if obj.value else []
    if hasattr(obj, "_obj"):  # ctypes.byref(x)
        return _pointers_in(obj._obj)
    if isinstance(obj, ctypes._Pointer):
        return _pointers_in(obj.contents) if obj else []
    if isinstance(obj, ctypes.Array):
        if issubclass(obj._type_, (ctypes.c_void_p, ctypes.Structure, ctypes.Array)):
            return [p for item in obj for p in _pointers_in(item)]
        return []
    if isinstance(obj, ctypes.Structure):
        out = []
        for name, ftype in obj._fields_:
            if ftype is ctypes.c_void_p or (isinstance(ftype, type) and issubclass(ftype, (ctypes.Array, ctypes.Structure))):
                out += _pointers_in(getattr(obj, name))
        return out
    return []


class Recorder:
    """An ``FFQLibrary`` look-alike that forwards every ``ffq_*`` call to `real` and records the pointers it was given."""

    def __init__(self, real) -> None:
        self._real = real
        self.path = f"{real.path}#guarded"  # != _native.LIBRARY_PATH: ops._base._native_route() is False, Python allocates
        assert self.path != str(_native.LIBRARY_PATH)
        self.backend_name = real.backend_name
        self.calls: list[Call] = []
        self.queries: list[tuple[str, int]] = []  # results of the *_workspace_bytes / *_slab_bytes queries

    @property
    def is_device(self) -> bool:
        return self._real.is_device

    def check(self, status: int) -> None:
        self._real.check(status)

    def __getattr__(self, name: str):
        attr = getattr(self._real, name)
        if not name.startswith("ffq_") or attr is None:
            return attr
        argtypes = _cabi.SIGNATURES[name][1]

        def call(*args):
            result = attr(*args)
            if name.endswith("_bytes"):
                self.queries.append((name, int(result)))
            if name in LAUNCHING:
                assert len(args) == len(argtypes), (name, len(args), len(argtypes))
                pointers: list[int] = []
                workspaces = []
                for i, (tp, a) in enumerate(zip(argtypes[:-1], args[:-1])):  # (the last argument is the stream)
                    if tp in (ctypes.c_int, ctypes.c_int64, ctypes.c_double, ctypes.c_size_t):
                        continue
                    pointers += _pointers_in(a)
                    if tp is ctypes.c_void_p and argtypes[i + 1] is ctypes.c_size_t:
                        workspaces.append((a, int(args[i + 1])))
                self.calls.append(Call(name, pointers, workspaces, int(result)))
            return result

        return call


# the entry points that enqueue work: their last argument is the stream (include/ffq.h)
LAUNCHING = frozenset(name for name, (_, argtypes) in _cabi.SIGNATURES.items() if argtypes and argtypes[-1] is ctypes.c_void_p)


# ---- one guarded run --------------------------------------------------------------------------------------------------------------
def tree_map(f, obj):
    if isinstance(obj, torch.Tensor):
        return f(obj)
    if isinstance(obj, (list, tuple)):
        return type(obj)(tree_map(f, o) for o in obj)
    if isinstance(obj, dict):
        return {k: tree_map(f, v) for k, v in obj.items()}
    return obj


def tensors_of(obj) -> list[torch.Tensor]:
    out: list[torch.Tensor] = []
    tree_map(out.append, obj)
    return out


def _sync(obj) -> None:
    if any(t.is_cuda for t in tensors_of(obj)):
        torch.cuda.synchronize()


@dataclass
class Run:
    """What one guarded run left behind; :func:`verdict` reads nothing else."""

    arena: Arena
    recorder: Recorder
    inputs: list[torch.Tensor]  # the adopted inputs (arena views), flattened
    inplace: list[bool]  # per input: a declared in-place operand
    before: list[torch.Tensor]  # the bytes of each input's body before the call
    result: object = None  # the call's result, still in the arena
    tickets: list[torch.Tensor] = field(default_factory=list)
    extrema: list[torch.Tensor] = field(default_factory=list)


def guarded_run(fn, inputs, inplace, library, poison: int) -> Run:
    arena = Arena(poison)
    marks: list[bool] = []
    for i, top in enumerate(inputs):
        marks += [i in inplace] * len(tensors_of(top))
    adopted = tree_map(arena.adopt, list(inputs))
    flat = tensors_of(adopted)
    before = [_clone(arena.find(t.data_ptr()).body()) if t.numel() else _empty(0, dtype=torch.uint8) for t in flat]
    recorder = Recorder(library)
    run = Run(arena, recorder, flat, marks, before)
    with use_backend(recorder), capture(arena) as scratch:
        run.result = fn(*adopted)
    _sync((flat, run.result))
    run.tickets, run.extrema = list(scratch["tickets"].values()), list(scratch["extrema"].values())
    return run


def plain_run(fn, inputs, library):
    """The unguarded run (on clones, so in-place operands start from the same values): (result, final state of the inputs)."""
    mine = tree_map(lambda t: _clone(t.detach()), list(inputs))
    with use_backend(Recorder(library)):  # (the same route as the guarded runs: ctypes; the allocator is torch's own)
        result = fn(*mine)
    _sync((mine, result))
    return result, tensors_of(mine)


def _same(a, b) -> bool:
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor):
        return a.shape == b.shape and a.dtype == b.dtype and same_with_nan(a, b)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    return not isinstance(a, torch.Tensor) and not isinstance(b, torch.Tensor) and a == b


def _differences(a, b, path="result") -> list[str]:
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)) and len(a) == len(b):
        return [d for i, (x, y) in enumerate(zip(a, b)) for d in _differences(x, y, f"{path}[{i}]")]
    if _same(a, b):
        return []
    if isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.shape == b.shape:
        x, y = a.double().flatten(), b.double().flatten()
        bad = ~((x == y) & (torch.signbit(x) == torch.signbit(y)) | (x.isnan() & y.isnan()))
        first = int(bad.nonzero()[0]) if bool(bad.any()) else -1
        return [f"{path}: {int(bad.sum())} of {x.numel()} elements differ, first at flat index {first}: {x[first].item()} vs {y[first].item()}"]
    return [f"{path}: {type(a).__name__} vs {type(b).__name__}"]


def verdict(run: Run, plain=None, other: Run | None = None, workspace_queries: bool = True, workspace_image: int = 0) -> list[str]:
    """The broken invariants of one guarded run, each line starting with the invariant's name; [] when the contract held. `plain`:
    :func:`plain_run`'s pair; `other`: the run under the other poison; `workspace_image`: bytes the caller adds to a queried size by the
    header's rule (the bf16 image of a forced two-pass weight-only GEMM)."""
    arena, out = run.arena, []
    # honesty: nothing the library was handed, and nothing the call returned, lives outside the arena
    for call in run.recorder.calls:
        for p in call.pointers:
            if arena.find(p) is None:
                out.append(f"HONESTY {call.name}: pointer {p:#x} is not inside an arena body (an allocation slipped past the harness)")
    for t in tensors_of(run.result):
        if not arena.owns(t):
            out.append(f"HONESTY: a returned tensor {tuple(t.shape)} {t.dtype} does not live in the arena")
    for t in run.tickets + run.extrema:
        if not arena.owns(t):
            out.append("HONESTY: ticket / extrema words were made outside the arena")
    if not run.recorder.calls:
        out.append("HONESTY: the call reached no launching entry point")
    # I1
    out += [f"I1 {line}" for line in arena.touched_guards()]
    # I2
    for i, (t, mark, was) in enumerate(zip(run.inputs, run.inplace, run.before)):
        if not t.numel():
            continue
        if mark:
            if plain is not None and not _same(t, plain[1][i]):
                out.append(f"I2 in-place input {i}: its final state differs from the unguarded run's: " + "; ".join(_differences(t, plain[1][i], "input")))
            continue
        now = arena.find(t.data_ptr()).body()
        if not torch.equal(now, was):
            at = int((now != was).nonzero()[0])
            out.append(f"I2 input {i} ({tuple(t.shape)} {t.dtype}) was written: byte {at} of its body changed")
    # I3
    if plain is not None:
        out += [f"I3 guarded (poison {arena.poison:#x}) vs unguarded: {d}" for d in _differences(run.result, plain[0])]
    if other is not None:
        out += [f"I3 poison {arena.poison:#x} vs poison {other.arena.poison:#x}: {d}" for d in _differences(run.result, other.result)]
        for i, (t, u, mark) in enumerate(zip(run.inputs, other.inputs, run.inplace)):
            if mark and not _same(t, u):
                out.append(f"I3 in-place input {i} differs between the poisons: " + "; ".join(_differences(t, u, "input")))
    # I4
    for t in run.tickets:
        if bool((t != 0).any()):
            out.append(f"I4 a ticket word was left at {int(t[(t != 0).nonzero()[0]].flatten()[0])} (index {int((t != 0).nonzero()[0])})")
    for t in run.extrema:
        if tuple(int(v) for v in t.cpu()) != EXTREMA_IDLE:
            out.append(f"I4 extrema words were left at {[hex(int(v) & 0xFFFFFFFF) for v in t.cpu()]}")
    # I5
    sizes = {n for _, n in run.recorder.queries}
    # (the weight-only GEMMs: slabs of the plan in force + the library's figure - the slabs of its own plan, ops/wq.py _wq_scratch)
    composed = {a + b - c for a in sizes for b in sizes for c in sizes}
    for call in run.recorder.calls:
        for pointer, nbytes in call.workspaces:
            if not pointer:
                continue
            block = arena.find(pointer)
            if block is None:
                continue  # (reported above)
            if block.pointer != pointer or block.nbytes != nbytes:
                out.append(f"I5 {call.name}: told {nbytes} workspace bytes, handed a buffer of {block.nbytes} (at +{pointer - block.pointer})")
            if workspace_queries and nbytes not in sizes and nbytes - workspace_image not in sizes and nbytes not in composed:
                out.append(f"I5 {call.name}: {nbytes} workspace bytes is not what the size queries returned ({sorted(sizes)})")
    return out


def check_call(fn, inputs, inplace=(), symbols=(), library=None, workspace_queries: bool = True, workspace_image: int = 0):
    """Run ``fn(*inputs)`` unguarded and under both poisons; assert I1-I5 and the honesty condition. `inputs`: tensors, or lists /
    tuples of tensors and None; `inplace`: positions in `inputs` the call writes by contract; `symbols`: entry points the call must
    have reached (what the case claims to cover). Returns (unguarded result, run A, run B)."""
    library = library if library is not None else _native.library()
    plain = plain_run(fn, inputs, library)
    run_a = guarded_run(fn, inputs, set(inplace), library, POISON_A)
    run_b = guarded_run(fn, inputs, set(inplace), library, POISON_B)
    problems = verdict(run_a, plain, run_b, workspace_queries, workspace_image) + verdict(run_b, plain, None, workspace_queries, workspace_image)
    reached = {c.name for c in run_a.recorder.calls}
    problems += [f"COVERAGE the call never reached {name}" for name in symbols if name not in reached]
    assert not problems, "\n".join(problems)
    return plain[0], run_a, run_b


# the rest of _cabi.SIGNATURES: entry points that enqueue nothing (tests/test_guards_cpu.py checks the partition)
EXEMPT: dict[str, str] = {
    "ffq_abi_version": "host query: returns a constant",
    "ffq_last_error": "host query: the thread's last error string",
    "ffq_backend_name": "host query: returns a constant string",
    "ffq_num_tiles": "host arithmetic on a tiling struct",
    "ffq_can_support_bitwidth": "host arithmetic on two numbers",
    "ffq_promote_types": "host table lookup",
    "ffq_dequantize_result_dtype": "host table lookup",
    "ffq_minmax_workspace_bytes": "host size query",
    "ffq_parameters_for_range_workspace_bytes": "host size query",
    "ffq_quantize_dynamic_workspace_bytes": "host size query",
    "ffq_linear_w8a8_workspace_bytes": "host size query",
    "ffq_bmm_w8a8_workspace_bytes": "host size query",
    "ffq_linear_w8a8_takes_earlier": "host shape predicate",
    "ffq_grid_sqerror_workspace_bytes": "host size query",
    "ffq_quantize_backward_workspace_bytes": "host size query",
    "ffq_mlp_gate_up_wq_workspace_bytes": "host size query",
    "ffq_mlp_gate_up_w8a8_workspace_bytes": "host size query",
    "ffq_mlp_gate_up_w8a8_estimating_workspace_bytes": "host size query",
    "ffq_sum_quantize_workspace_bytes": "host size query",
    "ffq_conv2d_w8a8_workspace_bytes": "host size query",
    "ffq_conv_transpose2d_w8a8_workspace_bytes": "host size query",
    "ffq_linear_wq_supported": "host shape predicate",
    "ffq_linear_wq_workspace_bytes": "host size query",
    "ffq_linear_wq_split": "host plan query",
    "ffq_linear_wq_tickets": "host plan query",
    "ffq_linear_wq_slab_bytes": "host size query",
    "ffq_force_generic_kernels": "test hook: sets a host flag, launches nothing",
}
