"""The guard-band harness (tests/guards.py) tested on host memory with the C oracle: it passes a correct library on every entry
point the oracle exports, it reports each planted defect under the right invariant, and the cases of tests/test_guards_gpu.py
cover every launching symbol of ``_cabi.SIGNATURES``. The defects live in a test-local wrapper around the oracle and touch only
host memory inside the test's own arena: nothing faults."""

from __future__ import annotations

import ctypes

import pytest
import torch

from fastforward_amd import _cabi, ops
from fastforward_amd.ops import _base

import guards

from test_guards_gpu import CASES, GUARDED, I8, BF16, one, real

HOST_CASES = [c for c in CASES if c.host]


@pytest.mark.parametrize("case", HOST_CASES, ids=[c.id for c in HOST_CASES])
def test_the_harness_passes_the_oracle(case, oracle_lib):
    assert all(getattr(oracle_lib, s) is not None for s in case.symbols)
    fn, inputs, inplace = case.build("cpu")
    guards.check_call(fn, inputs, inplace, case.symbols, library=oracle_lib, workspace_image=case.workspace_image)


def test_every_entry_point_the_oracle_exports_has_a_host_case(oracle_lib):
    exported = {name for name in guards.LAUNCHING if getattr(oracle_lib, name) is not None}
    # the persistent int8 GEMM's shape class starts at 64 tiles of 256 x 256: seconds per run in the oracle's double loops
    device_shapes = {"ffq_linear_w8a8_multi", "ffq_linear_w8a8_earlier", "ffq_linear_w8a8_gated", "ffq_mlp_gate_up_w8a8_estimating"}
    assert exported - device_shapes == {s for c in HOST_CASES for s in c.symbols}


# ---- planted defects --------------------------------------------------------------------------------------------------------------
def _byte(address: int):
    return ctypes.c_ubyte.from_address(address)


class Defective:
    """The oracle with one defect: `after(args)` runs after every ``ffq_quantize_by_tile`` call (data = args[0], out = args[10]);
    `workspace` makes the min/max size query ask for that many bytes. The defects act in the guarded runs only, where every buffer lies in the test's arena."""

    def __init__(self, real_lib, after=None, workspace: int = 0, after_minmax=None) -> None:
        self._real, self._after, self._workspace, self._after_minmax = real_lib, after, workspace, after_minmax
        self.path, self.backend_name, self.is_device, self.check = real_lib.path, real_lib.backend_name, real_lib.is_device, real_lib.check

    def __getattr__(self, name):
        attr = getattr(self._real, name)
        if name == "ffq_quantize_by_tile" and self._after is not None:
            def call(*args):
                status = attr(*args)
                if guards._PATCHED:  # (the unguarded run's buffers are torch's own: a defect there would damage the heap)
                    self._after(args)
                return status
            return call
        if name == "ffq_minmax_workspace_bytes" and self._workspace:
            return lambda *args: self._workspace
        if name == "ffq_minmax_by_tile" and self._after_minmax is not None:
            def call(*args):
                status = attr(*args)
                if guards._PATCHED:
                    self._after_minmax(args)
                return status
            return call
        return attr


SHAPE = (5, 24)  # 120 int8 codes: the output ends off every boundary
NUMEL = SHAPE[0] * SHAPE[1]


def quantize(x, s, o):
    return ops.quantize_by_tile(x, s, SHAPE, 8, I8, o)


def operands():
    return (real("cpu", SHAPE, BF16, 1), *one("cpu"))


def found(lib, fn=quantize, inputs=None):
    with pytest.raises(AssertionError) as info:
        guards.check_call(fn, operands() if inputs is None else inputs, library=lib)
    return [line.split()[0] for line in str(info.value).splitlines() if line.split()[0] in ("I1", "I2", "I3", "I4", "I5", "HONESTY")], str(info.value)


def test_the_undamaged_wrapper_passes(oracle_lib):
    guards.check_call(quantize, operands(), library=Defective(oracle_lib))


def test_a_byte_past_an_output_is_I1(oracle_lib):
    def after(args):
        _byte(args[10] + NUMEL).value ^= 0x55
    names, text = found(Defective(oracle_lib, after))
    assert set(names) == {"I1"} and "+0 after" in text and "fresh" in text


def test_a_byte_before_an_output_is_I1(oracle_lib):
    def after(args):
        _byte(args[10] - 1).value ^= 0x55
    names, text = found(Defective(oracle_lib, after))
    assert set(names) == {"I1"} and "-1 before" in text and "fresh" in text


def test_an_output_element_left_at_its_poison_is_I3(oracle_lib):
    def after(args):
        _byte(args[10] + 7).value = _byte(args[10] - 1).value  # (the guard byte before the output holds the run's poison)
    names, text = found(Defective(oracle_lib, after))
    assert set(names) == {"I3"} and "flat index 7" in text


def test_a_flipped_input_byte_is_I2(oracle_lib):
    def after(args):
        _byte(args[0] + 3).value ^= 0x01
    names, text = found(Defective(oracle_lib, after))
    assert set(names) == {"I2"} and "byte 3" in text


def test_a_byte_past_the_workspace_is_I1(oracle_lib):
    def after_minmax(args):
        assert args[8] == 64 and args[7]  # (workspace, workspace_bytes)
        _byte(args[7] + args[8]).value ^= 0x55
    lib = Defective(oracle_lib, workspace=64, after_minmax=after_minmax)
    names, text = found(lib, lambda x: ops.minmax_by_tile(x, SHAPE), (operands()[0],))
    assert set(names) == {"I1"} and "+0 after" in text and "(64,) torch.uint8" in text


def test_a_workspace_shorter_than_the_library_was_told_is_I5(oracle_lib, monkeypatch):
    monkeypatch.setattr(_base, "_workspace", lambda nbytes, device: torch.empty(nbytes - 16, dtype=torch.uint8, device=device) if nbytes > 16 else None)
    monkeypatch.setattr(ops.reductions, "_workspace", _base._workspace)
    names, text = found(Defective(oracle_lib, workspace=64), lambda x: ops.minmax_by_tile(x, SHAPE), (operands()[0],))
    assert set(names) == {"I5"} and "told 64 workspace bytes, handed a buffer of 48" in text


def test_a_ticket_word_left_at_one_is_I4(oracle_lib):
    ticket = {}

    def fn(x, s, o):  # (host calls take no ticket: the test makes the cached word itself, inside the capture)
        if guards._PATCHED:
            ticket["t"] = _base._TICKETS[("test", 0, 0)] = torch.zeros(8, dtype=torch.int32)
        return quantize(x, s, o)

    def after(args):
        ctypes.c_int32.from_address(ticket["t"].data_ptr() + 4 * 5).value = 1
    names, text = found(Defective(oracle_lib, after), fn)
    assert set(names) == {"I4"} and "index 5" in text
    assert ("test", 0, 0) not in _base._TICKETS  # (the capture put the package's own cache back)


def test_extrema_words_left_dirty_are_I4(oracle_lib):
    def fn(x, s, o):
        if guards._PATCHED:
            words = _base._EXTREMA_WORDS[(-1, 0)] = torch.zeros(4, dtype=torch.int32)
            words[1] = 3
        return quantize(x, s, o)
    names, _ = found(Defective(oracle_lib), fn)
    assert set(names) == {"I4"}


def test_a_result_that_reads_an_input_guard_is_I3(oracle_lib):
    def after(args):
        _byte(args[10]).value ^= _byte(args[0] + NUMEL * 2).value  # the first byte of the input's trailing guard
    names, text = found(Defective(oracle_lib, after))
    assert set(names) == {"I3"} and "flat index 0" in text


def test_an_output_allocated_outside_the_arena_is_flagged(oracle_lib):
    def fn(x):
        into = (guards._empty(1, dtype=BF16), guards._empty(1, dtype=BF16))  # torch's own allocator, past the capture
        return ops.minmax_by_tile(x, SHAPE, into=into)
    names, text = found(Defective(oracle_lib), fn, (operands()[0],))
    assert "HONESTY" in names and "not inside an arena body" in text and "does not live in the arena" in text


# ---- the coverage partition (pure Python) -----------------------------------------------------------------------------------------
def test_guarded_and_exempt_partition_the_abi():
    every = set(_cabi.SIGNATURES)
    exempt = set(guards.EXEMPT)
    assert GUARDED | exempt == every, (sorted(every - GUARDED - exempt), sorted((GUARDED | exempt) - every))
    assert not GUARDED & exempt
    # every symbol that takes a stream (the last argument of each launching entry point) is guarded; none is exempt
    assert GUARDED == guards.LAUNCHING, sorted(guards.LAUNCHING ^ GUARDED)
    assert all(isinstance(reason, str) and reason and "\n" not in reason for reason in guards.EXEMPT.values())
    for name in exempt - {"ffq_force_generic_kernels"}:  # pure host queries: no pointer to device memory, a plain return value
        restype, argtypes = _cabi.SIGNATURES[name]
        assert ctypes.c_void_p not in argtypes and restype is not None, name
