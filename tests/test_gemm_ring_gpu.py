"""The three-image ring form of the persistent int8 GEMM (csrc/ffq_linear.hip, RING3): the activation operand runs two super-steps
ahead of the MFMAs through three LDS images, the weight operand one super-step through two, and the epilogue works in the two images
the tile's last super-step was computed from (waves 0-3 in the activation image, waves 4-7 in the weight image).

The sums are integer, so whatever the fetch schedule there is one right answer and two oracles for it:
  * the exact contraction computed on the CPU (float64 products of integers below 2^53, held as int64) pushed through the plain
    epilogue's stated fp32 sequence — v = float(acc) + ox * rowsum_w[n];  y = (sx * sw[n]) * v (+ bias) — one IEEE operation per
    torch op, then one rounding to the output dtype;
  * the two-slot form of the same kernel on the same operands, bit for bit.
Either form is selected whatever the launch rule says with bits 3 / 4 of ffq_force_generic_kernels (include/ffq.h), which also lift
the 64-tile floor of the persistent kernel: the shapes here are the smallest at which the ring can go wrong.
"""

import pytest
import torch

from fastforward_amd import ops
from test_fullsize_gpu import exact_accumulators

pytestmark = pytest.mark.gpu
DEV = "cuda"
RING, TWO_SLOT = 8, 16  # ffq_force_generic_kernels: bit 3, bit 4


@pytest.fixture(autouse=True)
def _backend(hip_backend):
    yield


def _forced(bits, fn):
    from fastforward_amd import _native

    lib = _native.library()
    previous = lib.ffq_force_generic_kernels(bits)
    try:
        return fn()
    finally:
        lib.ffq_force_generic_kernels(previous)


def _operands(m, n, k, seed, per_token=False, with_bias=False):
    g = torch.Generator(device=DEV).manual_seed(seed)
    xq = torch.randint(-128, 128, (m, k), device=DEV, dtype=torch.int8, generator=g)
    wq = torch.randint(-128, 128, (n, k), device=DEV, dtype=torch.int8, generator=g)
    rows = m if per_token else 1
    sx = torch.rand(rows, device=DEV, generator=g) * 0.02 + 0.005
    ox = torch.round(torch.randn(rows, device=DEV, generator=g) * 20)
    sw = torch.rand(n, device=DEV, generator=g) * 1e-3 + 2e-4
    bias = torch.randn(n, device=DEV, generator=g).to(torch.bfloat16) if with_bias else None
    return xq, wq, sx, ox, sw, bias


def _exact_output(xq, wq, sx, ox, sw, bias, dtype=torch.bfloat16):
    """The plain epilogue on the exact integer contraction, all of it on the CPU."""
    xc, wc = xq.cpu(), wq.cpu()
    acc = exact_accumulators(xc, wc.double(), slice(0, xc.shape[0]))
    assert int(acc.abs().max()) < 2**24  # float(acc) is the integer itself
    rsw = wc.sum(dim=1, dtype=torch.int64).float()
    v = acc.float() + torch.round(ox.cpu()).reshape(-1, 1) * rsw[None, :]
    y = (sx.cpu().reshape(-1, 1) * sw.cpu()[None, :]) * v
    if bias is not None:
        y = y + bias.cpu().float()[None, :]
    return y.to(dtype)


def _launch(operands, dtype=torch.bfloat16):
    xq, wq, sx, ox, sw, bias = operands
    # (the row sums come with the call: below 64 tiles the forced forms run only where the launch needs no workspace, include/ffq.h)
    return ops.linear_w8a8(xq, wq, sx, ox, sw, None, bias=bias, out_dtype=dtype, w_rowsum=wq.sum(dim=1, dtype=torch.int32))


def _check_both_oracles(operands, dtypes=(torch.bfloat16,)):
    for dtype in dtypes:
        ring = _forced(RING, lambda: _launch(operands, dtype))
        want = _exact_output(*operands, dtype=dtype).to(DEV)
        assert ring.shape == want.shape and torch.equal(ring, want), f"{dtype}: {int((ring != want).sum())} of {want.numel()} outputs differ from the exact contraction"
        two_slot = _forced(TWO_SLOT, lambda: _launch(operands, dtype))
        assert torch.equal(ring, two_slot), f"{dtype}: {int((ring != two_slot).sum())} outputs differ from the two-slot form"


@pytest.mark.parametrize("k", [256, 384, 512, 640, 896])
def test_shortest_loops_and_every_residue_of_the_ring_index(k):
    """K / 128 = 2, 3, 4, 5, 7 at one tile: the shortest legal loop (both prologue images are the whole tile), every residue of the
    image index at the tile's end, and the re-loads after the block's last tile under the epilogue."""
    _check_both_oracles(_operands(256, 256, k, 7000 + k))


def test_ragged_edges_in_every_output_container():
    """M = 300, N = 200: rows past the edge re-read the last row, the cut column tile leaves by element stores — bf16, f16 and fp32
    (the three instantiations of the ring form)."""
    _check_both_oracles(_operands(300, 200, 640, 7101), dtypes=(torch.bfloat16, torch.float16, torch.float32))


@pytest.fixture(scope="module")
def many_tiles():
    """272 tiles on at most 256 blocks: some blocks cross a tile boundary with two activation images of the next tile in flight
    under the epilogue, and use the split scratch a second time. The exact output is computed once for the tests that share it."""
    operands = _operands(4352, 4096, 640, 7202)
    return operands, _exact_output(*operands).to(DEV)


def test_more_tiles_than_blocks(many_tiles):
    operands, want = many_tiles
    ring = _forced(RING, lambda: _launch(operands))
    assert torch.equal(ring, want), f"{int((ring != want).sum())} of {want.numel()} outputs differ from the exact contraction"
    assert torch.equal(ring, _forced(TWO_SLOT, lambda: _launch(operands)))


@pytest.mark.parametrize("m,n", [(256, 256), (1024, 512)], ids=str)
def test_power_of_two_depth_with_the_rotated_start(m, n):
    """K = 8192 turns the per-XCD rotation of the contraction depth on (index arithmetic only): one tile, and eight tiles so that
    every XCD — each with its own starting depth, seven of them wrapping inside the tile — computes one."""
    _check_both_oracles(_operands(m, n, 8192, 7303 + m))


def test_per_token_activation_parameters_and_a_bias():
    _check_both_oracles(_operands(512, 512, 640, 7404, per_token=True, with_bias=True))


def test_ten_repeated_launches_are_bit_identical(many_tiles):
    operands, want = many_tiles
    results = _forced(RING, lambda: [_launch(operands) for _ in range(10)])
    assert all(torch.equal(r, want) for r in results)


def test_capture_and_two_replays_are_bit_identical(many_tiles):
    operands, want = many_tiles
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()

    def capture():
        with torch.cuda.stream(side):
            _launch(operands)  # code objects, allocator
            with torch.cuda.graph(graph, stream=side):
                return _launch(operands)

    captured = _forced(RING, capture)  # the form is chosen on the host when the launch is recorded
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        captured.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(captured, want)


def test_several_outputs_in_one_launch_still_equal_separate_launches():
    """The launch rule keeps q / k / v as one launch on the two-slot form at any depth and size. Forced, the ring form writes the
    three outputs too, and each of the three separate launches gives the same bits on either form."""
    tokens, rows, k = 2048, (1024, 512, 512), 8192
    xq, wq, sx, ox, sw, _ = _operands(tokens, sum(rows), k, 7505)
    got = ops.linear_w8a8_multi(xq, wq, sx, ox, sw, rows)
    assert got is not None and len(got) == 3
    forced = _forced(RING, lambda: ops.linear_w8a8_multi(xq, wq, sx, ox, sw, rows))
    at = 0
    for out, ring_out, n in zip(got, forced, rows):
        one = lambda: ops.linear_w8a8(xq, wq[at:at + n], sx, ox, sw[at:at + n], None, out_dtype=torch.bfloat16, w_rowsum=wq[at:at + n].sum(dim=1, dtype=torch.int32))  # noqa: E731
        separate = one()
        assert torch.equal(out, separate) and torch.equal(ring_out, separate)
        assert torch.equal(_forced(RING, one), separate) and torch.equal(_forced(TWO_SLOT, one), separate)
        at += n
