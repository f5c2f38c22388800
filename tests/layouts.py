"""Views of a tensor in the layouts callers really pass: slices into a larger buffer, strided and permuted views, stride-0
expansions, channels-last. Every view is checked to be what it claims (contiguity, ``data_ptr() % 16``, strides), so a test
cannot quietly run on a fresh, aligned tensor instead.

A :class:`Layout` is a static description (its ``id`` names the kind and the pointer's remainder mod 16, known before any
device exists, so it can parametrize a test); ``layout.make(t)`` builds the view of ``t`` on ``t``'s device. All views but
``expand`` hold exactly the values of ``t``; ``expand`` holds ``t[:1]`` broadcast along dim 0 (callers compare against
``view.clone()``)."""

from __future__ import annotations

from dataclasses import dataclass

import torch

_PAD = 512  # bytes of slack around a view inside its buffer: a view never starts at the buffer's own (aligned) origin


@dataclass(frozen=True)
class Layout:
    kind: str  # "offset" | "transposed" | "step2" | "expand" | "channels_last"
    byte_offset: int = 0  # where the view starts inside its buffer, in bytes past an origin aligned to 64 bytes or more

    @property
    def id(self) -> str:
        return f"{self.kind}@{self.byte_offset}B-ptr{self.byte_offset % 16}"

    def make(self, t: torch.Tensor) -> torch.Tensor:
        view = _BUILD[self.kind](t, self.byte_offset)
        check(view, self, t)
        return view


def _buffer(numel: int, like: torch.Tensor, byte_offset: int) -> tuple[torch.Tensor, int]:
    """A flat buffer of `like`'s dtype with room for `numel` elements starting `byte_offset` bytes past an aligned origin."""
    item = like.element_size()
    assert byte_offset % item == 0, f"{byte_offset} B is not a whole number of {like.dtype} elements"
    start = (_PAD + byte_offset) // item
    buf = torch.full((start + numel + _PAD // item,), 77, dtype=like.dtype, device=like.device)  # (77: not a value a test produces)
    assert buf.data_ptr() % 64 == 0  # (the device allocator's blocks are 512-byte aligned, the host's 64)
    return buf, start


def _offset(t: torch.Tensor, byte_offset: int) -> torch.Tensor:
    buf, start = _buffer(t.numel(), t, byte_offset)
    view = buf[start:start + t.numel()].view(t.shape)
    view.copy_(t)
    return view


def _transposed(t: torch.Tensor, byte_offset: int) -> torch.Tensor:
    """The last two dims stored swapped: ``t.transpose(-1, -2).contiguous()`` at the offset, transposed back."""
    stored = _offset(t.transpose(-1, -2).contiguous(), byte_offset)
    return stored.transpose(-1, -2)


def _step2(t: torch.Tensor, byte_offset: int) -> torch.Tensor:
    """Every other element of a buffer twice as long in the last dim."""
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    stored = _offset(wide, byte_offset)
    view = stored[..., ::2]
    view.copy_(t)
    return view


def _expand(t: torch.Tensor, byte_offset: int) -> torch.Tensor:
    first = _offset(t[:1].contiguous(), byte_offset)
    return first.expand(t.shape)


def _channels_last(t: torch.Tensor, byte_offset: int) -> torch.Tensor:
    """A 4-d tensor stored NHWC, at the offset."""
    stored = _offset(t.permute(0, 2, 3, 1).contiguous(), byte_offset)
    return stored.permute(0, 3, 1, 2)


_BUILD = {"offset": _offset, "transposed": _transposed, "step2": _step2, "expand": _expand, "channels_last": _channels_last}


def check(view: torch.Tensor, layout: Layout, t: torch.Tensor) -> None:
    """The view is what `layout` says it is, and holds `t`'s values (``expand``: those of ``t[:1]``)."""
    assert view.shape == t.shape and view.dtype == t.dtype and view.device == t.device
    assert view.data_ptr() % 16 == layout.byte_offset % 16, (layout.id, view.data_ptr() % 16)
    assert view.storage_offset() * view.element_size() == _PAD + layout.byte_offset, (layout.id, view.storage_offset())
    kind = layout.kind
    if kind == "offset":
        assert view.is_contiguous()
    elif kind == "transposed":
        assert view.dim() >= 2 and view.stride(-2) == 1 and (view.shape[-1] == 1 or view.stride(-1) == view.shape[-2])
        assert not view.is_contiguous() or min(view.shape[-2:]) == 1
    elif kind == "step2":
        assert view.stride(-1) == 2 and not view.is_contiguous()
    elif kind == "expand":
        assert view.stride(0) == 0 and (view.shape[0] == 1 or not view.is_contiguous())
    elif kind == "channels_last":
        assert view.dim() == 4 and view.stride(1) == 1 and view.is_contiguous(memory_format=torch.channels_last)
        assert not view.is_contiguous() or view.shape[1] == 1
    else:
        raise ValueError(kind)
    want = t[:1].expand(t.shape) if kind == "expand" else t
    assert torch.equal(view, want) if not t.is_floating_point() else torch.equal(view.isnan(), want.isnan()) and torch.equal(
        view.nan_to_num(), want.nan_to_num())


def misaligned(item: int) -> list[Layout]:
    """Contiguous views at every pointer remainder an element of `item` bytes can have: 2, 4, 8 (and an odd byte count for
    one-byte elements), plus one that is 16-byte aligned but neither 128- nor 256-byte aligned."""
    offsets = [b for b in (1, 2, 4, 8) if b % item == 0]
    return [Layout("offset", b) for b in offsets] + [Layout("offset", 48)]


def strided(item: int, channels_last: bool = False, expand: bool = False) -> list[Layout]:
    """Non-contiguous views: transposed, step-2 (also at a one-element offset), stride-0 expand, channels-last (also at a
    one-element offset)."""
    out = [Layout("transposed", 0), Layout("step2", 0), Layout("step2", item)]
    if expand:
        out.append(Layout("expand", item))
    if channels_last:
        out += [Layout("channels_last", 0), Layout("channels_last", item)]
    return out


def every(item: int, **kinds: bool) -> list[Layout]:
    return misaligned(item) + strided(item, **kinds)


def ids(layouts: list[Layout]) -> list[str]:
    return [layout.id for layout in layouts]
