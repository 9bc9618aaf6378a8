"""Tensors as the training step really hands them to the kernels: contiguous VIEWS at an odd offset inside a larger live allocation
(a parameter inside GradBucketReducer's `pflat`, a gradient slot of a flat bucket, a channel slice of a concatenation), not fresh
allocations on a 512-byte boundary with allocator slack behind them.

`embed` puts a tensor `off` elements behind a 16-byte boundary in the middle of one flat allocation whose every other element is a
sentinel: one fixed quiet-NaN bit pattern for floats (a tail that is read and multiplied by a zero weight shows as NaN in the
result), one fixed out-of-range value for int32 (a tail index that is followed shows as a wrong value or a changed pad).  `intact`
compares the pads bit for bit, so a store past either end of the view -- a padded row of a finalizer's block, a 16-byte store on a
4-byte aligned pointer -- is seen even when it stores another NaN.  `pad` (elements, >= 4096 and larger than any overhang the code
under test can have: R * R + R + 1 for a grid's halo) keeps a wrong access INSIDE the allocation: the sentinel is what a wrong kernel
touches, never unmapped memory.  A plain module (like fuzz_cases.py), used by test_embedded_host.py on the CPU and by
test_gpu_embedded.py on the device."""
import torch

NAN_BITS = 0x7FC5A5A5          # a quiet NaN with a payload no arithmetic produces (the canonical quiet NaN is 0x7FC00000)
INT_SENTINEL = 0x7ADEAD00      # int32 tensors that are READ AS NUMBERS (amax words: as a float's bits it is 5.8e35): a word read by mistake dwarfs every true one
INDEX_SENTINEL = -1            # int32 tensors whose values are FOLLOWED (indices, voxel coordinates): out of every range, yet a kernel
                               # that does follow it lands an element (a halo: R * R + R + 1 elements) in front of the row, never far away
MIN_PAD = 4096


def _bits(dtype, sentinel=None):
    if dtype == torch.float32:
        return NAN_BITS
    if dtype == torch.int32:
        return INT_SENTINEL if sentinel is None else int(sentinel)
    raise TypeError(f'embed: float32 or int32 expected, got {dtype}')


def _as_bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def sentinel_filled(numel, dtype, device, sentinel=None):
    """One flat allocation of `numel` elements, every one the dtype's sentinel; starts on a 16-byte boundary."""
    whole = torch.full((int(numel),), _bits(dtype, sentinel), dtype=torch.int32, device=device)
    assert whole.data_ptr() % 16 == 0
    return whole.view(dtype)


def embed(t, off, pad=MIN_PAD, sentinel=None):
    """-> (view, whole): `whole` is one flat allocation of pad + off + t.numel() + pad sentinel elements; `view` is contiguous, shaped
    like t, holds t's values and starts `off` (0..3) elements behind a 16-byte boundary (pad is rounded up to a multiple of 4).
    sentinel: another int32 sentinel than INT_SENTINEL (INDEX_SENTINEL for tensors of indices); hand the same one to `intact`."""
    if off not in (0, 1, 2, 3):
        raise ValueError('embed: off must be 0, 1, 2 or 3')
    if pad < MIN_PAD:
        raise ValueError(f'embed: pad must be at least {MIN_PAD} elements')
    pad = (int(pad) + 3) // 4 * 4
    n = t.numel()
    whole = sentinel_filled(pad + off + n + pad, t.dtype, t.device, sentinel)
    view = whole[pad + off:pad + off + n].view(t.shape)
    view.copy_(t)
    return view, whole


def _span(whole, view):
    """(first, one past last) element of `view`'s storage extent inside `whole`."""
    first = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    extent = 1 + sum((s - 1) * st for s, st in zip(view.shape, view.stride())) if view.numel() else 0
    return first, first + extent


def intact(whole, view, sentinel=None):
    """True when every element of `whole` in front of and behind `view`'s extent still holds the sentinel, bit for bit."""
    lo, hi = _span(whole, view)
    flat = _as_bits(whole.reshape(-1))
    want = _bits(whole.dtype, sentinel)
    return bool((flat[:lo] == want).all()) and bool((flat[hi:] == want).all())


def embed_rows(t, off, extra_channels, pad=MIN_PAD):
    """t (B, C, S) -> (view, whole): the (B, C, S) channel slice [lead : lead + C] of a (B, C + extra_channels, S) sentinel-filled
    tensor that itself sits `off` elements behind a 16-byte boundary inside `whole`: rows contiguous within a sample, samples
    (C + extra_channels) * S apart -- what torch.cat's backward hands out (backend._f32_rows)."""
    if off not in (0, 1, 2, 3):
        raise ValueError('embed_rows: off must be 0, 1, 2 or 3')
    b, c, s = t.shape
    pad = (max(int(pad), MIN_PAD) + 3) // 4 * 4
    lead = extra_channels // 2
    whole = sentinel_filled(pad + off + b * (c + extra_channels) * s + pad, t.dtype, t.device)
    wide = whole[pad + off:pad + off + b * (c + extra_channels) * s].view(b, c + extra_channels, s)
    view = wide[:, lead:lead + c, :]
    view.copy_(t)
    return view, whole


def rows_intact(whole, view):
    """`intact` for a view that does not cover its extent (embed_rows, a channel slice passed as out=): every element of `whole`
    that is not an element of `view` still holds the sentinel."""
    flat = _as_bits(whole.reshape(-1))
    mask = torch.ones(flat.numel(), dtype=torch.bool, device=whole.device)
    first = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    idx = torch.zeros((), dtype=torch.long, device=whole.device)
    for size, stride in zip(view.shape, view.stride()):
        idx = idx.unsqueeze(-1) + torch.arange(size, device=whole.device) * stride
    mask[(idx + first).reshape(-1)] = False
    return bool((flat[mask] == _bits(whole.dtype)).all())


def back_to_back(shapes, off, device, pad=MIN_PAD):
    """-> ([views], whole): float32 tensors of `shapes` laid out one right behind the other with no gap (as a flat gradient bucket
    lays parameters out), the first `off` elements behind a 16-byte boundary, sentinel everywhere (the views included: they are
    destinations)."""
    sizes = [int(torch.Size(s).numel()) for s in shapes]
    pad = (max(int(pad), MIN_PAD) + 3) // 4 * 4
    whole = sentinel_filled(pad + off + sum(sizes) + pad, torch.float32, device)
    views, at = [], pad + off
    for shape, n in zip(shapes, sizes):
        views.append(whole[at:at + n].view(shape))
        at += n
    return views, whole


def group_intact(whole, views):
    """`intact` around a back_to_back group."""
    lo = (views[0].data_ptr() - whole.data_ptr()) // 4
    hi = (views[-1].data_ptr() - whole.data_ptr()) // 4 + views[-1].numel()
    flat = _as_bits(whole)
    return bool((flat[:lo] == NAN_BITS).all()) and bool((flat[hi:] == NAN_BITS).all())


def has_nan(t):
    return bool(torch.isnan(t).any()) if t.is_floating_point() else False
