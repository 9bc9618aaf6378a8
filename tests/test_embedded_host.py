"""The embedded-view helpers of tests/embedded.py on the CPU: offset arithmetic, contiguity, and that `intact` notices ONE changed
pad element -- front or back, first or last, a number or another NaN."""
import pytest
import torch

import embedded as E


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32])
@pytest.mark.parametrize('off', [0, 1, 2, 3])
@pytest.mark.parametrize('shape', [(13,), (3, 5, 7), (2, 4, 8), (1,)])
def test_embed_offsets_contiguity_and_values(dtype, off, shape):
    t = (torch.arange(int(torch.Size(shape).numel())).view(shape) * 3 - 7).to(dtype)
    view, whole = E.embed(t, off)
    assert whole.dim() == 1 and whole.numel() == E.MIN_PAD + off + t.numel() + E.MIN_PAD and whole.dtype == dtype
    assert whole.data_ptr() % 16 == 0 and view.data_ptr() % 16 == 4 * off
    assert view.data_ptr() == whole.data_ptr() + 4 * (E.MIN_PAD + off)
    assert view.is_contiguous() and view.shape == t.shape and view.dtype == dtype and torch.equal(view, t)
    assert view.untyped_storage().data_ptr() == whole.untyped_storage().data_ptr()          # a view, not a copy
    outside = torch.cat([whole[:E.MIN_PAD + off], whole[E.MIN_PAD + off + t.numel():]])
    assert outside.numel() == 2 * E.MIN_PAD + off
    if dtype == torch.float32:
        assert torch.isnan(outside).all() and (outside.view(torch.int32) == E.NAN_BITS).all()
    else:
        assert (outside == E.INT_SENTINEL).all()
    assert E.intact(whole, view)
    view.add_(1)                                                                              # writing the view itself is no damage
    assert E.intact(whole, view)


def test_embed_rejects_what_the_convention_excludes():
    t = torch.zeros(8)
    with pytest.raises(ValueError):
        E.embed(t, 4)
    with pytest.raises(ValueError):
        E.embed(t, -1)
    with pytest.raises(ValueError):
        E.embed(t, 1, pad=64)
    with pytest.raises(TypeError):
        E.embed(t.double(), 1)
    view, whole = E.embed(t, 3, pad=5001)                                                     # pads stay multiples of 4: off is the offset
    assert view.data_ptr() % 16 == 12 and whole.numel() == 2 * 5004 + 3 + 8


@pytest.mark.parametrize('dtype', [torch.float32, torch.int32])
@pytest.mark.parametrize('off', [0, 3])
def test_intact_sees_any_single_pad_element(dtype, off):
    t = torch.ones(10, dtype=dtype)
    first, last = E.MIN_PAD + off, E.MIN_PAD + off + 10
    for where in (0, 1, first - 1, last, last + 1, 2 * E.MIN_PAD + off + 9, E.MIN_PAD // 2, last + E.MIN_PAD // 2):
        view, whole = E.embed(t, off)
        assert E.intact(whole, view)
        whole[where] = 0
        assert not E.intact(whole, view), where
    if dtype == torch.float32:
        for where, bits in ((first - 1, 0x7FC00000), (last, 0x7FC00000), (0, E.NAN_BITS ^ 1), (last + 7, E.NAN_BITS | (1 << 31))):
            view, whole = E.embed(t, off)
            whole.view(torch.int32)[where] = bits if bits < (1 << 31) else bits - (1 << 32)  # another NaN is damage, too
            assert torch.isnan(whole[where]) and not E.intact(whole, view), (where, hex(bits))


def test_index_tensors_take_a_sentinel_of_their_own():
    idx = torch.arange(12, dtype=torch.int32).view(3, 4)
    view, whole = E.embed(idx, 2, sentinel=E.INDEX_SENTINEL)
    assert torch.equal(view, idx) and int((whole == E.INDEX_SENTINEL).sum()) == 2 * E.MIN_PAD + 2
    assert E.intact(whole, view, E.INDEX_SENTINEL) and not E.intact(whole, view)
    whole[-1] = E.INT_SENTINEL
    assert not E.intact(whole, view, E.INDEX_SENTINEL)


@pytest.mark.parametrize('off', [0, 1, 2, 3])
def test_embed_rows_is_a_channel_slice_with_a_batch_stride(off):
    t = torch.arange(2 * 3 * 8, dtype=torch.float32).view(2, 3, 8)
    view, whole = E.embed_rows(t, off, 5)
    assert torch.equal(view, t) and not view.is_contiguous()
    assert view.stride() == (8 * 8, 8, 1) and view.data_ptr() == whole.data_ptr() + 4 * (E.MIN_PAD + off + 2 * 8)
    assert E.rows_intact(whole, view)
    assert int(torch.isnan(whole).sum()) == whole.numel() - t.numel()
    for where in (0, E.MIN_PAD + off, E.MIN_PAD + off + 2 * 8 - 1, E.MIN_PAD + off + 5 * 8, E.MIN_PAD + off + 8 * 8 + 1, whole.numel() - 1):
        view, whole = E.embed_rows(t, off, 5)                                                  # ... between the samples included
        whole[where] = 1.0
        assert not E.rows_intact(whole, view), where
    one, whole = E.embed_rows(t[:1], off, 4)
    assert E.rows_intact(whole, one) and one.shape == (1, 3, 8)


def test_back_to_back_leaves_no_gap():
    for off in range(4):
        (b, w), whole = E.back_to_back([(7,), (7, 5)], off, 'cpu')
        assert b.data_ptr() % 16 == 4 * off and w.data_ptr() == b.data_ptr() + 4 * 7 and w.is_contiguous()
        assert E.group_intact(whole, [b, w])
        b.zero_(); w.zero_()
        assert E.group_intact(whole, [b, w])
        whole[E.MIN_PAD + off + 7 + 35] = 0.0                                                # one past the second destination
        assert not E.group_intact(whole, [b, w])
        (b, w), whole = E.back_to_back([(7,), (7, 5)], off, 'cpu')
        whole[E.MIN_PAD + off - 1] = 0.0                                                     # one before the first
        assert not E.group_intact(whole, [b, w])
