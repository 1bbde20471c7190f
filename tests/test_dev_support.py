"""The GPU tier's support layer (tests/_dev.py) on the CPU: the shared checks catch what they exist to catch, at the smallest
shapes at which they can go wrong."""
import numpy as np
import pytest
import torch

from _dev import SENTINEL, Fenced, Outputs, Padded, ordered, same_bits, ulps

f32 = np.float32
H, W, PAD = 3, 5, 2
PLANES = [((H, W), torch.uint8), ((H, W), torch.int16), ((H, W), torch.float32), ((H, W, 3), torch.uint8)]
IDS = ["uint8", "int16", "float32", "uint8x3"]


def raw_bytes(t):
    """the tensor's own memory as bytes: a write through it is a write into the buffer"""
    return t.view(torch.uint8).reshape(t.shape[0], -1)


# ---------------------------------------------------------------------------- Padded
@pytest.mark.parametrize("fill", [None, -7.0], ids=["bytes", "value"])
@pytest.mark.parametrize("shape,dtype", PLANES, ids=IDS)
def test_padded_check_catches_one_byte_anywhere_in_the_padding(shape, dtype, fill):
    if fill is not None and dtype == torch.uint8:
        fill = 249                                                # -7 as a byte
    item = torch.empty((), dtype=dtype).element_size() * (shape[2] if len(shape) == 3 else 1)
    row, step = W * item, (W + PAD) * item
    for y, x in ((None, None), (0, row), (H - 1, row), (H - 1, step - 1), (1, step - item)):
        p = Padded.empty(shape, dtype, PAD, fill, device="cpu")
        assert p.view.shape == shape and p.base.shape[1] == W + PAD and p.view.data_ptr() == p.base.data_ptr()
        p.view.zero_()                                            # writing the view is no write into the padding
        if y is None:
            p.check("untouched")
            continue
        raw_bytes(p.base)[y, x] ^= 1
        with pytest.raises(AssertionError, match="row padding of this plane was written"):
            p.check("this plane")


@pytest.mark.parametrize("fill", [None, -7.0], ids=["bytes", "value"])
def test_padded_float_low_byte_alone_is_caught(fill):
    """one low byte of one pad element; with a NaN as the fill, the case no comparison of values can see"""
    p = Padded.empty((H, W), torch.float32, PAD, fill, device="cpu")
    raw_bytes(p.base)[1, 4 * W] ^= 1                              # little endian: the low byte of the first pad element of row 1
    with pytest.raises(AssertionError):
        p.check("plane")
    q = Padded.empty((H, W), torch.float32, PAD, float("nan"), device="cpu")
    q.check("nan-filled")                                         # NaN != NaN, but its bytes are its bytes
    raw_bytes(q.base)[2, 4 * W] ^= 1
    assert torch.isnan(q.base[2, W])                              # still a NaN: no value comparison tells the two apart
    with pytest.raises(AssertionError):
        q.check("nan-filled")


def test_padded_fill_bytes():
    assert (raw_bytes(Padded.empty((H, W), torch.int16, PAD, device="cpu").base) == SENTINEL).all()
    assert (Padded.empty((H, W), torch.int16, PAD, device="cpu").base == -23131).all()
    assert (Padded.empty((H, W, 2), torch.float32, PAD, -7.0, device="cpu").base == -7.0).all()


@pytest.mark.parametrize("shape,dtype", PLANES, ids=IDS)
def test_padded_without_padding_is_dense(shape, dtype):
    p = Padded.empty(shape, dtype, 0, device="cpu")
    p.check("dense")
    assert p.view.is_contiguous() and p.view.shape == p.base.shape and p.view.data_ptr() == p.base.data_ptr()
    p.view.zero_()
    assert not p.base.any()


@pytest.mark.parametrize("pad", [0, PAD])
def test_padded_of_round_trips(pad):
    rng = np.random.default_rng(1)
    for a in (rng.integers(0, 256, (H, W), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
              rng.standard_normal((H, W, 2)).astype(f32)[:, ::-1]):               # the last one is not contiguous
        p = Padded.of(a, pad, device="cpu")
        assert np.array_equal(p.view.numpy(), a) and p.view.stride(0) == (W + pad) * (a.shape[2] if a.ndim == 3 else 1)
        p.check("upload")
    q = Padded.of(np.zeros((H, W), f32), PAD, 3.0, device="cpu")
    assert (q.base[:, W:] == 3.0).all() and not q.view.any()


def test_padded_stack_frames_share_one_base():
    rng = np.random.default_rng(2)
    frames = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(4)]
    views = Padded.stack(frames, PAD, device="cpu")
    assert len(views) == 4 and len({v.untyped_storage().data_ptr() for v in views}) == 1
    for k, (v, f) in enumerate(zip(views, frames)):
        assert np.array_equal(v.numpy(), f) and v.stride(0) == W + PAD and v.storage_offset() == k * H * (W + PAD)
    whole = torch.as_strided(views[0], (4, H, W + PAD), (H * (W + PAD), W + PAD, 1))
    assert (whole[:, :, W:] == SENTINEL).all()
    flow = Padded.stack([np.ones((H, W, 2), f32)] * 2, 1, 3.0, device="cpu")
    assert flow[1].shape == (H, W, 2) and flow[1].stride(0) == 2 * (W + 1) and flow[1].dtype == torch.float32
    assert torch.as_strided(flow[0], (2, H, W + 1, 2), (H * (W + 1) * 2, (W + 1) * 2, 2, 1))[:, :, W].eq(3.0).all()
    dense = Padded.stack(frames, 0, device="cpu")
    assert all(v.is_contiguous() and np.array_equal(v.numpy(), f) for v, f in zip(dense, frames))


# ---------------------------------------------------------------------------- Fenced
def test_fenced_catches_the_lead_the_padding_and_the_tail():
    h, row, pad, lead = 2, 4, 1, 3
    fill = np.arange(8, dtype=np.int32).reshape(h, row) - 3
    n = (lead + h * (row + pad)) * 4
    for at in (None, 0, 4 * lead - 1, 4 * (lead + row), 4 * (lead + row + pad + row) + 3, n, n + 63):
        f = Fenced(h, row, torch.int32, pad, lead, fill, device="cpu")
        assert f.bytes.numel() == n + 64 and f.view.storage_offset() == lead and f.view.stride() == (row + pad, 1)
        assert np.array_equal(f.numpy(), fill)
        if at is None:
            f.check("untouched")
            continue
        f.bytes[at] ^= 1
        with pytest.raises(AssertionError, match="of these rows|around these rows"):
            f.check("these rows")
        assert np.array_equal(f.numpy(), fill)                    # none of them is a byte of a row
    f = Fenced(h, row, torch.int32, pad, lead, device="cpu")
    f.view.zero_()
    f.check("written rows")


# ---------------------------------------------------------------------------- ordered, ulps, same_bits
def test_ordered_steps_by_one_between_neighbours():
    assert ordered(f32(0.0)) == ordered(f32(-0.0)) == 0
    tiny, big = f32(1e-45), np.finfo(f32).max
    assert tiny > 0 and tiny / f32(2) == 0
    for x in (f32(0.0), f32(-0.0), tiny, -tiny, f32(1.0), f32(-1.0), np.nextafter(big, f32(0)), -big, big):
        with np.errstate(over="ignore"):                          # the step up from the largest finite float is to infinity
            up = np.nextafter(x, f32(np.inf))
        assert ordered(up) - ordered(x) == 1, x
    assert np.nextafter(-tiny, f32(np.inf)) == 0 and ordered(-tiny) == -1 and ordered(tiny) == 1       # across zero
    a = np.array([[-np.inf, -2.0, -tiny], [0.0, 1.5, np.inf]], f32)
    assert ordered(a).shape == a.shape and (np.diff(ordered(a).ravel()) > 0).all()
    assert ordered(np.float64(1.0) + 1e-12) == ordered(f32(1.0))                                      # cast to float32 first


def test_ulps_and_same_bits():
    nan = f32(np.nan)
    assert ulps(nan, nan) == 0 and ulps(nan, f32(1.0)) > 1 and ulps(f32(1.0), nan) > 1
    a = np.array([1.0, np.nan, -0.0, 3.0], f32)
    b = np.array([np.nextafter(f32(1.0), f32(2.0)), np.nan, 0.0, 3.0], f32)
    assert ulps(a, b).tolist() == [1, 0, 0, 0]
    assert same_bits(a, a.copy()) and not same_bits(a, b)
    assert not same_bits(np.array([0.0], f32), np.array([-0.0], f32))
    assert not same_bits(np.zeros((2, 3), f32), np.zeros((3, 2), f32)) and not same_bits(np.zeros(6, f32), np.zeros((2, 3), f32))
    assert same_bits(np.zeros((4, 6), f32)[:, ::2], np.zeros((4, 3), f32))


# ---------------------------------------------------------------------------- Outputs
def outputs(pad):
    return Outputs(dict(omega=((H, W), torch.float32), vis=((H, W, 3), torch.uint8), field=((2, 2, 2), torch.float32, -7.0)),
                   dict(cells=((4,), torch.uint8, None), sums=((2, 3), torch.int64, -1), frame=((5,), torch.uint8, 0),
                        profile=((2,), torch.float32, -7.0)), pad, device="cpu")


def test_outputs_come_back_as_they_were_made():
    o = outputs(PAD)
    assert list(o.kw()) == ["omega", "vis", "field", "cells", "sums", "frame", "profile"]
    assert list(o.kw(only=("vis", "sums"))) == ["vis", "sums"] and o.kw(only=("vis",))["vis"] is o.t["vis"]
    assert o.t["vis"].shape == (H, W, 3) and o.t["vis"].stride(0) == 3 * (W + PAD) and o.t["field"].shape == (2, 2, 2)
    got = o.host()
    assert list(got) == list(o.kw())
    assert (got["cells"] == SENTINEL).all() and (got["sums"] == -1).all() and got["sums"].shape == (2, 3)
    assert not got["frame"].any() and (got["profile"] == f32(-7.0)).all() and (got["field"] == f32(-7.0)).all()
    assert (got["vis"] == SENTINEL).all() and (got["omega"].view(np.uint8) == SENTINEL).all()
    dense = outputs(0)
    assert all(v.is_contiguous() for v in dense.t.values())
    dense.host()


@pytest.mark.parametrize("name", ["omega", "vis", "field"])
def test_outputs_host_names_the_plane_whose_padding_was_written(name):
    o = outputs(PAD)
    for v in o.t.values():
        v.zero_()                                                 # what a kernel may write
    o.host()
    base = o.planes[name].base
    raw_bytes(base)[base.shape[0] - 1, -1] ^= 1                   # the last byte of the last pad element
    with pytest.raises(AssertionError, match="row padding of %s was written" % name):
        o.host()
