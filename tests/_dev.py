"""The GPU tier's buffers, padding checks and float comparisons, each once.

SENTINEL (0xA5) is the byte every buffer is filled with before a kernel sees it, unless a test names a value of its own: a byte
that is still there afterwards was not written.  Padded is h rows of w (x c) elements inside rows `pad` elements longer, with
nothing before the first row and nothing after the last row's padding; its check() compares the bytes of every pad element of
every row with the bytes they were filled with, so a changed low byte of a float counts.  Fenced adds to that `lead` elements
before the first row (an unaligned base) and 64 bytes after the last, and checks those too.  Outputs is a product's planes
(Padded) and flat arrays from one declaration; host() copies them back and checks every plane.  ordered() maps float32 to
integers in which neighbouring floats differ by one, +0.0 and -0.0 both to 0; one unit of ulps() is one such step, and a NaN
against a NaN is none.  Every constructor takes device="cuda"; tests/test_dev_support.py runs them on the CPU."""
import ctypes as C
import os

import numpy as np
import torch

from ripcurrents_amd._lib import ERRORS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESIZE, ESTATE = -1, -5, -6
assert (ERRORS[EINVAL], ERRORS[ESIZE], ERRORS[ESTATE]) == ("RC_EINVAL", "RC_ESIZE", "RC_ESTATE")
SENTINEL = 0xA5


# ---------------------------------------------------------------------------- buffers
def filled(shape, dtype, fill=None, device="cuda"):
    """a dense tensor with every element `fill`, or with every byte SENTINEL where fill is None"""
    if fill is not None:
        return torch.full(tuple(shape), fill, dtype=dtype, device=device)
    t = torch.empty(tuple(shape), dtype=dtype, device=device)
    t.view(torch.uint8).fill_(SENTINEL)
    return t


class Padded:
    """`view`: (h, w, ...) inside `base`: (h, w + pad, ...), the whole filled as filled() does before anything is uploaded."""

    def __init__(self, base, w, fill):
        self.base, self.view, self.w = base, base[:, :w], w
        self.fill = filled((1,), base.dtype, fill, "cpu").view(torch.uint8).numpy()      # one pad element's bytes

    @classmethod
    def empty(cls, shape, dtype, pad=0, fill=None, device="cuda"):
        return cls(filled((shape[0], shape[1] + pad) + tuple(shape[2:]), dtype, fill, device), shape[1], fill)

    @classmethod
    def of(cls, a, pad=0, fill=None, device="cuda"):
        """the host array `a` uploaded into padded rows"""
        t = torch.as_tensor(np.ascontiguousarray(a))
        p = cls.empty(t.shape, t.dtype, pad, fill, device)
        p.view.copy_(t)
        return p

    @staticmethod
    def stack(frames, pad, fill=None, device="cuda"):
        """all frames in one upload -> the list of their views, each in rows `pad` elements longer"""
        t = torch.as_tensor(np.stack(frames))
        base = filled(t.shape[:2] + (t.shape[2] + pad,) + t.shape[3:], t.dtype, fill, device)
        base[:, :, :t.shape[2]] = t.to(device)
        return [base[k, :, :t.shape[2]] for k in range(t.shape[0])]

    def check(self, what):
        if self.base.shape[1] > self.w:
            got = np.ascontiguousarray(self.base[:, self.w:].cpu().numpy()).view(np.uint8).reshape(-1, self.fill.size)
            assert (got == self.fill).all(), "row padding of %s was written" % what


class Fenced:
    """h rows of `row` elements inside a device allocation filled with SENTINEL bytes: `lead` elements before the first row (an
    unaligned base), `pad` elements after every row, 64 bytes after the last."""

    def __init__(self, h, row, dtype, pad=0, lead=0, fill=None, device="cuda"):
        self.h, self.row, self.pad, self.lead = h, row, pad, lead
        self.item = torch.empty((), dtype=dtype).element_size()
        self.step = row + pad
        self.bytes = torch.full(((lead + h * self.step) * self.item + 64,), SENTINEL, dtype=torch.uint8, device=device)
        self.view = torch.as_strided(self.bytes[:(lead + h * self.step) * self.item].view(dtype), (h, row), (self.step, 1), lead)
        if fill is not None:
            self.view.copy_(torch.as_tensor(np.ascontiguousarray(fill).reshape(h, row)).to(device))

    def check(self, what):
        b = self.bytes.cpu().numpy()
        n = self.h * self.step * self.item
        assert (b[:self.lead * self.item] == SENTINEL).all() and (b[self.lead * self.item + n:] == SENTINEL).all(), "fence bytes around %s changed" % what
        rows = b[self.lead * self.item:self.lead * self.item + n].reshape(self.h, self.step * self.item)
        assert (rows[:, self.row * self.item:] == SENTINEL).all(), "row padding of %s was written" % what

    def numpy(self):
        return self.view.cpu().numpy()


class Outputs:
    """planes: {name: (shape, dtype[, fill])}, each a Padded of (h, w, ...) = shape in rows `pad` longer; flat: {name: (shape, dtype,
    initial value)}, dense, None for SENTINEL bytes.  `t` holds what the device entry points take, by name; `views` is the product's
    own last step of host(): its record dtypes and shapes, applied to the dict in place."""

    def __init__(self, planes, flat, pad=0, views=None, device="cuda"):
        self.views = views
        self.planes = {k: Padded.empty(s[0], s[1], pad, *s[2:], device=device) for k, s in planes.items()}
        self.t = {k: p.view for k, p in self.planes.items()}
        self.t.update({k: filled(shape, dtype, init, device) for k, (shape, dtype, init) in flat.items()})

    def kw(self, only=None):
        return {k: v for k, v in self.t.items() if only is None or k in only}

    def host(self):
        """everything copied back, after the check of every plane's padding"""
        for k, p in self.planes.items():
            p.check(k)
        d = {k: v.cpu().numpy() for k, v in self.t.items()}
        if self.views:
            self.views(d)
        return d


# ---------------------------------------------------------------------------- float comparison
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def ordered(a):
    """float32 -> integers in which neighbouring floats differ by one"""
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(a, b):
    """units in the last place between float32 arrays; NaN against NaN is 0"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.where(np.isnan(a) & np.isnan(b), 0, np.abs(ordered(a) - ordered(b)))


# ---------------------------------------------------------------------------- the statements' cases
_REF = {}


def reference(module, ctx, name, case=None):
    """(case, *module.run_case(case, lut)) of a _*_ref module's case, computed once for the session and never changed; `case`:
    one of a test's own, kept under `name` beside the module's"""
    key = (module.__name__, name)
    if key not in _REF:
        case = case or module.cases()[name]
        _REF[key] = (case,) + module.run_case(case, ctx.jet_lut())
    return _REF[key]


# ---------------------------------------------------------------------------- the C ABI, for the refusal tests
NULL = C.c_void_p(None)


def ptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


def raw(ctx):
    """-> (the loaded library, the context's handle)"""
    return ctx._lib, ctx._h
