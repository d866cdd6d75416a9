"""What the Python wrappers of the search tiers (policy.py, elites.py, novelty.py, pareto.py) decide alike, once: whether two
tensors share memory, whether an argument is the tensor a kernel may be pointed at, the range of a draw's counters, the threshold of
a rate, the four weight pointers of a descriptor, and the launch on the caller's stream.  The wording of a refusal, the order of a
call's checks and the rules by which a call reuses buffers stay with the tier."""
import ctypes as C
import math

import torch

from . import _lib

ARRAYS = _lib.SNES_ARRAYS       # ("w1", "b1", "w2", "b2"): the members of a weight set, in the order of every descriptor


def _span(t):
    """[first byte, past the last byte) of a tensor's elements; None for an empty tensor"""
    n = t.numel()
    if not n:
        return None
    at = t.data_ptr()
    return at, at + n * t.element_size()


def overlaps(a, b):
    """Whether the bytes of two tensors meet -- [data_ptr, data_ptr + numel * element_size) of each; an empty tensor overlaps
    nothing.  Either may be a sequence of tensors: whether any of ``a`` meets any of ``b`` (each span is read once).  (The library
    checks every pair itself; the wrappers ask so that the message can name the argument.)"""
    these = (_span(a),) if isinstance(a, torch.Tensor) else [_span(t) for t in a]
    those = (_span(b),) if isinstance(b, torch.Tensor) else [_span(t) for t in b]
    for s in these:
        for o in those:
            if s is not None and o is not None and s[0] < o[1] and o[0] < s[1]:
                return True
    return False


def is_tensor(t, dtypes, shape, device):
    """Whether ``t`` is one contiguous tensor of that dtype (or one of a tuple of them) and shape (None: any) on ``device`` -- what a
    descriptor's pointer may be taken from.  The caller words the refusal."""
    return (isinstance(t, torch.Tensor) and t.dtype in (dtypes if isinstance(dtypes, tuple) else (dtypes,))
            and (shape is None or tuple(t.shape) == tuple(shape)) and t.is_contiguous() and t.device == device)


def draw_ok(what, generation, seed):
    """The counters of a random stream: ``generation`` is a uint32 of the descriptors, ``seed`` a uint64."""
    if not 0 <= int(generation) < 2 ** 32 or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("%s: generation must fit 32 bits and seed 64 (unsigned)" % what)


def rate_threshold(rate):
    """floor(rate * 2^32), what the library compares a 32-bit draw with for a rate in [0, 1] (the product of a binary64 by 2^32 is
    exact)"""
    return int(math.floor(float(rate) * 4294967296.0))


def point(desc, prefix, tensors):
    """``desc.<prefix>w1 .. <prefix>b2`` = the addresses of the four tensors of a weight set"""
    for k, t in zip(ARRAYS, tensors):
        setattr(desc, prefix + k, t.data_ptr())


def launch(fn, desc, device, wide, stream_member=False):
    """The library call ``fn(&desc, stream)`` queued on the current stream of ``device``, checked.  ``stream_member``: the call takes
    its stream as ``desc.stream`` instead (include/rem2d_cvt.h)."""
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device).cuda_stream
        if stream_member:
            desc.stream = stream
            rc = fn(C.byref(desc))
        else:
            rc = fn(C.byref(desc), C.c_void_p(stream))
        _lib.check(rc, wide)


def scratch_bytes(fn, desc, wide):
    """A ``*_scratch_bytes(&desc)`` of the library: the bytes, a negative value being its error code"""
    n = int(fn(C.byref(desc)))
    if n < 0:
        _lib.check(n, wide)
    return n
