"""Guarded device buffers for the boundary-shape GPU tests: outputs sit
between canary elements, scalars and workspaces start out as garbage, and
inputs are compared with their host copy after the call."""
import numpy as np
import torch

from tests import _gpu as G

NCAN = 64
CANARY = {np.uint64: np.uint64(0xC0FFEE00DEADBEEF),
          np.uint32: np.uint32(0xDEADBEEF),
          np.uint8: np.uint8(0xA5)}


class Out:
    """n elements of dtype on the device with NCAN canaries on each side,
    every element (the payload too) starting out as canary."""

    def __init__(self, n, dtype):
        self.n, self.dtype = int(n), dtype
        self.can = CANARY[dtype]
        self.t = G.dev(np.full(self.n + 2 * NCAN, self.can, dtype))
        self.ptr = self.t.data_ptr() + NCAN * np.dtype(dtype).itemsize

    def read(self, valid=None):
        """the payload, after checking the canaries; with `valid`, the
        payload beyond that many elements must be untouched as well."""
        h = G.host(self.t, self.dtype)
        assert np.all(h[:NCAN] == self.can), "wrote before the output"
        assert np.all(h[NCAN + self.n:] == self.can), \
            "wrote past the output"
        body = h[NCAN:NCAN + self.n]
        if valid is not None:
            assert np.all(body[valid:] == self.can), \
                "wrote past the valid count"
            return body[:valid]
        return body


class In:
    """a host array on the device, with a check that it was left alone."""

    def __init__(self, arr):
        self.h = np.array(arr, order="C")      # private, writable copy
        # a zero-sized input still needs a non-NULL address
        self.t = G.dev(self.h if self.h.size else
                       np.zeros(1, self.h.dtype))
        self.ptr = self.t.data_ptr()

    def check(self):
        if self.h.size:
            got = G.host(self.t, self.h.dtype).reshape(self.h.shape)
            assert np.array_equal(got, self.h), "input changed"


def garbage(n, dtype):
    """n device elements of dtype holding a non-zero pattern: the calls
    under test must zero what their header says they zero."""
    return G.dev(np.full(int(n), CANARY[dtype], dtype))


def filled_ws(nbytes):
    w = G.ws(nbytes)
    w.fill_(0xFF)
    return w


def sync():
    torch.cuda.synchronize()
