"""Device buffers: what both the batch (core.py) and the learners (learners.py) need, in a module neither of them is."""
import ctypes as C

import numpy as np


class DeviceArray:
    """A caller-owned device buffer allocated through the handle (no torch needed)."""

    def __init__(self, batch, shape, dtype):
        self.batch = batch
        self.shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        batch._check(batch.lib.soccer_malloc(batch.h, self.nbytes, C.byref(p)))
        self.ptr = p.value

    def upload(self, host):
        a = np.ascontiguousarray(host, dtype=self.dtype)
        assert a.nbytes == self.nbytes, "size mismatch: %d vs %d bytes" % (a.nbytes, self.nbytes)
        b = self.batch
        b._check(b.lib.soccer_memcpy_h2d(b.h, self.ptr, a.ctypes.data, self.nbytes))
        return self

    def upload_rows(self, first_row, host):
        """Copy `host` (rows of the same width) into rows first_row.. of a 2-D+ buffer."""
        a = np.ascontiguousarray(host, dtype=self.dtype)
        row_bytes = int(np.prod(self.shape[1:])) * self.dtype.itemsize
        assert a.nbytes % row_bytes == 0 and int(first_row) * row_bytes + a.nbytes <= self.nbytes
        b = self.batch
        b._check(b.lib.soccer_memcpy_h2d(b.h, self.ptr + int(first_row) * row_bytes, a.ctypes.data, a.nbytes))
        return self

    def download_rows(self, first_row, n_rows):
        row_bytes = int(np.prod(self.shape[1:])) * self.dtype.itemsize
        out = np.empty((int(n_rows),) + self.shape[1:], self.dtype)
        b = self.batch
        b._check(b.lib.soccer_memcpy_d2h(b.h, out.ctypes.data, self.ptr + int(first_row) * row_bytes, out.nbytes))
        return out

    def download(self, out=None):
        if out is None:
            out = np.empty(self.shape, self.dtype)
        b = self.batch
        b._check(b.lib.soccer_memcpy_d2h(b.h, out.ctypes.data, self.ptr, self.nbytes))
        return out

    def fill(self, value):
        b = self.batch
        b._check(b.lib.soccer_memset(b.h, self.ptr, int(value), self.nbytes))
        return self

    def row(self, k):
        """Device pointer of row k of a 2-D buffer."""
        return self.ptr + int(k) * self.shape[-1] * self.dtype.itemsize

    def free(self):
        if self.ptr and self.batch.h:
            self.batch.lib.soccer_free(self.batch.h, self.ptr)
        self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _ptr(x):
    """Device pointer of a DeviceArray / torch tensor / int / None."""
    if x is None:
        return None
    if isinstance(x, DeviceArray):
        return x.ptr
    if isinstance(x, int):
        return x
    if hasattr(x, "data_ptr"):          # torch tensor on the handle's device
        return x.data_ptr()
    raise TypeError("expected a DeviceArray, a device tensor or an integer address, got %r" % type(x))
