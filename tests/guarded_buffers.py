"""Guarded device buffers and the parity-record writer shared by the kernel-level GPU tests
(test_gpu_krylov_kernels.py, test_gpu_matrix_kernels.py, test_gpu_assembly_kernels.py, test_gpu_dem_kernels.py,
test_gpu_levelset_kernels.py, test_gpu_scan.py, test_gpu_exchange_kernels.py, test_gpu_laser_kernels.py).  Test infrastructure only.

Every host array sits inside a larger device buffer between guard bands of GUARD sentinels of its own type: a NaN with a
recognisable payload for float64 and float32, a fixed bit pattern for the integer types.  Slot.check compares the bands
and every entry outside a `written` mask bit for bit with what was uploaded.
"""
import json
import os

import numpy as np

F64, F32, I32, U8, U32, U64 = np.float64, np.float32, np.int32, np.uint8, np.uint32, np.uint64
GUARD = 64
SENT = np.array([0x7FF8DEADBEEF0BAD], np.uint64).view(F64)[0]
SENT32 = np.array([0x7FC0BEEF], np.uint32).view(F32)[0]
_FILL = {np.dtype(F64): SENT, np.dtype(F32): SENT32, np.dtype(I32): 0x5A5A5A5A, np.dtype(U8): 0xA5, np.dtype(U32): 0xA5A55A5A,
         np.dtype(U64): 0xA5A55A5AC3C33C3C}
_RAW = {8: np.uint64, 4: np.uint32, 1: np.uint8}


def raw(a):
    """the bits of an array as unsigned integers of the same width"""
    a = np.ascontiguousarray(a)
    return a.view(_RAW[a.dtype.itemsize])


def bits(a):
    return np.ascontiguousarray(a, F64).view(np.uint64)


def sent(n, dtype=F64):
    return np.full(int(n), _FILL[np.dtype(dtype)], dtype)


def assert_bits(got, want, what, dtype=F64):
    g, w = raw(np.ascontiguousarray(got, dtype)), raw(np.asarray(want).astype(dtype))
    assert g.shape == w.shape, what
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, "%s: %d of %d entries differ, first at %d: got %r, want %r" % (
        what, bad.size, g.size, bad[0], np.asarray(got).ravel()[bad[0]], np.asarray(want).ravel()[bad[0]])


class Pool:
    """the guarded device buffers of one test; freed when the test ends"""

    def __init__(self, api):
        self.api, self.slots = api, []

    def slot(self, data, off=0, dtype=F64):
        s = Slot(self.api, data, off, dtype)
        self.slots.append(s)
        return s

    def free(self):
        for s in self.slots:
            s.dev.free()
        self.slots = []


class Slot:
    """a host array inside a larger device buffer: [guard | off | data | guard]"""

    def __init__(self, api, data, off, dtype):
        data = np.ascontiguousarray(data, dtype)
        self.n, self.lo, self.dtype = data.size, GUARD + off, np.dtype(dtype)
        self.image = np.full(self.lo + self.n + GUARD + 1, _FILL[self.dtype], dtype)
        self.image[self.lo: self.lo + self.n] = data
        self.dev = api.DeviceArray(self.image.size, dtype)
        self.dev.upload(self.image)
        self.ptr = self.dev.ptr + self.lo * self.dtype.itemsize
        assert (self.ptr & 15) == (off * self.dtype.itemsize) % 16

    def reset(self, data=None):
        if data is not None:
            self.image[self.lo: self.lo + self.n] = data
        self.dev.upload(self.image)

    def host(self):
        """what was uploaded (without the bands)"""
        return self.image[self.lo: self.lo + self.n]

    def get(self):
        return self.dev.numpy()[self.lo: self.lo + self.n]

    def check(self, what, written=None):
        """bands, and every entry outside the boolean mask `written`, hold what was uploaded; returns the data"""
        now = self.dev.numpy()
        keep = np.ones(now.size, bool)
        if written is not None:
            keep[self.lo: self.lo + self.n] = ~np.broadcast_to(written, (self.n,))
        bad = np.flatnonzero(keep & (raw(now) != raw(self.image)))
        assert bad.size == 0, "%s: %d entries outside the output changed, first at offset %d" % (
            what, bad.size, bad[0] - self.lo)
        return now[self.lo: self.lo + self.n]


ALL = True  # written-mask: the whole array is output


class Recorder:
    """err / bound records of one test module, written to the file named by DFL_PARITY_OUT when the module ends"""

    def __init__(self, mode="w"):
        self.rows, self.mode = [], mode

    def __call__(self, kernel, case, ratio, **extra):
        r = {"kernel": kernel, "case": case, "max_err_over_bound": float(ratio)}
        r.update(extra)
        self.rows.append(r)

    def write(self):
        out = os.environ.get("DFL_PARITY_OUT")
        if out and self.rows:
            with open(out, self.mode) as fh:
                for r in self.rows:
                    fh.write(json.dumps(r) + "\n")
