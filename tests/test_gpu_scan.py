"""The chunked exclusive scan alone (csrc/k_scan.hip): dfl_scan_counts through its C launcher on guarded buffers -- count[n],
start[n + 1] and chunk_sum sized exactly dfl_scan_num_chunks(n), each between guard bands.  Integers only, so the expectation
is exact equality with numpy: start = the int32 exclusive cumulative sum, start[n] = the total, count all zero afterwards,
the guard bands bit for bit as uploaded (every entry of the three arrays is an output or scratch).

Shapes: n = 0, 1, 3, 4, 5 (the four-per-thread tail); 1023, 1024, 1025 (a second chunk that writes only start[n]); 2047,
2048, 4 * 1024 + 1; 256 * 1024 - 1 and + 1 (the first chunk with 256 chunk totals in front of it); 258 * 1024 + 5 (chunks 257
and 258, where a thread of the loop over the chunk totals takes a second trip).  Data: seeded integers in 0..7, all zeros, a
single 1 in the last entry.  The largest case is 1 MB of integers."""
import ctypes as C

import numpy as np
import pytest

from guarded_buffers import ALL, I32, Pool

pytestmark = pytest.mark.gpu
CHUNK = 1024
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 2047, 2048, 4 * 1024 + 1, 256 * 1024 - 1, 256 * 1024 + 1, 258 * 1024 + 5]


@pytest.fixture(scope="module")
def api():
    from dedflow_amd import api as A
    L = A.lib()  # raises if the HIP library is missing: no fallback
    L.dfl_scan_num_chunks.restype, L.dfl_scan_num_chunks.argtypes = C.c_int32, [C.c_int32]
    L.dfl_scan_counts.restype, L.dfl_scan_counts.argtypes = None, [C.c_int32] + 4 * [C.c_void_p]
    return A


@pytest.fixture
def pool(api):
    p = Pool(api)
    yield p
    p.free()


def _data(kind, n):
    if kind == "random":
        return np.random.default_rng(1000 + n).integers(0, 8, size=n).astype(I32)
    a = np.zeros(n, I32)
    if kind == "last_one" and n:
        a[-1] = 1
    return a


@pytest.mark.parametrize("n", SIZES)
def test_num_chunks(api, n):
    assert api.lib().dfl_scan_num_chunks(n) == (n + 1 + CHUNK - 1) // CHUNK


@pytest.mark.parametrize("kind", ["random", "zeros", "last_one"])
@pytest.mark.parametrize("n", SIZES)
def test_scan_counts(api, pool, n, kind):
    L = api.lib()
    data = _data(kind, n)
    nchunk = L.dfl_scan_num_chunks(n)
    count = pool.slot(data, dtype=I32)
    start = pool.slot(np.full(n + 1, -7, I32), dtype=I32)
    chunk = pool.slot(np.full(nchunk, -7, I32), dtype=I32)
    L.dfl_scan_counts(n, count.ptr, chunk.ptr, start.ptr, L.DflStream())
    api.sync()
    want = np.zeros(n + 1, np.int64)
    np.cumsum(data, dtype=np.int64, out=want[1:])
    assert want[-1] < 2 ** 31
    got = start.check(f"start n={n} {kind}", written=ALL)
    assert got.dtype == I32 and np.array_equal(got, want.astype(I32)), (n, kind)
    assert got[n] == data.sum(dtype=np.int64)
    assert not count.check(f"count n={n} {kind}", written=ALL).any(), (n, kind)
    padded = np.zeros(nchunk * CHUNK, np.int64)
    padded[:n] = data
    assert np.array_equal(chunk.check(f"chunk_sum n={n} {kind}", written=ALL), padded.reshape(nchunk, CHUNK).sum(axis=1)), (n, kind)
