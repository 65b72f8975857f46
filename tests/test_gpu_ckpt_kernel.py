"""GPU: known answers of the checkpoint's pack kernel (csrc/shud_ckpt.hip) through shud_ckpt_pack_test — one launch
over many segments: destination bytes equal source bytes, the guard words around and between the destinations are
untouched, the per-segment sums equal a numpy uint64 restatement, and the checksum-only mode writes nothing."""
import ctypes as C

import numpy as np
import pytest

from shud_rhs import abi
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu

# one segment each; zero-length segments between non-empty ones; 1024 16-byte records = 2048 words per tile and eight
# tiles = 16384 words per workgroup, so 2047 .. 2050 cross the tile border, 16383 .. 16387 the workgroup border on
# either alignment, and 64 * 1024 + 3 takes five workgroups
WORDS = [255, 0, 1, 2, 0, 256, 257, 1023, 1024, 1025, 0, 2047, 2048, 2049, 2050, 64 * 1024 + 3, 0, 4097,
         16383, 16384, 16385, 16386, 16387]
FILL = 0xA5A5A5A5A5A5A5A5
GUARD = 3


def np_checksum(w):
    w = np.asarray(w, dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(w.sum(dtype=np.uint64)), int((np.arange(1, w.size + 1, dtype=np.uint64) * w).sum(dtype=np.uint64))


def contents(n, rng):
    """random bits with, at the front, middle and end: quiet and signalling NaNs with payloads, +-0, denormals, all ones"""
    w = rng.integers(0, 2**64, size=n, dtype=np.uint64)
    special = np.array([0x7FF8000000000123, 0xFFF8DEADBEEF0001, 0x7FF0000000000001, 0xFFF4000000ABCDEF,   # q/s NaNs
                        0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x800FFFFFFFFFFFFF,   # +-0, denormals
                        0xFFFFFFFFFFFFFFFF, 0x7FF0000000000000], dtype=np.uint64)
    for at in (0, n // 2, n - special.size):
        if 0 <= at and at + special.size <= n:
            w[at:at + special.size] = special
    if 0 < n < special.size:
        w[:] = special[:n]
    return w


def pack(segs, misalign, verify):
    lib = rt.lib()
    nseg = len(segs)
    src = np.concatenate([s for s in segs] + [np.zeros(0, dtype=np.uint64)])
    words = np.array([s.size for s in segs], dtype=np.int64)
    mis = np.array(misalign, dtype=np.int32)
    cap = int(words.sum()) + (GUARD + 2) * (nseg + 2)
    slab = np.zeros(cap, dtype=np.uint64)
    nslab = C.c_int64()
    off = np.zeros(nseg, dtype=np.int64)
    c0, c1 = np.zeros(nseg, dtype=np.uint64), np.zeros(nseg, dtype=np.uint64)
    rc = lib.shud_ckpt_pack_test(nseg, src.ctypes.data_as(abi.c_uint64_p), words.ctypes.data_as(abi.c_int64_p),
                                 mis.ctypes.data_as(abi.c_int32_p), GUARD, FILL, int(verify),
                                 slab.ctypes.data_as(abi.c_uint64_p), cap, C.byref(nslab),
                                 off.ctypes.data_as(abi.c_int64_p), c0.ctypes.data_as(abi.c_uint64_p),
                                 c1.ctypes.data_as(abi.c_uint64_p))
    assert rc == abi.SHUD_OK, lib.shud_rhs_last_error_string()
    return slab[:nslab.value], off, c0, c1


@pytest.fixture(scope="module")
def segments():
    rng = np.random.default_rng(20261021)
    return [contents(n, rng) for n in WORDS]


@pytest.mark.parametrize("phase", ["aligned", "off8", "mixed"])
def test_pack_copies_bytes_keeps_guards_and_sums(segments, phase):
    n = len(segments)
    mis = {"aligned": [0] * n, "off8": [1] * n, "mixed": [k % 2 for k in range(n)]}[phase]
    slab, off, c0, c1 = pack(segments, mis, verify=False)
    covered = np.zeros(slab.size, dtype=bool)
    for k, s in enumerate(segments):
        assert off[k] >= GUARD and off[k] + s.size + GUARD <= slab.size, k
        assert off[k] % 2 == mis[k]                       # the slab offset takes the source's 16-byte phase
        assert slab[off[k]:off[k] + s.size].tobytes() == s.tobytes(), (k, s.size)
        assert not covered[off[k]:off[k] + s.size].any()
        covered[off[k]:off[k] + s.size] = True
        assert (int(c0[k]), int(c1[k])) == np_checksum(s), (k, s.size)
    assert np.all(slab[~covered] == np.uint64(FILL))      # before, between and after the destinations
    assert (~covered).sum() >= GUARD * (n + 1)


def test_verify_mode_same_sums_writes_nothing(segments):
    mis = [k % 2 for k in range(len(segments))]
    slab, _, c0, c1 = pack(segments, mis, verify=True)
    assert np.all(slab == np.uint64(FILL))
    for k, s in enumerate(segments):
        assert (int(c0[k]), int(c1[k])) == np_checksum(s), (k, s.size)
