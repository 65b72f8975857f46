"""CPU: the numpy restatement of the device reduction order (tests/ode_kernels_py.py) is pinned before it judges the
device (tests/test_gpu_ode_kernels.py).

(1) It equals the C oracle's device_order_sum (oracle/shud_oracle_ode.c, written independently from the same kernel
    comment) bit for bit at every reduction size the GPU test uses, for both input families.
(2) Faithfulness: every term passes through at most D = 6 + 4 + ceil(nblk/4096) + 2 + 6 + 4 additions (wave butterfly,
    waves_tree, the finalize accumulator, the two-level accumulator combine, and the finalize's two butterflies), so
    |sum - fsum(term)| <= D u sum|term| / (1 - D u) with u = 2^-53 (Higham, Accuracy and Stability, §4.2: any
    summation order whose longest chain is D additions).  Derived, not measured.
(3) Discriminating power: on the signed family the device-order sum differs in bits from the left-to-right serial sum
    at every size >= 65, and from the same tree with a single finalize accumulator at every size with more than 2048
    partials — so a device that summed in either of those orders would fail the GPU comparison.
(4) Integer family: the sum is the closed-form integer exactly.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest

import ode_kernels_py as K
from conftest import ORACLE_DIR

SIZES = K.SMALL_SIZES + K.LARGE_SIZES
U = 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _lib():
    lib = C.CDLL(os.path.join(ORACLE_DIR, "liboracle.so"))
    lib.oracle_ode_device_order_sum.restype = C.c_double
    lib.oracle_ode_device_order_sum.argtypes = [C.c_long, C.c_void_p]
    return lib


def _oracle_sum(term):
    term = np.ascontiguousarray(term, dtype=np.float64)
    return _lib().oracle_ode_device_order_sum(term.size, term.ctypes.data)


def _bits(x):
    return np.float64(x).view(np.uint64)


@functools.lru_cache(maxsize=2)
def _signed_term(n):
    x, y = K.signed_pair(n)
    t = x * y
    t.setflags(write=False)
    return t


def _int_term(n):
    e = K.integer_entries(n)
    return e * e


def _int_closed_form(n):
    return sum(c * (v + 1) ** 2 for v, c in enumerate(K.integer_counts(n)))


@pytest.mark.parametrize("n", SIZES)
def test_numpy_order_equals_oracle_order(n):
    for name, term in (("signed", _signed_term(n)), ("integer", _int_term(n))):
        got, want = K.device_order_sum(term), _oracle_sum(term)
        assert _bits(got) == _bits(want), (name, n, got, want)


@pytest.mark.parametrize("n", SIZES)
def test_device_order_sum_faithful(n):
    term = _signed_term(n)
    D = 6 + 4 + -(-K.grid_blocks(n) // 4096) + 2 + 6 + 4
    bound = D * U * math.fsum(np.abs(term)) / (1.0 - D * U)
    err = abs(K.device_order_sum(term) - math.fsum(term))
    assert err <= bound, (n, err, bound)


@pytest.mark.parametrize("n", [s for s in SIZES if s >= 65])
def test_order_differs_from_serial_sum(n):
    term = _signed_term(n)
    serial = np.cumsum(term)[-1]                                 # left to right, one running sum
    assert _bits(K.device_order_sum(term)) != _bits(serial), n


@pytest.mark.parametrize("n", [s for s in SIZES if K.grid_blocks(s) > 2048])
def test_order_differs_from_single_finalize_accumulator(n):
    term = _signed_term(n)
    assert _bits(K.device_order_sum(term)) != _bits(K.device_order_sum(term, fin_acc=1)), n


@pytest.mark.parametrize("n", K.LARGE_SIZES)
def test_integer_family_closed_form(n):
    term = _int_term(n)
    want = float(_int_closed_form(n))
    assert K.device_order_sum(term) == want
    assert _oracle_sum(term) == want
    assert sum(K.integer_counts(n)) == n


def test_sum_unchanged_by_unaccumulated_lanes():
    """The water-balance kernels go through the same reduction but hand block_partial the term itself where the
    integrator's hand it 0.0 + term.  The two differ only for a term of -0.0 (0.0 + -0.0 = +0.0), and a -0.0 survives
    the block's tree only if every lane of the 1024-block holds one: so the partials, and with them the total, are
    the same bits whenever not every term of a block is -0.0.  Condition on the inputs here: strictly positive.
    (A per-block property: the small sizes, up to 17 blocks with a one-lane tail, cover it.)"""
    for n in K.SMALL_SIZES:
        term = np.abs(_signed_term(n)) + 2.0 ** -1000
        assert (term > 0.0).all()
        part = K.block_partials(term, 0.0, np.add, accumulated=False)
        assert np.array_equal(part.view(np.uint64), K.block_partials(term, 0.0, np.add).view(np.uint64)), n
        assert _bits(K.finalize(part, 0.0, np.add)) == _bits(K.device_order_sum(term)) == _bits(_oracle_sum(term)), n


def test_device_order_min():
    """fmin tree: identity +inf, a NaN operand is dropped, position of the minimum does not matter"""
    rng = np.random.default_rng(3)
    for n in (1, 65, 1025, 4097 * 1024 + 5):
        t = rng.uniform(1.0, 2.0, n)
        for pos in {0, n - 1, n // 2}:
            u = t.copy()
            u[pos] = 0.5
            assert K.device_order_min(u) == 0.5
            u[(pos + 1) % n] = np.nan
            assert K.device_order_min(u) == (0.5 if n > 1 else np.inf)
