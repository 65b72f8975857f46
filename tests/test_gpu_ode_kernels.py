"""GPU: every launcher of the integrator's vector kernels (shud_ode_dev.h, the code objects of libshud_rhs.so reached
through libshud_kat.so's shud_kat_ode_run) against the plain numpy restatement tests/ode_kernels_py.py.

All comparisons are exact: vectors and reduced slots by their uint64 bits (the sign of zero counts; where the
reference is NaN a NaN is required).  Every reduction case also checks the host-mapped twin, the sequence word, the
error word and that no slot outside [slot0, slot0 + nacc) was written.

Sizes: ode_kernels_py.SMALL_SIZES for every launcher; LARGE_SIZES (1024, 1025, 4096, 4097 and 5122 partials: the
finalize's three regimes, the guarded loads of a ragged trip and the [a * nblk + b] partial layout at large nblk)
for every reduction launcher, with a signed cancelling family (restated order) and a small-integer family (closed
form, order-free: a dropped, duplicated or misplaced partial changes it).
"""
import ctypes as C
import functools
import itertools
import os

import numpy as np
import pytest

import ode_kernels_py as K
from conftest import PKG_DIR

pytestmark = pytest.mark.gpu

OPS = {name: i for i, name in enumerate(
    ["EWT", "PREDICT", "PREDICT_PEND", "RESTORE", "RESCALE", "VSUM", "VSUM_ZERO", "COPY", "SCALE_TO", "ZERO",
     "AXPY_MULTI", "RESIDUAL", "KRYLOV_V0", "DQ_WORK", "ATIMES", "MGS", "NORMALIZE", "NEWTON", "COMPLETE",
     "COMPLETE_EWT", "ETA_NORMS", "DKY"])}
MAXV, NI, ND = 5, 12, 4
NSLOT = K.S_COUNT + 2
SENT = -(4096.0 + np.arange(NSLOT))          # a distinct sentinel per slot: an unwritten slot still holds it


@functools.lru_cache(maxsize=None)
def _lib():
    from shud_rhs import runtime as rt
    rt.lib()
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    vp = C.c_void_p
    lib.shud_kat_ode_run.restype = C.c_int
    lib.shud_kat_ode_run.argtypes = [C.c_int, C.c_int64, vp, vp, vp, vp, vp, vp, vp, vp, C.c_uint64, C.c_int,
                                     C.c_uint32]
    lib.shud_kat_ode_grid_blocks.argtypes = [C.c_int64]
    s, l, q = C.c_int(), C.c_int(), C.c_int()
    assert lib.shud_kat_ode_slots(C.byref(s), C.byref(l), C.byref(q)) == len(OPS)
    assert (s.value, l.value, q.value) == (K.S_COUNT, K.MAXL, K.QMAX)          # the restatement's constants
    return lib


def run(op, n, vecs, ip=(), dp=(), c0=None, c1=None, ds=None, seq=1, err=None):
    """one launcher (+ its finalize) on copies of vecs (arrays of n or (cols, n) entries, or None: absent)
    -> (rc, vectors after, ds after, hds after); ds: {slot: value} over the sentinels"""
    lib = _lib()
    arrs = [None if v is None else np.array(v, dtype=np.float64, order="C") for v in vecs] + [None] * (MAXV - len(vecs))
    cols = np.array([0 if a is None else a.size // n if n > 0 else 1 for a in arrs], dtype=np.int32)
    ptrs = (C.c_void_p * MAXV)(*[None if a is None else a.ctypes.data for a in arrs])
    ipa = np.zeros(NI, dtype=np.int32)
    ipa[:len(ip)] = ip
    dpa = np.zeros(ND)
    dpa[:len(dp)] = dp
    cs = []
    for c in (c0, c1):
        a = np.zeros(K.MAXL + 1)
        if c is not None:
            a[:len(c)] = c
        cs.append(a)
    dsa = SENT[:K.S_COUNT].copy()
    for k, v in (ds or {}).items():
        dsa[k] = v
    hds = SENT.copy()
    rc = lib.shud_kat_ode_run(OPS[op], n, ipa.ctypes.data, dpa.ctypes.data, cs[0].ctypes.data, cs[1].ctypes.data,
                              C.cast(ptrs, C.c_void_p), cols.ctypes.data, dsa.ctypes.data, hds.ctypes.data,
                              seq, int(err is not None), 0 if err is None else err)
    return rc, arrs, dsa, hds


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def assert_same(got, want, what):
    got, want = np.atleast_1d(np.asarray(got, dtype=np.float64)), np.atleast_1d(np.asarray(want, dtype=np.float64))
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ok = (_bits(got) == _bits(want)) | (np.isnan(want) & np.isnan(got))
    if not ok.all():
        i = np.unravel_index(int(np.argmax(~ok)), ok.shape)
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} entries differ, first at {i}: "
                             f"got {got[i]!r} want {want[i]!r}")


def _ds_base(ds_in):
    base = SENT[:K.S_COUNT].copy()
    for k, v in ds_in.items():
        base[k] = v
    return base


def _word(x):
    return int(np.float64(x).view(np.uint64))


def check_slots(what, ds, hds, ds_in, slot0, want, seq, err):
    """reduced slots, twin, sequence word, error word, untouched neighbours"""
    for a, w in enumerate(want):
        assert_same(ds[slot0 + a], w, f"{what}: ds[{slot0 + a}]")
        assert _bits(hds[slot0 + a]) == _bits(ds[slot0 + a]) or (np.isnan(ds[slot0 + a]) and np.isnan(hds[slot0 + a])), \
            f"{what}: hds[{slot0 + a}]"
    assert _word(hds[K.S_COUNT + 1]) == seq, what
    if err is not None:
        assert _word(hds[K.S_COUNT]) & 0xFFFFFFFF == err, what
    else:
        assert hds[K.S_COUNT] == SENT[K.S_COUNT], what
    keep = np.ones(K.S_COUNT, dtype=bool)
    keep[slot0:slot0 + len(want)] = False
    assert_same(ds[keep], _ds_base(ds_in)[keep], f"{what}: ds outside the result slots")
    assert_same(hds[:K.S_COUNT][keep], SENT[:K.S_COUNT][keep], f"{what}: hds outside the result slots")


# ---- input families -------------------------------------------------------------------------------------------------
class Signed:
    """signed cancelling vectors (ode_kernels_py.signed_pair), weights 10^U(-3, 3) where a kernel divides by ewt"""
    exact = False

    def __init__(self, n, seed=11):
        self.n = n
        self.rng = np.random.default_rng(seed)
        self._pair = []

    def v(self):
        if not self._pair:
            self._pair = list(K.signed_pair(self.n, int(self.rng.integers(1 << 30))))
        return self._pair.pop()

    def w(self):
        return 10.0 ** self.rng.uniform(-3, 3, self.n)

    def s(self, val, ival):
        return val


class Ints:
    """entries 1..7 by block index, ewt = 1, coefficients 1 (or the stated integer)"""
    exact = True

    def __init__(self, n):
        self.n = n

    def v(self):
        return K.integer_entries(self.n)

    def w(self):
        return np.ones(self.n)

    def s(self, val, ival):
        return ival


class Ints7(Ints):
    """the seven distinct entries once: the per-value terms of the closed form"""

    def __init__(self):
        self.n = 7

    def v(self):
        return np.arange(1.0, 8.0)


# ---- reduction launchers: one case = device arguments + the restatement's call --------------------------------------
def c_ewt(f):
    zn0, rtol, atol = f.v(), f.s(1e-6, 0.0), f.s(1e-10, 1.0)
    return dict(op="EWT", vecs=[zn0, np.zeros(f.n)], dp=[rtol, atol], outs={1: "ewt"}, slot0=K.S_EWTMIN,
                ref=lambda: K.ewt_set(zn0, rtol, atol))


def c_residual(f, with_ycor=True):
    zn1, ycor, ft, e = f.v(), f.v() if with_ycor else None, f.v(), f.w()
    rl1, ng = f.s(0.75, 1.0), f.s(-0.3, 1.0)
    return dict(op="RESIDUAL", vecs=[zn1, ycor, ft, e, np.zeros(f.n)], dp=[rl1, ng], outs={4: "delta"},
                slot0=K.S_RES, ref=lambda: K.residual(zn1, ycor, ft, rl1, ng, e))


def c_krylov_v0(f):
    d, e, c = f.v(), f.w(), f.s(1.7, 1.0)
    return dict(op="KRYLOV_V0", vecs=[d, e, np.zeros(f.n)], dp=[c], outs={2: "V0"}, slot0=K.S_SIG,
                ref=lambda: K.krylov_v0(d, e, c))


def c_atimes(f):
    w, fy, V, e, V0 = f.v(), f.v(), f.v(), f.w(), f.v()
    if f.exact:
        fy = 3.0 * fy                                    # jv = w - fy = -2e, z = jv + e: x = -e
    ng = f.s(-0.37, 1.0)
    ds = {K.S_SIG: f.s(3.7, 1.0) * f.n}
    return dict(op="ATIMES", vecs=[w, fy, V, e, V0], dp=[ng], ds=ds, outs={0: "w"}, slot0=K.S_W,
                ref=lambda: K.atimes(w, fy, V, e, V0, ng, ds))


def c_mgs(f, prev=True, nxt=True, slot0=K.S_H0 + 3):
    w, Vp, Vn = f.v(), f.v() if prev else None, f.v() if nxt else None
    hslot = slot0 - 1
    ds = {hslot: f.s(0.6, -1.0)}
    return dict(op="MGS", vecs=[w, Vp, Vn], ip=[hslot, slot0], ds=ds, outs={0: "w"} if prev else {}, slot0=slot0,
                ref=lambda: K.mgs(w, Vp, ds, hslot, Vn))


def c_normalize(f):
    w, c, e = f.v(), f.s(1.3, 2.0), f.w()
    return dict(op="NORMALIZE", vecs=[w, e], dp=[c], outs={0: "w"}, slot0=K.S_SIG, ref=lambda: K.normalize(w, c, e))


def c_newton(f, krydim=5, dsrc=False, ycor_zero=False):
    V = np.stack([f.v() for _ in range(krydim)]) if krydim else None
    yg = [f.s(0.9 - 0.17 * k, 1.0) for k in range(krydim)]
    d, e, yc = f.v() if dsrc else None, f.w(), f.v()
    return dict(op="NEWTON", vecs=[V, d, e, yc], ip=[krydim, int(ycor_zero)], c0=yg, outs={3: "ycor"},
                slot0=K.S_DEL, ref=lambda: K.newton_update(V, krydim, yg, d, e, yc, ycor_zero))


def c_complete_ewt(f, q=0, copy_to=-1, jst=1):
    zn, acor = np.stack([f.v() for _ in range(K.QMAX + 1)]), f.v()
    l = [f.s(1.0 / (j + 1.5), 1.0) for j in range(K.QMAX + 1)]
    rtol, atol = f.s(1e-6, 0.0), f.s(1e-10, 1.0)
    return dict(op="COMPLETE_EWT", vecs=[zn, acor, np.zeros(f.n)], ip=[q, copy_to, jst], dp=[rtol, atol], c0=l,
                outs={0: "zn", 2: "ewt_next"}, slot0=K.S_EWTMIN,
                ref=lambda: K.complete_step_ewt(zn, acor, l, q, copy_to, jst, rtol, atol))


def c_eta_norms(f, has_q=True, has_qmax=True, pq=True):
    znq, znm, acor, e = f.v() if has_q else None, f.v() if has_qmax else None, f.v(), f.w()
    nc, lq = f.s(-0.8, 1.0), f.s(0.4, 1.0)
    if not (has_qmax or pq):
        acor = None                                       # the kernel then loads no acor: null is allowed
    return dict(op="ETA_NORMS", vecs=[znq, znm, acor, e], ip=[int(pq)], dp=[nc, lq], outs={}, slot0=K.S_ETAQM1,
                ref=lambda: K.eta_norms(znq, znm, acor, nc, e, int(pq), lq))


RED_CASES = dict(ewt=c_ewt, residual=c_residual, krylov_v0=c_krylov_v0, atimes=c_atimes, mgs=c_mgs,
                 normalize=c_normalize, newton_update=c_newton, complete_step_ewt=c_complete_ewt,
                 eta_norms=c_eta_norms)


def run_case(case, n, what, seq=1, err=None, want=None):
    """run one case; vectors against the restatement; slots against `want` (default: the restated order)"""
    rc, vecs, ds, hds = run(case["op"], n, case["vecs"], case.get("ip", ()), case.get("dp", ()), case.get("c0"),
                            case.get("c1"), case.get("ds"), seq, err)
    assert rc == 0, (what, rc)
    outs, accs = case["ref"]()
    for k, name in case["outs"].items():
        assert_same(vecs[k].reshape(np.shape(outs[name])), outs[name], f"{what}: {name}")
    for k, v in enumerate(case["vecs"]):                 # a vector the launcher does not write is unchanged
        if v is not None and k not in case["outs"]:
            assert_same(vecs[k].reshape(np.shape(v)), v, f"{what}: input vector {k}")
    if accs:
        check_slots(what, ds, hds, case.get("ds", {}), case["slot0"], K.reduce_accs(accs) if want is None else want,
                    seq, err)
    else:
        assert_same(ds, _ds_base(case.get("ds", {})), f"{what}: ds")
        assert_same(hds, SENT, f"{what}: hds")
    return ds


@pytest.mark.parametrize("name", list(RED_CASES))
def test_reduction_launcher_small_sizes(name):
    for k, n in enumerate(K.SMALL_SIZES):
        err = 0x5 if k % 2 == 0 else None
        run_case(RED_CASES[name](Signed(n, seed=100 + k)), n, f"{name} n={n}", seq=1000 + k, err=err)


@pytest.mark.parametrize("n", K.LARGE_SIZES)
@pytest.mark.parametrize("name", list(RED_CASES))
def test_reduction_launcher_large_signed(name, n):
    run_case(RED_CASES[name](Signed(n)), n, f"{name} n={n}", seq=(1 << 40) + n, err=0x5)


@pytest.mark.parametrize("n", K.LARGE_SIZES)
@pytest.mark.parametrize("name", list(RED_CASES))
def test_reduction_launcher_large_integer_closed_form(name, n):
    """expected slots: sum over the values 1..7 of (entries holding it) * (the kernel's term for it), in Python
    integers — no restated order involved"""
    _, accs7 = RED_CASES[name](Ints7())["ref"]()
    cnt = K.integer_counts(n)
    want = []
    for t7, mn in accs7:
        assert all(float(t).is_integer() for t in t7)
        if mn:
            want.append(float(min(int(t) for t, c in zip(t7, cnt) if c)))
        else:
            tot = sum(int(t) * c for t, c in zip(t7, cnt))
            assert abs(tot) < 2 ** 53
            want.append(float(tot))
    assert any(w != 0.0 for w in want)
    run_case(RED_CASES[name](Ints(n)), n, f"{name} n={n}", seq=7, err=None, want=want)


# ---- the min accumulator -------------------------------------------------------------------------------------------
N_MIN = K.LARGE_SIZES[-1]
MIN_POS = dict(first=0, last=N_MIN - 1, block1024=1024 * 1024, block4096=4096 * 1024)


@functools.lru_cache(maxsize=1)
def _min_base():
    y = np.random.default_rng(5).uniform(1.0, 2.0, N_MIN) * np.where(np.arange(N_MIN) % 3 == 0, -1.0, 1.0)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("where", list(MIN_POS))
@pytest.mark.parametrize("name", ["ewt", "complete_step_ewt"])
def test_min_accumulator_position(name, where):
    """the unique minimum of rtol|y| + atol at entry 0, at entry n - 1 (inside the ragged tail), at the first entry of
    block 1024 (the first partial of acc[1]) and of block 4096 (the first partial of the second trip)"""
    n, pos = N_MIN, MIN_POS[where]
    y = _min_base().copy()
    y[pos] = 0.125
    rtol, atol = 1e-3, 1e-6
    if name == "ewt":
        case = dict(op="EWT", vecs=[y, np.zeros(n)], dp=[rtol, atol], outs={1: "ewt"}, slot0=K.S_EWTMIN,
                    ref=lambda: K.ewt_set(y, rtol, atol))
        tmin = rtol * 0.125 + atol
    else:
        l = [1.0]                                         # zn[0] = 1*acor + zn[0] = 2y: the minimum stays where it is
        case = dict(op="COMPLETE_EWT", vecs=[y, y, np.zeros(n)], ip=[0, -1, 1], dp=[rtol, atol], c0=l,
                    outs={2: "ewt_next"}, slot0=K.S_EWTMIN,
                    ref=lambda: K.complete_step_ewt(y.reshape(1, n), y, l, 0, -1, 1, rtol, atol))
        tmin = rtol * 0.25 + atol
    ds = run_case(case, n, f"{name} min at {where}", seq=3, err=0x5)
    assert ds[K.S_EWTMIN] == tmin


@pytest.mark.parametrize("name", ["ewt", "complete_step_ewt"])
def test_min_ignores_nan_sum_keeps_it(name):
    """a NaN in zn0: fmin drops it (the min is that of the other entries), the sum of squares is NaN"""
    n = 4 * 1024 + 77
    y = np.random.default_rng(6).uniform(1.0, 2.0, n)
    y[1500] = np.nan
    y[3000] = 0.5
    rtol, atol = 1e-3, 1e-6
    with np.errstate(invalid="ignore"):
        if name == "ewt":
            case = dict(op="EWT", vecs=[y, np.zeros(n)], dp=[rtol, atol], outs={1: "ewt"}, slot0=K.S_EWTMIN,
                        ref=lambda: K.ewt_set(y, rtol, atol))
        else:
            a = np.zeros(n)
            case = dict(op="COMPLETE_EWT", vecs=[y, a, np.zeros(n)], ip=[0, -1, 0], dp=[rtol, atol], c0=[1.0],
                        outs={0: "zn", 2: "ewt_next"}, slot0=K.S_EWTMIN,
                        ref=lambda: K.complete_step_ewt(y.reshape(1, n), a, [1.0], 0, -1, 0, rtol, atol))
        ds = run_case(case, n, f"{name} NaN", seq=4)
    assert ds[K.S_EWTMIN] == rtol * 0.5 + atol and np.isnan(ds[K.S_NRM])


# ---- variants -------------------------------------------------------------------------------------------------------
def _slab(rng, n, cols=K.QMAX + 1):
    """a Nordsieck-like slab: signed values over several decades with signed zeros sprinkled in"""
    z = rng.standard_normal((cols, n)) * 10.0 ** rng.uniform(-2, 2, (cols, n))
    z[rng.random((cols, n)) < 0.05] = -0.0
    z[rng.random((cols, n)) < 0.05] = 0.0
    return z


def _ew_case(op, vecs, outs, ref, **kw):
    return dict(op=op, vecs=vecs, outs=outs, ref=ref, slot0=0, **kw)


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5])
def test_predict_restore(q):
    rng = np.random.default_rng(20 + q)
    for n in K.SMALL_SIZES:
        zn = _slab(rng, n)
        for with_y in (False, True):
            y = np.full(n, 9.0) if with_y else None
            run_case(_ew_case("PREDICT", [zn, y, np.full(n, 8.0)], {0: "zn", 1: "y"} if with_y else {0: "zn"},
                              lambda: K.predict(zn, q, with_y), ip=[q]), n, f"predict q={q} n={n} y={with_y}")
        run_case(_ew_case("RESTORE", [zn], {0: "zn"}, lambda: K.restore(zn, q), ip=[q]), n, f"restore q={q} n={n}")


@pytest.mark.parametrize("q", [1, 2, 3, 4, 5])
def test_predict_pend(q):
    """the deferred cvCompleteStep (+ cvRescale) applied in registers: j0, resc, copy_to (5 only for q < 5, as
    cvCompleteStep guarantees), with and without y, ycor aliasing pd.acor"""
    rng = np.random.default_rng(30 + q)
    l = [1.0, 1.0] + [0.37 / j for j in range(2, K.QMAX + 1)]
    r = [0.0] + [0.83 ** j for j in range(1, K.QMAX + 1)]
    for n in K.SMALL_SIZES:
        zn, acor = _slab(rng, n), _slab(rng, n, 1)[0]
        for j0, resc, copy_to, with_y, alias in itertools.product((0, 1), (0, 1), (-1, 5) if q < 5 else (-1,),
                                                                  (False, True), (0, 1)):
            y = np.full(n, 9.0) if with_y else None
            run_case(_ew_case("PREDICT_PEND", [zn, y, acor], {0: "zn", 1: "y"} if with_y else {0: "zn"},
                              lambda: K.predict_pend(zn, q, with_y, acor, l, r, j0, resc, copy_to),
                              ip=[q, j0, resc, copy_to, alias], c0=l, c1=r), n,
                     f"predict_pend q={q} n={n} j0={j0} resc={resc} copy_to={copy_to} y={with_y} alias={alias}")


def test_rescale_axpy_multi_complete_step():
    """every (jlo, jhi / q) the controller passes: rescale q = 1..5; cvIncreaseBDF (src = q + 1, columns 2..q, q < 5),
    cvDecreaseBDF (src = q, columns 2..q - 1); materialize (j0 in {0, 1}, q, copy_to) and materialize0 (0, 0, -1)"""
    rng = np.random.default_rng(40)
    c = [0.0] + [0.61 ** j for j in range(1, K.QMAX + 2)]
    for n in K.SMALL_SIZES:
        zn, acor = _slab(rng, n), _slab(rng, n, 1)[0]
        for q in range(1, K.QMAX + 1):
            run_case(_ew_case("RESCALE", [zn], {0: "zn"}, lambda: K.rescale(zn, q, c), ip=[q], c0=c), n,
                     f"rescale q={q} n={n}")
        axpy = [(q + 1, 2, q) for q in range(1, K.QMAX)] + [(q, 2, q - 1) for q in range(2, K.QMAX + 1)]
        for src, jlo, jhi in axpy:
            run_case(_ew_case("AXPY_MULTI", [zn], {0: "zn"}, lambda: K.axpy_multi(zn, src, c, jlo, jhi),
                              ip=[src, jlo, jhi], c0=c), n, f"axpy_multi src={src} [{jlo}, {jhi}] n={n}")
        comp = [(j0, q, ct) for j0 in (0, 1) for q in range(1, K.QMAX + 1) for ct in ((-1, 5) if q < 5 else (-1,))]
        for jlo, q, ct in comp + [(0, 0, -1)]:
            run_case(_ew_case("COMPLETE", [zn, acor], {0: "zn"}, lambda: K.complete_step(zn, acor, c, jlo, q, ct),
                              ip=[jlo, q, ct], c0=c), n, f"complete_step jlo={jlo} q={q} copy_to={ct} n={n}")


def test_complete_step_ewt_variants():
    """jst 0 and 1 (zn[0] stored or left pending), every q, copy_to; the controller's own call is (q 0, -1, jst 1)"""
    for k, n in enumerate(K.SMALL_SIZES):
        for q, jst in itertools.product(range(K.QMAX + 1), (0, 1)):
            for ct in (-1, 5) if q < 5 else (-1,):
                run_case(c_complete_ewt(Signed(n, seed=50 + k), q, ct, jst), n,
                         f"complete_step_ewt q={q} copy_to={ct} jst={jst} n={n}", seq=q + 1, err=0x5)


def test_vsum_scale_copy_zero_signed_zeros():
    """-0.0 + 0.0 is +0.0 in k_vsum_zero and in predict's y = zn[0] + 0.0; scale_to in place (x == z)"""
    rng = np.random.default_rng(60)
    for n in K.SMALL_SIZES:
        x, y = _slab(rng, n, 1)[0], _slab(rng, n, 1)[0]
        x[::3] = -0.0
        y[::6] = 0.0
        junk = np.full(n, 7.0)
        run_case(_ew_case("VSUM", [x, y, junk], {2: "z"}, lambda: K.vsum(x, y)), n, f"vsum n={n}")
        case = _ew_case("VSUM_ZERO", [x, junk, junk], {1: "ycor", 2: "z"}, lambda: K.vsum_zero(x))
        run_case(case, n, f"vsum_zero n={n}")
        assert not np.signbit(K.vsum_zero(x)[0]["z"][::3]).any()
        run_case(_ew_case("SCALE_TO", [x, junk], {1: "z"}, lambda: K.scale_to(-1.7, x), dp=[-1.7]), n, f"scale_to n={n}")
        run_case(_ew_case("SCALE_TO", [x], {0: "z"}, lambda: K.scale_to(-1.7, x), dp=[-1.7]), n,
                 f"scale_to in place n={n}")
        run_case(_ew_case("COPY", [x, junk], {1: "z"}, lambda: (dict(z=x), [])), n, f"copy n={n}")
        run_case(_ew_case("ZERO", [x], {0: "z"}, lambda: (dict(z=np.zeros(n)), [])), n, f"zero n={n}")
        zn = np.full((2, n), -0.0)                          # predict: zn[0] = -0 + -0 = -0, y = -0 + 0 = +0
        run_case(_ew_case("PREDICT", [zn, junk, junk], {0: "zn", 1: "y"}, lambda: K.predict(zn, 1, True), ip=[1]), n,
                 f"predict -0.0 n={n}")
        assert np.signbit(K.predict(zn, 1, True)[0]["zn"][0]).all()
        assert not np.signbit(K.predict(zn, 1, True)[0]["y"]).any()


def test_residual_dq_work_atimes_variants():
    """residual with ycor null and non-null; dq_work and atimes read S_SIG from the ds the test sets"""
    for k, n in enumerate(K.SMALL_SIZES):
        f = Signed(n, seed=70 + k)
        run_case(c_residual(f, with_ycor=False), n, f"residual no ycor n={n}", seq=2, err=0x5)
        for sig2 in (0.37 * n, 4.0 * n, 1e-9):
            V, e, y = f.v(), f.w(), f.v()
            ds = {K.S_SIG: sig2}
            run_case(_ew_case("DQ_WORK", [V, e, y, np.zeros(n)], {3: "work"}, lambda: K.dq_work(V, e, y, ds), ds=ds), n,
                     f"dq_work sig2={sig2} n={n}")
            case = c_atimes(f)
            case["ds"][K.S_SIG] = sig2
            run_case(case, n, f"atimes sig2={sig2} n={n}", seq=9)


def test_mgs_shapes():
    """Vprev and Vnext each present or null, reading ds[hslot], into the slots the controller uses"""
    for k, n in enumerate(K.SMALL_SIZES):
        for (prev, nxt), slot0 in zip(itertools.product((False, True), repeat=2),
                                      (K.S_R0 + K.MAXL, K.S_WN, K.S_H0 + 1, K.S_H0 + K.MAXL)):
            run_case(c_mgs(Signed(n, seed=80 + k), prev, nxt, slot0), n, f"mgs prev={prev} next={nxt} n={n}",
                     seq=11, err=0x5 if nxt else None)


@pytest.mark.parametrize("krydim", [0, 1, 5, 8, 9, 32])
def test_newton_update_krydim(krydim):
    """krydim 0 (delta = dsrc or +0.0), the unrolled path up to kNuK = 8, the generic loop (9, 32); ycor_zero both
    ways"""
    for k, n in enumerate(K.SMALL_SIZES):
        for dsrc, ycz in itertools.product((False, True) if krydim == 0 else (False,), (False, True)):
            run_case(c_newton(Signed(n, seed=90 + k), krydim, dsrc, ycz), n,
                     f"newton_update krydim={krydim} dsrc={dsrc} ycor_zero={ycz} n={n}", seq=13, err=0x5)


def test_eta_norms_variants():
    for k, n in enumerate(K.SMALL_SIZES):
        for has_q, has_qmax, pq in ((True, True, True), (True, True, False), (False, True, False),
                                    (True, False, True), (True, False, False)):
            run_case(c_eta_norms(Signed(n, seed=110 + k), has_q, has_qmax, pq), n,
                     f"eta_norms q={has_q} qmax={has_qmax} pq={pq} n={n}", seq=17)


@pytest.mark.parametrize("pending", [None, (0, 3), (1, 5)])
def test_dky_variants(pending):
    """nvec 1, 2 (every row of N_VLinearSum's case table) and 3..6; rscale 0 and non-zero; no completion pending, or
    one on zn[j0..q] (pending = (j0, q))"""
    rng = np.random.default_rng(120)
    a, b = 0.375, -2.5
    pairs = [(1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (1.0, b), (a, 1.0), (-1.0, b), (a, -1.0), (a, a), (a, -a), (a, b)]
    l = [1.0, 1.0] + [0.29 / j for j in range(2, K.QMAX + 1)]
    for n in K.SMALL_SIZES:
        zn, acor = _slab(rng, n), _slab(rng, n, 1)[0]
        combos = [(1, [3], [1.75])] + [(2, [4, 1], list(p)) for p in pairs]
        combos += [(nv, list(range(nv - 1, -1, -1)), [1.0 + 0.3 * k for k in range(nv)]) for nv in (3, 4, 5, 6)]
        for nvec, js, c in combos:
            pend = None if pending is None else dict(acor=acor, l=l, j0=pending[0], q=pending[1])
            for rscale in (0.0, 1.0 / 0.013):
                ip = [nvec, pend["j0"] if pend else 0, pend["q"] if pend else 0] + js
                run_case(_ew_case("DKY", [zn, np.zeros(n), acor if pend else None], {1: "out"},
                                  lambda: K.dky(zn, js, c, nvec, rscale, pend), ip=ip, dp=[rscale], c0=c,
                                  c1=l if pend else None), n,
                         f"dky nvec={nvec} c={c} rscale={rscale} pending={pending} n={n}")


def test_bad_arguments_are_refused():
    """out-of-range arguments return -1 without launching"""
    n = 65
    z, zn = np.zeros(n), np.zeros((K.QMAX + 1, n))
    bad = [("EWT", 0, [z, z], {}),
           ("PREDICT", n, [zn, None, z], dict(ip=[0])),
           ("PREDICT", n, [zn, None, z], dict(ip=[K.QMAX + 1])),
           ("PREDICT", n, [zn[:3], None, z], dict(ip=[3])),
           ("PREDICT_PEND", n, [zn, None, z], dict(ip=[2, 0, 0, K.QMAX + 1, 0])),
           ("RESTORE", n, [zn[:2]], dict(ip=[2])),
           ("AXPY_MULTI", n, [zn], dict(ip=[K.QMAX + 1, 2, 3])),
           ("AXPY_MULTI", n, [zn], dict(ip=[5, 0, 3])),
           ("MGS", n, [z, None, None], dict(ip=[K.S_COUNT, K.S_WN])),
           ("MGS", n, [z, None, None], dict(ip=[K.S_H0, K.S_COUNT])),
           ("NEWTON", n, [np.zeros((K.MAXL + 1, n)), None, z, z], dict(ip=[K.MAXL + 1, 0])),
           ("NEWTON", n, [zn[:2], None, z, z], dict(ip=[3, 0])),
           ("COMPLETE", n, [zn, z], dict(ip=[0, K.QMAX + 1, -1])),
           ("COMPLETE_EWT", n, [zn, z, z], dict(ip=[2, K.QMAX + 1, 0])),
           ("ETA_NORMS", n, [z, z, None, z], dict(ip=[0])),
           ("DKY", n, [zn, z, None], dict(ip=[K.QMAX + 2, 0, 0, 0])),
           ("DKY", n, [zn, z, None], dict(ip=[2, 0, 0, 1, K.QMAX + 1]))]
    for op, nn, vecs, kw in bad:
        rc, _, ds, hds = run(op, nn, vecs, **kw)
        assert rc == -1, (op, kw)
        assert_same(hds, SENT, op)
    assert _lib().shud_kat_ode_grid_blocks(N_MIN) == K.grid_blocks(N_MIN) == 5122
