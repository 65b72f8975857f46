"""Leaf-equation known-answer tests on edge-case grids (tests/kat_grids.py).

CPU: the oracle's C leaf functions (oracle_kat) against an independent pure-Python restatement of the same
reference lines (Python `math` is glibc libm, like the reference build) — bit for bit.
GPU: the kernels' own device functions (shud_physics.h through libshud_kat.so) against oracle_kat — bit for
bit wherever only IEEE-exact operations are involved (+,-,*,/,sqrt), within the parity tolerance
(|d| <= 1e-12|ref| + 1e-15) where OCML pow/cbrt/cos meet glibc (MANNING: cbrt; SATK: pow; SMS: cos) — a 1-ulp
libm difference is amplified by cancellation in -1 + pow(..) and 1 - cos(..)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from conftest import ATOL, ORACLE_DIR, PKG_DIR, RTOL
from kat_grids import ET_KAT, KAT, grid

ZERO, EPSILON, EPS_SLOPE, PI, GRAV = 1e-10, 0.005, 0.05e-6, 3.1415926, 9.8
_LIBM = C.CDLL("libm.so.6")                 # glibc cbrt (Python 3.10's math has none; numpy's is not glibc)
_LIBM.cbrt.restype = C.c_double
_LIBM.cbrt.argtypes = [C.c_double]


def _oracle_lib():
    lib = C.CDLL(os.path.join(ORACLE_DIR, "liboracle.so"))
    lib.oracle_kat.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.oracle_kat.restype = C.c_int
    return lib


def oracle_kat(name, x):
    out = np.zeros(x.shape[0])
    if name in ET_KAT:                      # the ET leaves live in shud_oracle_et.c
        lib = _oracle_lib()
        lib.oracle_et_kat.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        assert lib.oracle_et_kat(ET_KAT[name], x.ctypes.data, x.shape[0], out.ctypes.data) == 0
        return out
    assert _oracle_lib().oracle_kat(KAT[name], x.ctypes.data, x.shape[0], out.ctypes.data) == 0
    return out


# ---- pure-Python restatement (reference file:line per function) ----
def rmin(a, b):
    return b if a > b else a


def rmax(a, b):
    return b if a < b else a


def py_manning(A, n, R, S):               # Equations.hpp:54-63, pow23 :36-39
    t = _LIBM.cbrt(R)
    p23 = t * t
    if S > 0:
        return math.sqrt(S) * A * p23 / n
    return -1.0 * math.sqrt(-S) * A * p23 / n


def py_effkh(ygw, aq, md, kmac, af, kmx):  # Equations.cpp:116-134
    if md <= ZERO or ygw < aq - md:
        return kmx
    if ygw > aq:
        return (kmac * md * af + kmx * (aq - md * af)) / aq
    return (kmac * (ygw - (aq - md)) * af + kmx * (aq - md + (ygw - (aq - md)) * (1 - af))) / ygw


def py_weir(zi, yi, zj, yj, zbank, cwr, width, thr):   # MD_RiverFlux.cpp:65-98
    hi, hj = yi + zi, yj + zj
    dh = hj - hi
    if dh > 0:
        y = hi - zbank
        if y > 0 and yj > thr:
            if hi > zbank:
                y = dh
            return cwr * math.sqrt(2. * GRAV * y) * width * y * 60.
        return 0.
    y = hi - zbank
    if y > 0 and yi > thr:
        if hj > zbank:
            y = -dh
        return -1. * cwr * math.sqrt(2. * GRAV * y) * width * y * 60.
    return 0.


def py_r2e(yr, zr, ye, ze, ke, kr, L, D):  # Flux_RiverElement.cpp:11-55
    if ke < ZERO or kr < ZERO:
        return 0.
    K = (ke * 1. + kr * 1.) / (1. + 1.)
    he, hr = ye + ze, yr + zr
    dh = hr - he
    if dh > ZERO:
        A = (yr + (he - zr)) * .5 * L if he > zr else yr * L
        return 0. if yr < EPSILON else A * K * (dh / D)
    if dh < -ZERO:
        if ye > ZERO:
            return (yr + (he - zr)) * .5 * L * K * (dh / D)
        return 0.
    return 0.


def py_satk(s, n):                          # Equations.cpp:136-141
    t = -1. + math.pow(1. - math.pow(s, n / (n - 1.)), (n - 1.) / n)
    return math.sqrt(s) * t * t


def py_sms(ths, thr, s):                    # is_sm_et.cpp:131-140
    fc = ths * 0.75
    b = (s * (ths - thr) - thr) / (fc - thr)
    b = rmin(rmax(0., b), 1.)
    return 0.5 * (1 - math.cos(PI * b))


def py_dady(dA, w, s):                      # functions.hpp:125-153
    if dA == 0.:
        return 0.
    if abs(s) < EPS_SLOPE:
        with np.errstate(divide="ignore", invalid="ignore"):   # w = 0 is a KAT case: IEEE inf/NaN as in C
            return dA / w
    s = abs(s)
    cc = w * w + 4 * s * dA
    return -1. * w / (2. * s) if cc < ZERO else (-w + math.sqrt(cc)) / (2 * s)


def _fix(x):
    return 0. if x < 0. else x


def py_geom(kind):                          # River.hpp:115-127, River.cpp:49-62
    def f(w0, s, L, y):
        if kind == "AREA":
            return _fix(y * (w0 + y * s))
        if kind == "PEREM":
            return _fix(2.0 * math.sqrt(y * y + (y * s) * (y * s)) + w0)
        if kind == "TOPW":
            return _fix(y * s * 2.0 + w0)
        return _fix(0.5 * ((y * s * 2.0 + w0) + w0) * L)
    return f


PY = dict(MANNING=py_manning, EFFKH=py_effkh, WEIR=py_weir, R2E=py_r2e, SATK=py_satk, SMS=py_sms, DADY=py_dady,
          AREA=py_geom("AREA"), PEREM=py_geom("PEREM"), TOPW=py_geom("TOPW"), TOPAREA=py_geom("TOPAREA"))
TRANSCENDENTAL = {"MANNING", "SATK", "SMS"}


def _same(a, b):
    return (a == b) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("name", list(KAT))
def test_oracle_leaf_kat_vs_python(name):
    x = grid(name)
    got = oracle_kat(name, x)
    want = np.array([PY[name](*row) for row in x])
    bad = ~_same(got, want) | (np.signbit(got) != np.signbit(want))
    assert not bad.any(), f"{name}: {bad.sum()} of {x.shape[0]} differ, first row {x[np.argmax(bad)]}"


_REF_KAT = {}


def _ref_kat_all():
    """the reference's own leaf functions over every grid: live (libshud_ref_kat.so in a child process, which
    must then equal the committed recording) where the library was built, the recording alone otherwise"""
    if not _REF_KAT:
        import sys
        sys.path.insert(0, os.path.join(ORACLE_DIR, "ref"))
        import refio
        rec = refio.load_recording("kat")
        _REF_KAT["rec"] = rec
        _REF_KAT["live"] = None
        if refio.live_status("leaf equations (ref_kat)"):
            ids = {**KAT, **ET_KAT}
            _REF_KAT["live"] = refio.ref_kat_child({n: (ids[n], grid(n)) for n in ids})
    return _REF_KAT


@pytest.mark.parametrize("name", list(KAT) + list(ET_KAT))
def test_oracle_leaf_kat_vs_reference(name):
    """oracle_kat against the reference model's own functions (ref_kat), bit for bit, NaN patterns and the sign
    of zero included.  The ET leaves PET_PM_openwater, PET_Penman_Monteith and AerodynamicResistance have no
    other known-answer test."""
    r = _ref_kat_all()
    x = grid(name)
    got = oracle_kat(name, x)
    want = r["rec"][name]
    if r["live"] is not None:
        live = r["live"][name]
        assert live.shape == want.shape and np.array_equal(live.view(np.uint64), want.view(np.uint64)), \
            f"{name}: the committed recording is stale (oracle/ref/record.py)"
    assert want.shape == got.shape
    bad = ~_same(got, want) | (~np.isnan(want) & (np.signbit(got) != np.signbit(want)))
    assert not bad.any(), f"{name}: {bad.sum()} of {x.shape[0]} differ, first row {x[np.argmax(bad)]}"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(KAT))
def test_device_leaf_kat_vs_oracle(name):
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    lib.shud_kat_eval.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.shud_kat_eval.restype = C.c_int
    x = grid(name)
    got = np.zeros(x.shape[0])
    assert lib.shud_kat_eval(KAT[name], x.ctypes.data, x.shape[0], got.ctypes.data) == 0
    want = oracle_kat(name, x)
    if name in TRANSCENDENTAL:     # OCML vs glibc ulps, amplified by the formulas' own cancellation
        ok = _same(got, want) | (np.abs(got - want) <= RTOL * np.abs(want) + ATOL)
    else:
        ok = _same(got, want) & (np.signbit(got) == np.signbit(want))
    assert ok.all(), f"{name}: {(~ok).sum()} of {x.shape[0]} differ, first row {x[np.argmax(~ok)]}"


@pytest.mark.gpu
def test_cos_small_bit_identical():
    """cos_small (shud_physics.h: OCML's small-argument cos path without the Payne-Hanek branch and the |x| /
    finiteness selects) returns the same bits as the device's full cos on SoilMoistureStress's arguments
    K_PI * b, b in [0, 1] (is_sm_et.cpp:131-140), and on a wider grid below 2^30."""
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    lib.shud_kat_cos.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    rng = np.random.default_rng(11)
    n = 1 << 20
    b = np.concatenate([rng.uniform(0.0, 1.0, n // 2), 10 ** rng.uniform(-17, 0, n // 4)])
    x = np.concatenate([3.1415926 * b, rng.uniform(0.0, 2.0 ** 30, n // 8), 10 ** rng.uniform(-300, 9, n // 8),
                        np.array([0.0, 3.1415926, np.pi / 2, np.pi / 4, np.pi, 3 * np.pi / 4, 1.0, 5e-324,
                                  np.nextafter(2.0 ** 30, 0.0)])])
    x = np.ascontiguousarray(x)
    full, fast = np.zeros(x.size), np.zeros(x.size)
    assert lib.shud_kat_cos(0, x.ctypes.data, x.size, full.ctypes.data) == 0
    assert lib.shud_kat_cos(1, x.ctypes.data, x.size, fast.ctypes.data) == 0
    same = full.view(np.uint64) == fast.view(np.uint64)
    assert same.all(), f"{(~same).sum()} differ, first x = {x[np.argmax(~same)]!r}"


def _cdiv_operands():
    """(a, b) pairs for cdiv: divisors in the handle's admitted range [2^-20, 2^20] plus 0 / inf / NaN (the
    class constants a model may carry), numerators across the whole double range with the guard boundaries
    2^-948 / 2^1000, subnormals, DBL_MAX, signed zeros, infinities and NaN."""
    rng = np.random.default_rng(2024)
    n = 1 << 18
    b = np.concatenate([np.exp2(rng.uniform(-20, 20, n)) * rng.choice([-1.0, 1.0], n),
                        rng.uniform(1e-3, 1e4, n),
                        np.array([2.0 ** -20, 2.0 ** 20, 1.0, 3.0, 0.1, 0.3, 0.0, -0.0, np.inf, -np.inf, np.nan])])
    m = b.size
    e = rng.uniform(-1074, 1024, m)
    a = np.exp2(np.clip(e, -1074, 1023.999)) * rng.choice([-1.0, 1.0], m)
    # boundary bands: just below/above the guard thresholds and at the subnormal / overflow edges
    band = rng.integers(0, 6, m)
    a = np.where(band == 0, np.exp2(rng.uniform(-952, -944, m)), a)
    a = np.where(band == 1, np.exp2(rng.uniform(996, 1004, m)) * rng.uniform(1, 1.999, m), a)
    a = np.where(band == 2, rng.integers(1, 1 << 52, m).astype(np.uint64).view(np.float64), a)   # subnormals
    a = np.where(band == 3, np.finfo(np.float64).max * rng.uniform(0.5, 1.0, m), a)
    specials = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.0 ** -948, 2.0 ** 1000,
                         np.nextafter(2.0 ** -948, 0), np.nextafter(2.0 ** 1000, np.inf), np.finfo(np.float64).max])
    sa, sb = np.meshgrid(specials, b[-11:])
    a = np.concatenate([a, sa.ravel()])
    b = np.concatenate([b, sb.ravel()])
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def _bits_same(got, want):
    return (got.view(np.uint64) == want.view(np.uint64)) | (np.isnan(got) & np.isnan(want))


def test_cdiv_algorithm_bit_identical(tmp_path):
    """The reciprocal division cdiv (shud_physics.h: q0 = a*RN(1/b), one fma residual, one fma correction;
    IEEE division on the cold path for 0 < |a| < 2^-948 or |a| > 2^1000) restated in C with glibc's correctly
    rounded fma equals IEEE a / b bit for bit on the admitted divisors — subnormal quotients and overflow
    included — while the unguarded form does not (Markstein needs no under/overflow)."""
    import subprocess
    so = str(tmp_path / "libcdiv.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC", "-o", so,
                           os.path.join(os.path.dirname(__file__), "cdiv_emul.c"), "-lm"])
    lib = C.CDLL(so)
    lib.cdiv_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    a, b = _cdiv_operands()
    with np.errstate(all="ignore"):
        want = a / b
    got, raw = np.zeros_like(a), np.zeros_like(a)
    lib.cdiv_eval(a.ctypes.data, b.ctypes.data, a.size, 1, got.ctypes.data)
    lib.cdiv_eval(a.ctypes.data, b.ctypes.data, a.size, 0, raw.ctypes.data)
    ok = _bits_same(got, want)
    assert ok.all(), f"{(~ok).sum()} differ, first (a, b) = {a[np.argmax(~ok)]!r}, {b[np.argmax(~ok)]!r}"
    assert not _bits_same(raw, want).all()          # the guard is needed: the raw form misses subnormal cases


@pytest.mark.gpu
def test_cdiv_bit_identical():
    """The device cdiv with the host's reciprocal equals IEEE a / b bit for bit on the same operands."""
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    lib.shud_kat_cdiv.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    a, b = _cdiv_operands()
    with np.errstate(all="ignore"):
        want = a / b
    got = np.zeros_like(a)
    assert lib.shud_kat_cdiv(a.ctypes.data, b.ctypes.data, a.size, got.ctypes.data) == 0
    ok = _bits_same(got, want)
    assert ok.all(), f"{(~ok).sum()} differ, first (a, b) = {a[np.argmax(~ok)]!r}, {b[np.argmax(~ok)]!r}"


def _fast_operands(n=1 << 21, seed=23):
    """the fast paths' domains and edges: random bit patterns (every class and exponent), magnitudes 10^-320..10^308,
    Manning slopes and weir depths, values straddling the guard bounds 2^-767 (sqrt), 2^-900 / 2^600 (numerator),
    2^-100 / 2^100 (divisor), signed zeros, infinities, NaN"""
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 2 ** 63, n // 4, dtype=np.uint64).view(np.float64) * rng.choice([-1.0, 1.0], n // 4)
    mag = 10 ** rng.uniform(-320, 308, n // 4) * rng.choice([-1.0, 1.0], n // 4)
    phys = rng.uniform(-2.0, 2.0, n // 4) * 10 ** rng.uniform(-12, 3, n // 4)
    edges = []
    for e in (-767, -900, 600, -100, 100, -1022, 1023, 0):
        edges.append(np.ldexp(1.0, e) * np.array([1.0, 1.0 - 2 ** -53, 1.0 + 2 ** -52, -1.0]))
    edges.append(np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308,
                           1.7976931348623157e308]))
    rest = 10 ** rng.uniform(-5, 5, n // 4)
    a = np.concatenate([raw, mag, phys, rest] + edges)
    b = np.concatenate([rng.permutation(a[: a.size - sum(e.size for e in edges)])] +
                       [10 ** rng.uniform(-40, 40, sum(e.size for e in edges))])
    b = np.where(rng.random(b.size) < 0.5, b, np.ldexp(rng.uniform(0.5, 1.0, b.size),
                                                        rng.integers(-110, 110, b.size)) * rng.choice([-1.0, 1.0], b.size))
    return a, b


@pytest.mark.gpu
def test_fast_sqrt_div_bit_identical():
    """shud_physics.h sqrt_nr (LLVM's f64 sqrt chain without its tiny-argument scaling and zero/inf select, those on a
    cold path) and div_nr / recip_nr (the f64 division chain without v_div_scale / v_div_fixup, the reciprocal shared
    by divisions with one divisor) return the same bits as the device's own sqrt and a / b on every operand class."""
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    lib.shud_kat_fast.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    a, b = _fast_operands()
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    out = [np.zeros_like(a) for _ in range(4)]
    for k in range(4):
        assert lib.shud_kat_fast(k, a.ctypes.data, b.ctypes.data, a.size, out[k].ctypes.data) == 0
    for fast, ref, name in ((0, 1, "sqrt_nr"), (2, 3, "div_nr")):
        ok = _bits_same(out[fast], out[ref])
        assert ok.all(), f"{name}: {(~ok).sum()} differ, first (a, b) = {a[np.argmax(~ok)]!r}, {b[np.argmax(~ok)]!r}"
    with np.errstate(all="ignore"):                 # and both are the IEEE results (correctly rounded)
        assert _bits_same(out[1], np.sqrt(a)).all()
        assert _bits_same(out[3], a / b).all()


@pytest.mark.gpu
def test_cbrt_glibc_bit_identical():
    """shud_physics.h cbrt_glibc (glibc 2.35's s_cbrt.c restated for the device; pow23 / Manning's R^(2/3),
    Equations.hpp:36-39) equals this host's glibc cbrt (libm.so.6 via ctypes) bit for bit: Manning's domain (hydraulic radius and
    surface depth 1e-12 .. 1e3), every exponent (incl. subnormals), signed zeros, infinities and NaN."""
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    lib.shud_kat_fast.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    rng = np.random.default_rng(29)
    n = 1 << 19
    a = np.concatenate([10 ** rng.uniform(-12, 3, n // 2), rng.uniform(0.0, 0.5, n // 4),
                        10 ** rng.uniform(-323, 308, n // 4) * rng.choice([-1.0, 1.0], n // 4),
                        np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, 1.0, 8.0, -27.0, 0.5, 2.0 ** -1074])])
    a = np.ascontiguousarray(a)
    got = np.zeros_like(a)
    assert lib.shud_kat_fast(4, a.ctypes.data, a.ctypes.data, a.size, got.ctypes.data) == 0
    libm = C.CDLL("libm.so.6")                    # glibc's own cbrt (numpy.cbrt is numpy's implementation, not libm's)
    libm.cbrt.restype, libm.cbrt.argtypes = C.c_double, [C.c_double]
    want = np.array([libm.cbrt(float(x)) for x in a])
    ok = _bits_same(got, want)
    assert ok.all(), f"{(~ok).sum()} differ, first x = {a[np.argmax(~ok)]!r}"


# ---- pow_tab (shud_powtab.h): satKfun's pow ----------------------------------------------------------------------
def _pow_tab_operands(n=1 << 20, seed=11):
    """satKfun's domain (Equations.cpp:136-141): bases satn in (ZERO, 0.99] and 1 - satn^ex1 in (0, 1], exponents
    ex1 = n/(n-1) and ex2 = (n-1)/n of Beta = n > 1 (close to 1 too, where ex1 is huge and satn^ex1 underflows), plus
    bases close to 1, subnormal results and the edges"""
    rng = np.random.default_rng(seed)
    beta = np.concatenate([1.0 + rng.uniform(1e-6, 4.0, n // 2), 1.0 + 10 ** rng.uniform(-12, 3, n // 2)])
    x = np.concatenate([rng.uniform(1e-10, 0.99, n // 4), 10 ** rng.uniform(-10, 0, n // 4),
                        1.0 - 10 ** rng.uniform(-17, -0.01, n // 4), 10 ** rng.uniform(-300, 0, n // 4)])
    y = np.where(rng.random(n) < 0.5, beta / (beta - 1.0), (beta - 1.0) / beta)
    edge_x = np.array([1.0, 0.99, 1e-10, 0.5, np.nextafter(1.0, 0.0), 5e-324, 2.2250738585072014e-308, 1e-10, 0.9])
    edge_y = np.array([3.0, 1.0, 0.5, 2.0, 1e6, 1.0, 1.0, 70.0, 7000.0])
    return np.concatenate([x, edge_x]), np.concatenate([y, edge_y])


def _pow_tab_lib(tmp_path, compact=None):
    """the C build of shud_powtab.h (compact: force SHUD_PT_COMPACT; None: the header's default, as the kernels)"""
    import subprocess
    so = str(tmp_path / f"libpowtab{'' if compact is None else compact}.so")
    flags = [] if compact is None else [f"-DSHUD_PT_COMPACT={compact}"]
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-shared", "-fPIC"] + flags + ["-I",
                           os.path.join(PKG_DIR, "csrc"), "-o", so,
                           os.path.join(os.path.dirname(__file__), "pow_tab_emul.c"), "-lm"])
    lib = C.CDLL(so)
    for f in (lib.pow_tab_eval, lib.pow_glibc_eval):
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    return lib


@pytest.mark.parametrize("compact", [0, 1])
def test_pow_tab_accuracy(tmp_path, compact):
    """pow_tab restated in C from the same header the kernels compile (glibc's correctly rounded fma): within 1 ulp
    of glibc's pow (the reference's libm) everywhere on satKfun's domain, bit-identical to it on >= 99.5 % of the
    operands, and within 0.7 ulp of the exact x^y (decimal, 50 digits) wherever the two differ (sampled) — glibc's
    pow is itself within ~0.51 ulp there."""
    from decimal import Decimal, getcontext
    lib = _pow_tab_lib(tmp_path, compact)
    x, y = _pow_tab_operands()
    got, ref = np.zeros_like(x), np.zeros_like(x)
    lib.pow_tab_eval(x.ctypes.data, y.ctypes.data, x.size, got.ctypes.data)
    lib.pow_glibc_eval(x.ctypes.data, y.ctypes.data, x.size, ref.ctypes.data)
    d = np.abs(got.view(np.int64) - ref.view(np.int64))
    assert d.max() <= 1, f"max {d.max()} ulp at (x, y) = {x[np.argmax(d)]!r}, {y[np.argmax(d)]!r}"
    assert (d == 0).mean() >= 0.995, (d == 0).mean()
    getcontext().prec = 50
    worst = 0.0
    for k in np.nonzero(d)[0][:400]:
        t = (Decimal(y[k]) * Decimal(x[k]).ln()).exp()
        if t == 0 or float(t) < 2.2250738585072014e-308:
            continue
        worst = max(worst, float(abs(Decimal(got[k]) - t) / Decimal(math.ulp(float(t)))))
    assert worst <= 0.7, worst


@pytest.mark.gpu
def test_pow_tab_device_bit_identical(tmp_path):
    """The kernels' pow_tab (HIP build of shud_powtab.h) returns the bits of its C restatement on satKfun's domain."""
    clib = _pow_tab_lib(tmp_path)
    lib = C.CDLL(os.path.join(PKG_DIR, "libshud_kat.so"))
    lib.shud_kat_pow.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    x, y = _pow_tab_operands()
    want = np.zeros_like(x)
    clib.pow_tab_eval(x.ctypes.data, y.ctypes.data, x.size, want.ctypes.data)
    xy = np.ascontiguousarray(np.stack([x, y], 1))
    got = np.zeros_like(x)
    assert lib.shud_kat_pow(2, xy.ctypes.data, x.size, got.ctypes.data) == 0
    same = got.view(np.uint64) == want.view(np.uint64)
    assert same.all(), f"{(~same).sum()} differ, first (x, y) = {xy[np.argmax(~same)]}"
