"""CPU: the restatement of the SHUD_WB_DIAG_QUAD monitor (tests/wb_quad_py.py) against hand-spelled values, and the
new C-ABI symbols of include/shud_wb.h.  No GPU."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

import cases
import wb_py
import wb_quad_py as qp
from conftest import ROOT
from shud_rhs import abi, shudio

LIB = os.path.join(ROOT, "shud-up_amd", "libshud_rhs.so")
R1 = np.array([4.0, 1.0, 0.5, 0.25, 2.0, 0.0, -8.0])            # dyadic rates: every product below is exact
R2 = np.array([2.0, 3.0, 1.5, 0.75, -1.0, 0.0, 16.0])
R3 = np.array([0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5])


def _basin(interval=60, trapz=False, prefix=None, **header):
    m, y = cases.single_element()
    st = wb_py.host_summary(m, y) + (np.zeros(1), np.zeros(1))
    return wb_py.WaterBalancePy(m, interval, st, trapz=trapz, prefix=prefix, **header), st


def test_quad_abi_exported_and_bound():
    new = {"shud_wb_quad_enable", "shud_wb_quad_step", "shud_wb_read_quad", "shud_wb_time_quad"}
    assert new <= set(abi.WB_FUNCTIONS)
    lib = C.CDLL(LIB)
    for n in new:
        assert hasattr(lib, n), n
    abi.bind(lib)
    assert lib.shud_wb_quad_step.argtypes == [C.c_void_p, C.c_double]
    # a null handle is an argument error, not a crash
    assert lib.shud_wb_quad_enable(None) == lib.shud_wb_quad_step(None, 0.0) == abi.SHUD_ERR_ARG


def test_first_step_is_euler_from_start_time():
    b, _ = _basin()
    q = qp.QuadMonitorPy(b, start_time=10.0)
    q.step(10.5, R1)
    assert q.acc.tolist() == (R1 * 0.5).tolist() == [2.0, 0.5, 0.25, 0.125, 1.0, 0.0, -4.0]
    assert q.prev.tolist() == R1.tolist() and q.has_prev and q.last_t == 10.5 and q.steps == 1


def test_later_steps_are_the_trapezoid():
    b, _ = _basin()
    q = qp.QuadMonitorPy(b)
    q.step(0.25, R1)                                            # R1 * 0.25
    q.step(1.0, R2)                                             # + 0.5 (R1 + R2) 0.75
    q.step(3.0, R3)                                             # + 0.5 (R2 + R3) 2
    want = R1 * 0.25 + 0.5 * (R1 + R2) * 0.75 + 0.5 * (R2 + R3) * 2.0
    assert q.acc.tolist() == want.tolist()
    assert q.acc[0] == 1.0 + 2.25 + 2.5 and q.acc[6] == -2.0 + 3.0 + 16.5
    assert q.prev.tolist() == R3.tolist() and q.steps == 3


def test_repeated_t_leaves_the_state_alone():
    b, _ = _basin()
    q = qp.QuadMonitorPy(b, start_time=5.0)
    q.step(5.0, R1)                                             # dt = 0 before any rate: has_prev stays 0
    assert not q.has_prev and not q.acc.any() and not q.prev.any() and q.steps == 0
    q.step(6.0, R1)
    acc, prev = q.acc.copy(), q.prev.copy()
    q.step(6.0, R2)                                             # repeated t
    q.step(5.5, R2)                                             # t going back: only quad_last_t moves
    assert np.array_equal(q.acc, acc) and np.array_equal(q.prev, prev) and q.has_prev and q.last_t == 5.5
    q.step(6.5, R2)                                             # dt from the recorded t; the trapezoid with R1
    assert q.acc.tolist() == (acc + 0.5 * (R1 + R2) * 1.0).tolist()


@pytest.mark.parametrize("trapz", [False, True])
def test_trapz_switch_has_no_influence(trapz):
    b, _ = _basin(trapz=trapz)
    q = qp.QuadMonitorPy(b)
    for t, r in ((0.5, R1), (2.0, R2), (2.5, R3)):
        q.step(t, r)
    want = R1 * 0.5 + 0.5 * (R1 + R2) * 1.5 + 0.5 * (R2 + R3) * 0.5
    assert q.acc.tolist() == want.tolist()


def test_row_formula():
    acc = [8.0, 2.0, 1.0, 0.5, 4.0, 0.25, 100.0]               # P ET Qout Qedge Qbc Qss noncons
    row = qp.quad_row(3.0, acc)
    assert row.tolist() == [3.0] + acc + [3.0 - (8.0 + 4.0 + 0.25 - 2.0 - 1.0 - 0.5)]
    assert row[8] == -5.75                                      # noncons is reported, not budgeted


def test_write_zeroes_accumulators_keeps_previous_rates_and_shares_the_gate(tmp_path):
    hdr = dict(forc_start_time=20000101, radiation_input_mode=1, terrain_radiation=1, solar_lonlat_mode="FIXED",
               lon=-122.71, lat=39.195)
    b, st = _basin(interval=30, prefix=tmp_path / "r", **hdr)
    q = qp.QuadMonitorPy(b, prefix=tmp_path / "r", **hdr)
    wrote, rows = [], []
    plan = [(10.0, R1), (29.5, R2), (30.4, R3), (30.9, R1), (47.0, R2), (60.0, R3), (75.0, R1), (90.7, R2)]
    for t, r in plan:
        q.step(t, r)
        before = q.acc.copy()
        w = q.maybe_write(t, st)
        assert w == (wb_py.write_gate(t, 30, -1 if not rows else rows[-1][0]) is not None)
        wrote.append(w)
        if w:
            rows.append((int(np.floor(t)), before))
            assert not q.acc.any() and q.prev.tolist() == r.tolist() and q.has_prev and q.last_t == t
            assert q.row[1:8].tolist() == before.tolist() and q.row[0] == b.basin_row[0]
        else:
            assert np.array_equal(q.acc, before)
    assert wrote == [False, False, True, False, False, True, False, True] and q.rows == b.rows == 3
    # the interval after a write starts with the trapezoid over the kept previous rate
    e = 0.0 + 0.5 * (R3 + R1) * (30.9 - 30.4)
    e = e + 0.5 * (R1 + R2) * (47.0 - 30.9)
    e = e + 0.5 * (R2 + R3) * (60.0 - 47.0)
    assert rows[1][1].tolist() == e.tolist()
    b.close()
    q.close()
    dq = shudio.read_dat(str(tmp_path / "r") + qp.QUAD_EXT)
    db = shudio.read_dat(str(tmp_path / "r") + ".basinwbfull.dat")
    assert dq["t"].tolist() == db["t"].tolist() == [0.0, 30.0, 60.0]          # t_quantized = floor - interval
    assert np.array_equal(dq["data"][:, 0], db["data"][:, 0])
    raw = open(str(tmp_path / "r") + qp.QUAD_EXT, "rb").read()
    hb = wb_py.header_bytes("basinwbfull_quad (m3)", 9, **hdr)
    assert raw[:len(hb)] == hb and len(raw) == len(hb) + 3 * 80
    assert raw[:1024].split(b"\n")[1] == b"# Water-balance diagnostic: basinwbfull_quad (m3)"
    assert struct.unpack("<11d", raw[1024:1024 + 88]) == (20000101.0, 9.0) + tuple(float(k) for k in range(1, 10))
    assert raw[len(hb):len(hb) + 80] == struct.pack("<10d", 0.0, *qp.quad_row(db["data"][0, 0], rows[0][1]))


def test_rates_from_flux_arrays():
    """quad_terms on hand-made flux arrays: Qout is QrivDown at the outlets only, the edge split follows nabr, Qedge
    is empty under CloseBoundary"""
    m, _ = cases.variant(n=2000)
    NE, NR = m.num_ele, m.num_riv
    rng = np.random.default_rng(3)
    d = {k: rng.integers(-8, 9, NE).astype(np.float64) for k in ("q_es", "q_eu", "q_eg", "q_tu", "q_tg")}
    d["qele_surf"], d["qele_sub"] = (rng.integers(-8, 9, 3 * NE).astype(np.float64) for _ in range(2))
    d["qriv_down"] = rng.integers(1, 9, NR).astype(np.float64)
    ic, prcp = np.ones(NE), np.full(NE, 2.0)
    outs = wb_py.outlet_list(m)
    assert 0 < outs.size < NR and not m.close_boundary
    for order in ("device", "seq"):                              # integer terms: every order gives the exact sum
        r = qp.quad_rates(m, ic, d, prcp, order=order)
        nb = np.asarray(m.nabr).reshape(3, NE)
        qe = (d["qele_surf"] + d["qele_sub"]).reshape(3, NE)
        assert r[abi.SHUD_WB_QOUT] == d["qriv_down"][outs].sum()
        assert r[abi.SHUD_WB_QEDGE] == qe[nb < 0].sum() and r[abi.SHUD_WB_NONCONS] == qe[nb >= 0].sum()
        assert r[abi.SHUD_WB_QSS] == 0.0
        qbc = np.concatenate([wb_py.ele_qbc(m), wb_py.riv_qbc(m)])             # table values: not integers
        assert np.abs(qbc).sum() > 0 and abs(r[abi.SHUD_WB_QBC] - qbc.sum()) <= 1e-12 * np.abs(qbc).sum()
    m.close_boundary = 1
    assert qp.quad_rates(m, ic, d, prcp)[abi.SHUD_WB_QEDGE] == 0.0
