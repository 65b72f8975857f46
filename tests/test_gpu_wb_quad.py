"""GPU: the SHUD_WB_DIAG_QUAD monitor on the device (shud_wb_quad_enable / shud_wb_quad_step / the quad row of
shud_wb_maybe_write, include/shud_wb.h) against its numpy restatement (tests/wb_quad_py.py) fed with the values read
back from the handle, on the rig of tests/test_gpu_wb.py.

The seven rates are reductions: each is held to the bound every summation order meets,
|gpu - fsum(terms)| <= (n - 1) 2^-53 sum|terms|, and equals the restatement run with the device's tree
(wb_py.device_sum) bit for bit.  Qout is the sum of QrivDown as f() left it: its terms are copies, no cbrt.  Given
the rates, the monitor step and the quad row are scalar IEEE operations in the reference's order (the library is
built with -ffp-contract=off): accumulators, previous rates, rows and the file are compared bit for bit."""
import os

import numpy as np
import pytest

import cases
import oracle
import shud_gpu_run
import test_gpu_wb as tw
import wb_py
import wb_quad_py as qp
from shud_rhs import abi, driver, host, shudio, synth, workload
from shud_rhs import runtime as rt
from shud_rhs.solver import ZERO

pytestmark = pytest.mark.gpu
QUAD_FILE = "syn" + qp.QUAD_EXT


def _closed(m):
    m.close_boundary = 1
    return m.finalize()


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 1023, 1024, 1025, 2000, 1_060_000])
def test_rates_reduction_edges(ne):
    """Sizes around the wave (64) and the 1024-lane workgroup, NE = 2000 (+-BC elements and reaches, outlets) and
    1,060,000: just above 1024 workgroups, where the finalize's threads take more than one partial.  The cases
    below 2000 are river-less subsets (no outlet: Qout is 0.0); every case has an open boundary."""
    m, y = tw._bound_case(ne)
    NE = m.num_ele
    assert m.close_boundary == 0
    if ne < 2000:
        assert NE == ne
    elif ne == 2000:                                           # two 1024-lane workgroups, the second one partly idle
        assert 1024 < NE <= 2048, NE
    else:
        assert (1 << 20) < NE < 1.1 * (1 << 20), NE
    rig = tw.Rig(m)
    rig.advance(0.0, y)
    wb = rt.WaterBalance(rig.h, 60)
    wb.quad_enable()
    rig.advance(12.5, workload.random_state(m, seed=9))
    wb.on_et_update()
    wb.quad_step(12.5)
    d = rig.h.diagnostics()
    ic = d["e_ic"]                                             # on_et_update after f(): the carried value
    q = wb.read_quad()
    rate = q["rate"]
    assert np.array_equal(q["acc"], rate * 12.5) and q["last_t"] == 12.5
    nb = np.asarray(m.nabr).reshape(3, NE)
    qe = d["qele_surf"].reshape(3, NE) + d["qele_sub"].reshape(3, NE)
    outs = wb_py.outlet_list(m)
    big = ne >= 2000
    tw._check_bound("P", rate[abi.SHUD_WB_P], m.step["prcp"] * m.ele["area"], must_be_live=True)
    tw._check_order("P", rate[abi.SHUD_WB_P], m.step["prcp"] * m.ele["area"])
    tw._check_bound("ET", rate[abi.SHUD_WB_ET],
                    (ic + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * m.ele["area"], must_be_live=True)
    tw._check_order("ET", rate[abi.SHUD_WB_ET],
                    (ic + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * m.ele["area"])
    tw._check_bound("Qout", rate[abi.SHUD_WB_QOUT], d["qriv_down"][outs], must_be_live=big)
    tw._check_bound("Qedge", rate[abi.SHUD_WB_QEDGE], qe[nb < 0], must_be_live=True)
    tw._check_bound("Qbc", rate[abi.SHUD_WB_QBC], np.concatenate([wb_py.ele_qbc(m)[np.asarray(m.ibc) < 0],
                                                                 wb_py.riv_qbc(m)[np.asarray(m.riv_bc) < 0]]),
                    must_be_live=big)
    tw._check_bound("Qss", rate[abi.SHUD_WB_QSS], np.zeros(int((np.asarray(m.iss) != 0).sum())))
    tw._check_bound("noncons", rate[abi.SHUD_WB_NONCONS], qe[nb >= 0], must_be_live=big)
    terms = qp.quad_terms(m, ic, d, m.step["prcp"])
    assert rate[abi.SHUD_WB_QOUT] == wb_py.device_sum(terms["Qout"])          # copies of QrivDown: bit for bit
    assert (outs.size > 0) == big and (big or rate[abi.SHUD_WB_QOUT] == 0.0)
    assert np.array_equal(rate, qp.quad_rates(m, ic, d, m.step["prcp"]))      # the device's tree, restated
    g = wb.read(arrays=False)                                  # the sample's scalars were not touched
    assert not g["basin_acc"].any() and not g["basin_rate"].any() and g["last_t"] == 0.0
    wb.close()
    rig.close()


PLAN = [(7.5, None), (20.0, "step"), (20.0, None), (45.25, "carried"), (60.0, None), (61.5, "step"), (95.0, None),
        (120.0, "carried")]


def _monitor_run(trapz, closed=False):
    """the monitor over PLAN on variant(n=2000): seven integrating steps with unequal dt, one repeated t, interval
    ends (sample + maybe_write) at 60 and 120 in the middle.  After every step the device's accumulators and
    previous rates must equal the restatement fed with the device's own rates.  -> the device bits per step"""
    m, y0 = cases.variant(n=2000)
    if closed:
        m = _closed(m)
    rig = tw.Rig(m)
    rig.advance(0.0, y0)
    wb = rt.WaterBalance(rig.h, 60, start_time=0.0, trapz=trapz)
    wb.quad_enable()
    ref = qp.QuadMonitorPy(None, start_time=0.0)
    wb.on_et_update()
    rng = np.random.default_rng(21)
    bits, rows = [], 0
    for k, (t, et) in enumerate(PLAN):
        if et == "step":
            rig.new_step(seed=300 + k)
            wb.on_et_update()
        rig.advance(t, y0 if k == 0 else workload.random_state(m, seed=500 + k))
        if et == "carried":
            wb.on_et_update()
        before = wb.read_quad()
        wb.quad_step(t)
        q = wb.read_quad()
        if k == 2:                                             # the repeated t: nothing but quad_last_t moves
            assert np.array_equal(q["acc"], before["acc"]) and np.array_equal(q["rate"], before["rate"])
        else:
            assert np.abs(q["rate"]).sum() > 0
        ref.step(t, q["rate"])
        assert np.array_equal(q["acc"], ref.acc) and np.array_equal(q["rate"], ref.prev), (k, t)
        assert q["last_t"] == ref.last_t == t
        if closed:
            assert q["rate"][abi.SHUD_WB_QEDGE] == 0.0 and q["acc"][abi.SHUD_WB_QEDGE] == 0.0
        elif k != 2:
            assert q["rate"][abi.SHUD_WB_QEDGE] != 0.0
        rig.h.h2d(rig.d_du, rng.normal(0.0, 1e-4, m.num_y))
        wb.sample(t, rig.d_du)
        wrote = wb.maybe_write(t)
        assert wrote == (t in (60.0, 120.0))
        if wrote:
            rows += 1
            ref.write(t - 60.0, wb.read(arrays=False)["basin_row"][0])
            q = wb.read_quad()
            assert np.array_equal(q["row"], ref.row) and not q["acc"].any()
            assert np.array_equal(q["rate"], ref.prev)         # the previous rates are kept
        bits.append((q["acc"].copy(), q["rate"].copy(), q["row"].copy()))
    assert rows == 2 and ref.steps == 7
    wb.close()
    rig.close()
    return bits


def test_monitor_arithmetic_bit_for_bit():
    """open boundary, +-BC elements and reaches, SS flags, every outlet code; once with the diagnostic's trapz off
    and once on: the same quad bits.  On a closed-boundary copy Qedge is 0.0."""
    a, b = _monitor_run(False), _monitor_run(True)
    for k, (x, y) in enumerate(zip(a, b)):
        for u, v in zip(x, y):
            assert np.array_equal(u, v), k
    _monitor_run(False, closed=True)


def _hand_run(tmp_path, name, quad, trapz=False, ref=False):
    """the hand-driven run of test_gpu_wb.test_files_byte_identical, with the monitor interleaved when quad.
    -> (the device's last read, quad reads after each maybe_write)"""
    m, _ = cases.variant(n=2000)
    m = tw._critical_outlets(m)
    hdr = dict(forc_start_time=20000101, radiation_input_mode=1, terrain_radiation=1, solar_lonlat_mode="FIXED",
               lon=-122.71, lat=39.195)
    rig = tw.Rig(m, storages=True)
    rig.advance(0.0, workload.random_state(m, seed=40))
    wb = rt.WaterBalance(rig.h, 30, trapz=trapz, prefix=tmp_path / name, **hdr)
    if quad:
        wb.quad_enable()
    basin = qref = None
    if ref:
        basin = wb_py.WaterBalancePy(m, 30, rig.state(), trapz=trapz, prefix=tmp_path / "ref", **hdr)
        qref = qp.QuadMonitorPy(basin, prefix=tmp_path / "ref", **hdr)
        basin.on_et_update(rig.h.diagnostics()["e_ic"])
    wb.on_et_update()
    ic = rig.h.diagnostics()["e_ic"]
    rng = np.random.default_rng(8)
    wrote, reads = [], []
    for k, t in enumerate([10.0, 30.4, 30.9, 47.0, 60.0, 75.5, 90.0]):
        rig.advance(t, workload.random_state(m, seed=41 + k))
        rig.set_storages(10 + k)
        dy = rng.normal(0.0, 1e-4, m.num_y)
        if quad:
            wb.quad_step(t)
        rig.h.h2d(rig.d_du, dy)
        wb.sample(t, rig.d_du)
        wrote.append(wb.maybe_write(t))
        if ref:
            d, st = rig.h.diagnostics(), rig.state()
            qref.step(t, qp.quad_rates(m, ic, d, m.step["prcp"]))
            basin.sample(t, dy, d, m.step["prcp"], m.step["net_prep"], st[3])
            assert qref.maybe_write(t, st) == wrote[-1], t
        if quad and wrote[-1]:
            reads.append(wb.read_quad())
            if ref:
                assert np.array_equal(reads[-1]["row"], qref.row)
    assert wrote == [False, True, False, False, True, False, True]
    g = wb.read()
    wb.close()
    if ref:
        basin.close()
        qref.close()
    rig.close()
    return g, reads


def test_quad_file_byte_identical(tmp_path):
    """basinwbfull_quad.dat (and the five other files) against the restatement run with the device's tree; rows at
    the basin file's times, column 0 the basin row's, the accumulators 0.0 after a write"""
    _, reads = _hand_run(tmp_path, "dev", quad=True, ref=True)
    for _, ext in wb_py.LABELS + [(qp.QUAD_LABEL, qp.QUAD_EXT)]:
        a, b = open(str(tmp_path / "dev") + ext, "rb").read(), open(str(tmp_path / "ref") + ext, "rb").read()
        assert a == b, (ext, len(a), len(b))
    dq = shudio.read_dat(str(tmp_path / "dev") + qp.QUAD_EXT)
    db = shudio.read_dat(str(tmp_path / "dev") + ".basinwbfull.dat")
    assert dq["header"].splitlines()[1] == "# Water-balance diagnostic: basinwbfull_quad (m3)"
    assert dq["t"].tolist() == db["t"].tolist() == [0.0, 30.0, 60.0] and dq["data"].shape == (3, 9)
    assert np.array_equal(dq["data"][:, 0], db["data"][:, 0]) and np.isfinite(dq["data"]).all()
    assert np.abs(dq["data"][:, 1:8]).sum() > 0 and not np.array_equal(dq["data"][:, 3], db["data"][:, 3])
    assert len(reads) == 3
    for k, r in enumerate(reads):
        assert not r["acc"].any() and np.array_equal(r["row"], dq["data"][k])


@pytest.mark.parametrize("trapz", [False, True])
def test_monitor_leaves_the_sample_alone(tmp_path, trapz):
    """the same sample / maybe_write calls with and without interleaved quad_step calls: the five files and every
    array and scalar of the diagnostic's read-back are identical"""
    ga, _ = _hand_run(tmp_path, "with", quad=True, trapz=trapz)
    gb, _ = _hand_run(tmp_path, "without", quad=False, trapz=trapz)
    for _, ext in wb_py.LABELS:
        a, b = open(str(tmp_path / "with") + ext, "rb").read(), open(str(tmp_path / "without") + ext, "rb").read()
        assert a == b and len(a) >= 1024 + 8 * 11 + 3 * 8 * 10, ext      # header + three rows, at the least
    assert os.path.exists(str(tmp_path / "with") + qp.QUAD_EXT)
    assert not os.path.exists(str(tmp_path / "without") + qp.QUAD_EXT)
    assert set(tw.ARR4) <= set(ga)
    for key in ga:
        assert np.array_equal(np.asarray(ga[key]), np.asarray(gb[key]), equal_nan=True), key


def test_interface_errors(tmp_path):
    m, y = cases.single_element()
    rig = tw.Rig(m)
    rig.h.h2d(rig.d_y, y)
    rig.h.eval_device(0.0, rig.d_y, rig.d_f)
    rig.h.summary(rig.d_y)                                     # an evaluation, but no refresh_diagnostics yet
    wb = rt.WaterBalance(rig.h, 30)
    with pytest.raises(rt.ShudRhsError) as e:                  # a monitor step without the monitor
        wb.quad_step(5.0)
    assert e.value.code == abi.SHUD_ERR_ARG
    wb.quad_enable()
    with pytest.raises(rt.ShudRhsError) as e:                  # twice
        wb.quad_enable()
    assert e.value.code == abi.SHUD_ERR_ARG
    with pytest.raises(rt.ShudRhsError) as e:                  # before refresh_diagnostics
        wb.quad_step(5.0)
    assert e.value.code == abi.SHUD_ERR_ARG and "refresh_diagnostics" in str(e.value)
    assert wb.read_quad()["last_t"] == 0.0 and not wb.read_quad()["acc"].any()
    rig.h.refresh_diagnostics()
    wb.quad_step(5.0)
    assert wb.read_quad()["last_t"] == 5.0 and wb.read_quad()["acc"][abi.SHUD_WB_P] > 0
    wb.close()
    wb = rt.WaterBalance(rig.h, 30)
    rig.h.h2d(rig.d_du, np.zeros(m.num_y))
    wb.sample(5.0, rig.d_du)
    with pytest.raises(rt.ShudRhsError) as e:                  # after a sample
        wb.quad_enable()
    assert e.value.code == abi.SHUD_ERR_ARG
    wb.close()
    # the quad file on /dev/full: the error comes out of maybe_write or, at the latest, close
    (tmp_path / "w.basinwbfull_quad.dat").symlink_to("/dev/full")
    wb = rt.WaterBalance(rig.h, 30, prefix=tmp_path / "w")
    wb.quad_enable()
    errs = []
    for call in (lambda: wb.maybe_write(30.0), wb.close):
        try:
            call()
        except rt.ShudRhsError as ex:
            errs.append(ex)
    assert errs and "basinwbfull_quad" in str(errs[0]) and errs[0].code == abi.SHUD_WB_ERR_IO
    (tmp_path / "nodir").mkdir()
    wb = rt.WaterBalance(rig.h, 30, prefix=tmp_path / "nodir" / "w")
    (tmp_path / "nodir" / "w.basinwbfull_quad.dat").mkdir()   # cannot be opened for writing
    with pytest.raises(rt.ShudRhsError) as e:
        wb.quad_enable()
    assert e.value.code == abi.SHUD_WB_ERR_IO
    wb.close()
    rig.close()


@pytest.mark.parametrize("kind", ["omp", "lake", "partitioned"])
def test_refused_handles_stay_refused(kind):
    """quad lives on a shud_wb handle: the kinds shud_wb_create refuses have none to enable it on"""
    tw.test_refusals(kind)


@pytest.mark.parametrize("case", ["plain", "bc_substep"])
def test_drivers_byte_identical_with_quad(tmp_path, case):
    """shud_gpu under SHUD_WB_DIAG=1 SHUD_WB_DIAG_QUAD=1 against ShudSolver.run(wb=, quad=True) over the first six
    hours of the synthetic project of test_gpu_wb.test_drivers_byte_identical: the 24 ordinary and the six
    diagnostic files byte-identical; as many monitor steps as internal steps of the integrator."""
    src = tmp_path / "in"
    if case == "bc_substep":
        synth.write_project(str(src), "syn", 2000, days=1.0, max_step=30.0, et_step=10.0, dt_out=60, bc=True,
                            cfg_output=True)
    else:
        synth.write_project(str(src), "syn", 2000, days=1.0, max_step=10.0, et_step=60.0, dt_out=60)
    out_c, out_p = tmp_path / "out_cpp", tmp_path / "out_py"
    r = shud_gpu_run.run(["-o", out_c, "-C", src, "-e", 0.25, src, "syn"],
                         env={"SHUD_WB_DIAG": "1", "SHUD_WB_DIAG_QUAD": "1"})
    assert "not supported" not in r.stderr
    line = shud_gpu_run.json_line(r)
    assert line["quad_steps"] == line["cvode_steps"] > 6 and line["loop_phases_s"]["wb_quad"] > 0
    steps, st = tw._python_run(src, out_p, trapz=False, end_day=0.25, quad=True)
    assert steps == st["nst"] == line["cvode_steps"]
    files = tw._dat(out_c)
    assert len(files) == 30 and files == tw._dat(out_p) and set(tw.WB_FILES + [QUAD_FILE]) <= set(files)
    for f in files:
        a, b = open(out_c / f, "rb").read(), open(out_p / f, "rb").read()
        assert a == b, f
        d = shudio.read_dat(str(out_c / f))
        assert d["t"].size == 6 and np.all(np.isfinite(d["data"])), f
        assert np.array_equal(d["t"], np.arange(6) * 60.0), f
    basin = shudio.read_dat(str(out_c / "syn.basinwbfull.dat"))["data"]
    quad = shudio.read_dat(str(out_c / QUAD_FILE))["data"]
    assert np.array_equal(quad[:, 0], basin[:, 0]) and quad[:, 1].sum() > 0
    print("first-row residuals: basin (Euler at solver steps)", basin[0, 8], "quad", quad[0, 8], "dS", basin[0, 0])
    print("six-hour residuals: basin", basin[:, 8].sum(), "quad", quad[:, 8].sum(), "dS", basin[:, 0].sum())
    if case == "plain":
        # what the monitor is for: over the first hour's fast river drain the Euler rule at 10-minute solver steps
        # leaves -3.8e5 m3 of a dS of -1.37e6 m3, the trapezoid at the integrator's own steps 1.9e3 m3 (measured
        # ratio 0.005; asserted with the factor of two the ratio had to clear).  Not asserted with
        # boundary-condition tables: fixed-head elements and reaches move water the budget does not count.
        assert abs(quad[0, 8]) < abs(basin[0, 8])


@pytest.mark.parametrize("value", ["0", None])
def test_driver_quad_off_writes_no_quad_file(tmp_path, value):
    """SHUD_WB_DIAG_QUAD=0 or unset under SHUD_WB_DIAG=1: the 29 files of the diagnostic alone; and
    SHUD_WB_DIAG_QUAD=1 without SHUD_WB_DIAG is not read at all"""
    src = tmp_path / "in"
    synth.write_project(str(src), "syn", 2000, days=1.0, max_step=10.0, et_step=60.0, dt_out=60)
    base = {"SHUD_WB_DIAG": None, "SHUD_WB_DIAG_QUAD": None}
    for name, env, nfiles in (("on", dict(SHUD_WB_DIAG="1", **({} if value is None else {"SHUD_WB_DIAG_QUAD": value})),
                               29), ("nodiag", {"SHUD_WB_DIAG_QUAD": "1"}, 24)):
        r = shud_gpu_run.run(["-o", tmp_path / name, "-C", src, "-e", "0.125", src, "syn"], env=dict(base, **env))
        files = tw._dat(tmp_path / name)
        assert len(files) == nfiles and QUAD_FILE not in files
        assert "wb_quad" not in r.stdout and "quad_steps" not in r.stdout


def test_quad_loop_vs_oracle_chain_first_hour(tmp_path):
    """The device quad loop (ET prelude, integrator in ONE_STEP mode under a stop time, the monitor's f(), the
    monitor) against the CPU chain driven through the same loop: oracle ET, oracle RHS, oracle integrator, the
    restated rates (the reference's sequential sums) and monitor step.  Solver counters identical; y within 1e-6
    of the error weight after every internal step (tests/test_gpu_host.py's bound).  The difference of the seven
    accumulators is printed, not asserted: no spread of the chain under rounding-level perturbations
    (tests/traj.py) was produced for them."""
    synth.write_project(str(tmp_path), "syn", 2000, days=1.0, max_step=10.0, et_step=60.0, dt_out=60)
    P = host.Project(str(tmp_path), "syn", cwd=str(tmp_path))
    c = P.control()
    ctl = driver.solver_control(c)
    y0 = P.array("y0")
    m, h = driver.device_model(P)
    oe = oracle.OracleEt(P.et_model())
    oe.set_state(P.array("y_is"), P.array("y_snow"))
    r = oracle.OracleRhs(m, abi.SHUD_MODE_SERIAL)
    r.set_step_inputs(step={"u_satn": np.zeros(m.num_ele)})
    args = (ctl.start, y0, ctl.reltol, ctl.abstol, ctl.init_step, ctl.max_step, ctl.min_step, ctl.max_num_steps)
    d = rt.OdeSolver(h, *args)
    o = oracle.OracleOde(r, *args)
    d_y, d_du = h.device_alloc(8 * m.num_y), h.device_alloc(8 * m.num_y)
    h.h2d(d_y, y0)
    h.summary(d_y)
    wb = rt.WaterBalance(h, 60, start_time=ctl.start)
    wb.quad_enable()
    qref = qp.QuadMonitorPy(None, start_time=ctl.start)
    t = tnext = ctl.start
    worst = dt_worst = 0.0
    for i in range(6):                                  # 10-minute solver steps, one ET step (60 min)
        tnext += ctl.solver_step
        while t + ZERO < tnext:
            tout = tnext
            f = P.forcing(t, tout)
            assert h.et_step(f) == abi.SHUD_OK and oe.step(f) == (0, -1)
            wb.on_et_update()
            r.set_step_inputs(step=oe.step_inputs())
            eo = oe.get()
            d.set_stop_time(tout)
            o.set_stop_time(tout)
            while t + ZERO < tout:
                fd, td = d.solve_device(tout, d_y, one_step=True)
                fo, t, yo = o.solve(tout, one_step=True)
                # an internal step ends at tn + h, and h is the last h times a power |1/(q+1)| <= 1/2 of an error
                # norm of the two states.  The states are held to 1e-6 of the error weight, i.e. to a relative
                # 1e-6 * reltol of a norm of order one, so every h, and with it the sum t of the h so far, is held
                # to the same relative figure (the times are equal again at every stop time)
                assert fd == fo and fo >= 0 and abs(td - t) <= 1e-6 * ctl.reltol * max(1.0, abs(t)), (fd, fo, td, t)
                dt_worst = max(dt_worst, abs(td - t))
                yd = h.d2h(np.empty(m.num_y), d_y)
                err = np.abs(yd - yo) / (1e-6 * (ctl.reltol * np.abs(yo) + ctl.abstol))
                worst = max(worst, float(err.max()))
                assert err.max() <= 1.0, f"t={t}: {err.max():.3e} of the bound"
                h.eval_device(td, d_y, d_du)             # both monitor f() calls are stateful
                h.refresh_diagnostics()
                wb.quad_step(td)
                _, code, _, _ = r.eval(t, yo)
                assert code == 0
                qref.step(t, qp.quad_rates(m, eo["qEleE_IC"], r.diagnostics(), eo["qEleprep"], order="seq"))
    sd, so = d.stats(), o.stats()
    for key in ["nst", "nfe", "nni", "nli", "netf", "ncfn"]:
        assert sd[key] == so[key], (key, sd[key], so[key])
    q = wb.read_quad()
    assert qref.steps == sd["nst"] and q["last_t"] == qref.last_t == 60.0
    print(f"y: worst {worst:.3e} of the bound over {sd['nst']} internal steps; worst |t_gpu - t_cpu| {dt_worst:.3e}")
    for k, name in enumerate(wb_py.BASIN):
        den = abs(qref.acc[k]) or 1.0
        print(f"quad acc {name}: gpu={q['acc'][k]!r} cpu={qref.acc[k]!r} |d|={abs(q['acc'][k] - qref.acc[k]):.3e} "
              f"rel={abs(q['acc'][k] - qref.acc[k]) / den:.3e}")
    assert np.isfinite(q["acc"]).all() and q["acc"][abi.SHUD_WB_P] >= 0
    wb.close()
    d.close()
    h.device_free(d_y)
    h.device_free(d_du)
    h.close()
    P.close()
