"""GPU: the water-balance diagnostics on the device (include/shud_wb.h; the reference's WaterBalanceDiag) against
the numpy restatement (tests/wb_py.py) fed with the values read back from the handle: the replayed flux arrays of
the last f() (RhsHandle.diagnostics), the state, DY and the step inputs.

Per element the device keeps the reference's operation order: accumulators and residuals must match bit for bit.
Basin sums are reductions: each is held to the bound every summation order meets,
|gpu - fsum(terms)| <= (n - 1) 2^-53 sum|terms|, and files are compared byte for byte against the restatement
run with the device's reduction tree (wb_py.device_sum).  Outlet discharge through Manning's equation uses cbrt
(OCML on the device, glibc in the restatement): it is held to the project's parity tolerance, and the models of
the bound and file tests carry critical-depth outlets only (sqrt: correctly rounded on both sides), so their
terms are exact."""
import glob
import math
import os

import numpy as np
import pytest

import cases
import ode_kernels_py
import shud_gpu_run
import wb_py
from conftest import ATOL, RTOL
from shud_rhs import abi, driver, et, partition, shudio, synth, workload
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu
ARR4 = ["acc3", "accfull", "acc3_budget", "accfull_budget"]
RES4 = ["resid3", "residfull", "resid3_budget", "residfull_budget"]


def _critical_outlets(m):
    """every outlet a critical-depth one (down = -4): Qout terms without cbrt"""
    m.riv_down[m.riv_down < 0] = -4
    return m.finalize()


class Rig:
    """a handle with its device vectors, driven like the loop: state -> f() -> summary -> flux arrays"""

    def __init__(self, m, mode=abi.SHUD_MODE_SERIAL, storages=False):
        """storages: attach an ET prelude and give it non-zero yEleSnow / yEleIS (set_storages); without one the
        diagnostic reads both as 0.0"""
        self.m = m
        self.h = rt.RhsHandle(m, mode=mode)
        self.h.set_step_inputs()
        self.d_y, self.d_f, self.d_du = (self.h.device_alloc(8 * m.num_y) for _ in range(3))
        self.snow = self.ice = np.zeros(m.num_ele)
        if storages:
            self.h.et_attach(et.synth_et(m.num_ele, seed=4, lake_frac=0.0))
            self.set_storages(1)

    def set_storages(self, seed):
        """yEleSnow (half the elements bare, up to 5 cm) and yEleIS (up to 0.2 mm): unlike each other, so a swap shows"""
        rng = np.random.default_rng(900 + seed)
        NE = self.m.num_ele
        self.snow = np.where(rng.random(NE) < 0.5, 0.0, rng.uniform(0.0, 0.05, NE))
        self.ice = rng.uniform(1e-5, 2e-4, NE)
        self.h.et_set_state(self.ice, self.snow)

    def advance(self, t, y):
        h = self.h
        h.h2d(self.d_y, y)
        h.eval_device(t, self.d_y, self.d_f)
        h.summary(self.d_y)
        h.refresh_diagnostics()
        self.y = y

    def state(self):
        return wb_py.host_summary(self.m, self.y) + (self.snow, self.ice)

    def new_step(self, seed):
        self.m.step = workload.random_step_inputs(self.m, seed=seed)
        self.h.set_step_inputs()

    def close(self):
        for p in (self.d_y, self.d_f, self.d_du):
            self.h.device_free(p)
        self.h.close()


def _both_sample(rig, wb, ref, t, dy):
    """sample + maybeWrite on the device and in the restatement; -> (wrote, device read-back)"""
    m = rig.m
    rig.h.h2d(rig.d_du, dy)
    wb.sample(t, rig.d_du)
    wrote = wb.maybe_write(t)
    d = rig.h.diagnostics()
    st = rig.state()
    ref.sample(t, dy, d, m.step["prcp"], m.step["net_prep"], st[3])
    assert ref.maybe_write(t, st) == wrote, t
    return wrote, wb.read()


@pytest.mark.parametrize("trapz", [False, True])
def test_per_element_arithmetic_bit_for_bit(trapz):
    """variant(n=2000): open boundary, +-BC elements and reaches, SS flags, every outlet code, negative states.
    Seven integrating samples with unequal dt, one repeated t (the early return), interval ends at 60 and 120;
    ic_raw from fresh step inputs and from the carried qEleE_IC of the last f().  An ET prelude is attached with
    non-zero snow and interception storages that change between the rows (the "full" storages read them)."""
    m, y0 = cases.variant(n=2000)
    rig = Rig(m, storages=True)
    rig.advance(0.0, y0)
    wb = rt.WaterBalance(rig.h, 60, start_time=0.0, trapz=trapz)
    ref = wb_py.WaterBalancePy(m, 60, rig.state(), trapz=trapz)
    wb.on_et_update()
    ref.on_et_update(rig.h.diagnostics()["e_ic"])              # the carried value after the first f()
    rng = np.random.default_rng(21)
    plan = [(7.5, None), (20.0, "step"), (20.0, None), (45.25, "carried"), (60.0, None), (61.5, "step"),
            (95.0, None), (120.0, "carried")]
    rows = 0
    for k, (t, et) in enumerate(plan):
        if et == "step":                                       # ET(t, tout) then onETUpdate
            rig.new_step(seed=300 + k)
            rig.set_storages(k)
            wb.on_et_update()
            ref.on_et_update(m.step["e_ic"])
        rig.advance(t, y0 if k == 0 else workload.random_state(m, seed=500 + k))
        if et == "carried":
            wb.on_et_update()
            ref.on_et_update(rig.h.diagnostics()["e_ic"])
        dy = rng.normal(0.0, 1e-4, m.num_y)
        wrote, g = _both_sample(rig, wb, ref, t, dy)
        assert wrote == (t in (60.0, 120.0))
        rows += wrote
        for j, name in enumerate(ARR4):
            assert np.array_equal(g[name], ref.acc[j], equal_nan=True), (k, t, name)
        if wrote:
            for j, name in enumerate(RES4):
                assert np.array_equal(g[name], ref.resid[j], equal_nan=True), (k, t, name)
                assert np.abs(g[name]).max() > 0
            assert not np.array_equal(g["resid3"], g["residfull"])     # the snow / interception change is in
        assert g["last_t"] == t and g["rows"] == rows
    assert rows == 2
    wb.close()
    rig.close()


def _bound_case(ne):
    if ne == 1:
        return cases.single_element(0)
    if ne >= 2000:
        m, _ = cases.variant(n=ne)
        m = _critical_outlets(m)
        return m, workload.random_state(m, seed=77)
    m0, _ = cases.ccw()
    r = cases._subset(m0, np.arange(ne), close_boundary=0)
    return r, workload.random_state(r, seed=70 + ne)


def _check_bound(name, got, terms, must_be_live=False):
    terms = np.asarray(terms, dtype=np.float64).ravel()
    n, s_abs = terms.size, math.fsum(np.abs(terms).tolist())
    bound = max(n - 1, 0) * 2.0 ** -53 * s_abs
    ref = math.fsum(terms.tolist())
    print(f"{name}: n={n} gpu={got!r} fsum={ref!r} |d|={abs(got - ref):.3e} bound={bound:.3e}")
    if must_be_live:
        assert s_abs > 0, name
    assert abs(got - ref) <= bound, (name, got, ref, bound)


def _check_order(name, got, terms):
    """the same bits as the one reduction order of the device (csrc/shud_reduce.h, shared with the integrator) as
    tests/ode_kernels_py.py restates it; terms: one per element in index order, fp64 numpy, left to right"""
    want = ode_kernels_py.device_order_sum(np.asarray(terms, dtype=np.float64))
    print(f"{name}: gpu={got!r} device_order_sum={want!r}")
    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64), (name, got, want)


@pytest.mark.parametrize("ne", [1, 63, 64, 65, 255, 256, 257, 2000, 1_060_000, 4_250_000])
def test_reduction_edges(ne):
    """Sizes around the wave (64) and quarter-workgroup edges, and NE = 2000 (two 1024-lane workgroups, +-BC
    elements and reaches, critical-depth outlets); every case has an open boundary, so the edge sum is live.
    The finalize kernel is one 1024-thread workgroup: up to 1024 partials (NE <= 1,048,576) each thread takes at
    most one, into its first accumulator; above that the four interleaved accumulators of a thread fill (partials
    t + k*1024), and above 4096 partials (NE > 4,194,304) its loop makes a second trip.  Both sizes are here,
    just above each limit: a wrong stride or index there drops or doubles partials only on such meshes."""
    m, y = _bound_case(ne)
    assert m.close_boundary == 0
    NE = m.num_ele
    if ne < 2000:
        assert NE == ne
    elif ne > 2000:                                            # just above 1024 / 4096 workgroups of 1024 lanes
        lim = (1 << 20) if ne < 2_000_000 else (4 << 20)
        assert lim < NE < 1.1 * lim, NE
    rig = Rig(m)
    rig.advance(0.0, y)
    wbs = [rt.WaterBalance(rig.h, 60) for _ in range(2)]
    st = rig.state()
    g0 = wbs[0].read(arrays=False)
    _check_bound("storage_ele", g0["storage"][0], sfull_of(m, st) * m.ele["area"], must_be_live=True)
    _check_order("storage_ele", g0["storage"][0], sfull_of(m, st) * m.ele["area"])
    _check_bound("storage_riv", g0["storage"][1], wb_py.river_storage_terms(m, st[3]), must_be_live=m.num_riv > 0)
    rig.advance(12.5, workload.random_state(m, seed=9))
    dy = np.random.default_rng(ne).normal(0.0, 1e-4, m.num_y)
    rig.h.h2d(rig.d_du, dy)
    for w in wbs:
        w.on_et_update()
        w.sample(12.5, rig.d_du)
    d = rig.h.diagnostics()
    st = rig.state()
    ic = d["e_ic"]                                             # on_et_update after f(): the carried value
    nb = np.asarray(m.nabr).reshape(3, NE)
    qe = d["qele_surf"].reshape(3, NE) + d["qele_sub"].reshape(3, NE)
    g = wbs[0].read()
    rate = g["basin_rate"]
    assert np.array_equal(g["basin_acc"], rate * 12.5)
    _check_bound("P", rate[abi.SHUD_WB_P], m.step["prcp"] * m.ele["area"], must_be_live=True)
    _check_order("P", rate[abi.SHUD_WB_P], m.step["prcp"] * m.ele["area"])
    _check_bound("ET", rate[abi.SHUD_WB_ET],
                 (ic + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * m.ele["area"], must_be_live=True)
    _check_order("ET", rate[abi.SHUD_WB_ET],
                 (ic + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * m.ele["area"])
    _check_bound("Qout", rate[abi.SHUD_WB_QOUT], wb_py.outlet_terms(m, st[3])[wb_py.outlet_list(m)],
                 must_be_live=ne >= 2000)
    _check_bound("Qedge", rate[abi.SHUD_WB_QEDGE], qe[nb < 0], must_be_live=True)
    _check_bound("Qbc", rate[abi.SHUD_WB_QBC], np.concatenate([wb_py.ele_qbc(m)[np.asarray(m.ibc) < 0],
                                                              wb_py.riv_qbc(m)[np.asarray(m.riv_bc) < 0]]),
                 must_be_live=ne >= 2000)
    _check_bound("Qss", rate[abi.SHUD_WB_QSS], np.zeros(int((np.asarray(m.iss) != 0).sum())))
    _check_bound("noncons", rate[abi.SHUD_WB_NONCONS], qe[nb >= 0], must_be_live=ne >= 2000)
    assert g["n_outlets"] == wb_py.outlet_list(m).size
    # two independent diagnostics on the same inputs: identical bits
    g2 = wbs[1].read()
    for key in g:
        assert np.array_equal(np.asarray(g[key]), np.asarray(g2[key]), equal_nan=True), key
    assert wbs[0].maybe_write(60.0) and wbs[1].maybe_write(60.0)
    ga, gb = wbs[0].read(), wbs[1].read()
    for key in ga:
        assert np.array_equal(np.asarray(ga[key]), np.asarray(gb[key]), equal_nan=True), key
    _check_bound("storage_ele@write", ga["storage"][0], sfull_of(m, st) * m.ele["area"], must_be_live=True)
    _check_order("storage_ele@write", ga["storage"][0], sfull_of(m, st) * m.ele["area"])
    for w in wbs:
        w.close()
    rig.close()


def sfull_of(m, st):
    return (st[0] + m.par["Sy"] * st[1] + m.par["Sy"] * st[2]) + st[4] + st[5]


def test_outlets():
    """Qout on variant (outlet codes -1..-4; Manning and critical depth) within the parity tolerance; one Manning
    outlet driven to a negative stage (cross-section area clamped at 0: its term is 0); exactly 0.0 without
    rivers."""
    m, _ = cases.variant(n=2000)
    y = workload.random_state(m, seed=31)
    outs = wb_py.outlet_list(m)
    assert set(np.asarray(m.riv_down)[outs].tolist()) == {-1, -2, -3, -4}
    neg = [r for r in outs if m.riv_down[r] != -4 and m.riv_bc[r] == 0][0]
    y[3 * m.num_ele + neg] = -0.3
    rig = Rig(m)
    rig.advance(0.0, y)
    wb = rt.WaterBalance(rig.h, 60)
    rig.advance(5.0, y)
    rig.h.h2d(rig.d_du, np.zeros(m.num_y))
    wb.sample(5.0, rig.d_du)
    st = rig.state()
    terms = wb_py.outlet_terms(m, st[3])
    raw = st[3][neg] * (m.riv["riv_bottom_width"][neg] + st[3][neg] * m.riv["riv_bankslope"][neg])
    assert raw < 0 and terms[neg] == 0.0                     # the clamp decides this term
    ref = math.fsum(terms[outs])
    got = wb.read(arrays=False)["basin_rate"][abi.SHUD_WB_QOUT]
    print(f"Qout gpu={got!r} ref={ref!r} |d|={abs(got - ref):.3e}")
    assert ref > 0 and abs(got - ref) <= RTOL * abs(ref) + ATOL
    wb.close()
    rig.close()

    m, y = cases.riverless()
    rig = Rig(m)
    rig.advance(0.0, y)
    wb = rt.WaterBalance(rig.h, 60)
    rig.advance(5.0, y)
    rig.h.h2d(rig.d_du, np.zeros(m.num_y))
    wb.sample(5.0, rig.d_du)
    g = wb.read(arrays=False)
    assert g["n_outlets"] == 0 and g["basin_rate"][abi.SHUD_WB_QOUT] == 0.0 and g["storage"][1] == 0.0
    assert g["basin_rate"][abi.SHUD_WB_QEDGE] == 0.0           # ccw: CloseBoundary
    assert g["basin_rate"][abi.SHUD_WB_P] > 0
    wb.close()
    rig.close()


@pytest.mark.parametrize("trapz", [False, True])
def test_files_byte_identical(tmp_path, trapz):
    """the five files of a short hand-driven run against the restatement's; row times are tf - interval"""
    m, _ = cases.variant(n=2000)
    m = _critical_outlets(m)
    hdr = dict(forc_start_time=20000101, radiation_input_mode=1, terrain_radiation=1, solar_lonlat_mode="FIXED",
               lon=-122.71, lat=39.195)
    rig = Rig(m, storages=True)
    rig.advance(0.0, workload.random_state(m, seed=40))
    wb = rt.WaterBalance(rig.h, 30, trapz=trapz, prefix=tmp_path / "dev", **hdr)
    ref = wb_py.WaterBalancePy(m, 30, rig.state(), trapz=trapz, prefix=tmp_path / "ref", **hdr)
    wb.on_et_update()
    ref.on_et_update(rig.h.diagnostics()["e_ic"])
    rng = np.random.default_rng(8)
    wrote = []
    for k, t in enumerate([10.0, 30.4, 30.9, 47.0, 60.0, 75.5, 90.0]):
        rig.advance(t, workload.random_state(m, seed=41 + k))
        rig.set_storages(10 + k)
        wrote.append(_both_sample(rig, wb, ref, t, rng.normal(0.0, 1e-4, m.num_y))[0])
    assert wrote == [False, True, False, False, True, False, True]
    g = wb.read(arrays=False)
    assert np.array_equal(g["basin_row"], ref.basin_row)
    wb.close()
    ref.close()
    for k, (_, ext) in enumerate(wb_py.LABELS):
        a, b = open(str(tmp_path / "dev") + ext, "rb").read(), open(str(tmp_path / "ref") + ext, "rb").read()
        assert a == b, (ext, len(a), len(b))
        d = shudio.read_dat(str(tmp_path / "dev") + ext)
        assert d["t"].tolist() == [0.0, 30.0, 60.0] and d["data"].shape[1] == (m.num_ele if k < 4 else 9)
        assert np.isfinite(d["data"]).all()
    rig.close()


def test_write_errors_surface(tmp_path):
    """a file on /dev/full: the error comes out of maybe_write or, at the latest, close"""
    m, y = cases.single_element()
    rig = Rig(m)
    rig.advance(0.0, y)
    (tmp_path / "w.elewb3_resid.dat").symlink_to("/dev/full")
    wb = rt.WaterBalance(rig.h, 30, prefix=tmp_path / "w")
    errs = []
    for call in (lambda: wb.maybe_write(30.0), wb.close):
        try:
            call()
        except rt.ShudRhsError as e:
            errs.append(e)
    assert errs and "elewb3_resid" in str(errs[0]) and errs[0].code == abi.SHUD_WB_ERR_IO
    rig.close()


def _python_run(src, outdir, trapz, end_day=-1.0, quad=False):
    """shud_rhs.driver's run with the diagnostics (quad: and the monitor) -> (monitor steps, integrator stats)"""
    run = driver.ProjectRun(src, "syn", outdir, cwd=src, end_day=end_day, wb=True, trapz=trapz, quad=quad).start()
    t, _ = run.run()
    assert abs(t - run.c["end_time"]) < 1e-6
    res = run.sv.quad_steps, run.sv.stats()
    run.close()
    return res


def _shud_gpu(src, outdir, env, end_day=None):
    return shud_gpu_run.run(["-o", outdir, "-C", src] + (["-e", end_day] if end_day else []) + [src, "syn"], env=env)


def _dat(d):
    return sorted(os.path.basename(f) for f in glob.glob(str(d / "*.dat")))


WB_FILES = sorted("syn" + ext for _, ext in wb_py.LABELS)


@pytest.mark.parametrize("case", ["plain", "bc_substep", "trapz"])
def test_drivers_byte_identical(tmp_path, case):
    """shud_gpu with SHUD_WB_DIAG=1 against ShudSolver.run(wb=...) over the same project: the 24 ordinary and the 5
    new .dat files byte-identical, every value finite.  trapz: SHUD_WB_DIAG_TRAPZ=1 over the first six hours."""
    src = tmp_path / "in"
    if case == "bc_substep":
        synth.write_project(str(src), "syn", 2000, days=1.0, max_step=30.0, et_step=10.0, dt_out=60, bc=True,
                            cfg_output=True)
    else:
        synth.write_project(str(src), "syn", 2000, days=1.0, max_step=10.0, et_step=60.0, dt_out=60)
    env = {"SHUD_WB_DIAG": "1"}
    end_day, nrow = (0.25, 6) if case == "trapz" else (None, 24)
    if case == "trapz":
        env["SHUD_WB_DIAG_TRAPZ"] = "1"
    out_c, out_p = tmp_path / "out_cpp", tmp_path / "out_py"
    r = _shud_gpu(src, out_c, env, end_day)
    assert '"wb_diag"' in r.stdout
    _python_run(src, out_p, trapz=case == "trapz", end_day=end_day or -1.0)
    files = _dat(out_c)
    assert len(files) == 29 and files == _dat(out_p) and set(WB_FILES) <= set(files)
    for f in files:
        a, b = open(out_c / f, "rb").read(), open(out_p / f, "rb").read()
        assert a == b, f
        d = shudio.read_dat(str(out_c / f))
        assert d["t"].size == nrow and np.all(np.isfinite(d["data"])), f
        assert np.array_equal(d["t"], np.arange(nrow) * 60.0), f
    basin = shudio.read_dat(str(out_c / "syn.basinwbfull.dat"))["data"]
    assert basin.shape == (nrow, 9) and basin[:, 1].sum() > 0    # it rained
    print("basin residual / accumulated P:", basin[:, 8].sum() / basin[:, 1].sum())


def test_driver_off_writes_no_diagnostic_files(tmp_path):
    """SHUD_WB_DIAG=off: exactly the 24 ordinary files, identical to a run without the variable"""
    src = tmp_path / "in"
    synth.write_project(str(src), "syn", 2000, days=1.0, max_step=10.0, et_step=60.0, dt_out=60)
    _shud_gpu(src, tmp_path / "off", {"SHUD_WB_DIAG": "off"}, end_day=0.125)
    _shud_gpu(src, tmp_path / "unset", {"SHUD_WB_DIAG": None}, end_day=0.125)
    files = _dat(tmp_path / "off")
    assert len(files) == 24 and not set(WB_FILES) & set(files) and files == _dat(tmp_path / "unset")
    for f in files:
        assert open(tmp_path / "off" / f, "rb").read() == open(tmp_path / "unset" / f, "rb").read(), f


def test_no_side_effects():
    """the same RHS evaluations from the same handle state, once with on_et_update / sample / maybe_write between
    them (no extra stateful eval) and once without: identical DY and carried state, bit for bit"""
    m, y0 = cases.variant(n=2000)
    res = []
    for with_wb in (True, False):
        rig = Rig(m)
        rig.advance(0.0, y0)
        wb = rt.WaterBalance(rig.h, 20) if with_wb else None
        dys = []
        for k in range(5):
            t = 10.0 * (k + 1)
            if wb:
                wb.on_et_update()
            rig.advance(t, workload.random_state(m, seed=60 + k))
            dys.append(rig.h.d2h(np.empty(m.num_y), rig.d_f))
            if wb:
                rig.h.h2d(rig.d_du, dys[-1])
                wb.sample(t, rig.d_du)
                assert wb.maybe_write(t) == (k % 2 == 1)
        d = rig.h.diagnostics()
        res.append((dys, d["e_ic"], d["u_satn"]))
        if wb:
            wb.close()
        rig.close()
    for a, b in zip(res[0][0], res[1][0]):
        assert np.array_equal(a, b, equal_nan=True)
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


@pytest.mark.parametrize("kind", ["omp", "lake", "partitioned"])
def test_refusals(kind):
    """SHUD_ERR_UNSUPPORTED with a message from shud_wb_create"""
    if kind == "omp":
        m, _ = cases.ccw()
        h = rt.RhsHandle(m, mode=abi.SHUD_MODE_OMP)
    elif kind == "lake":
        m, _ = cases.qhh()
        h = rt.RhsHandle(m)
    else:
        m, _ = cases.variant(n=2000)
        _, _, plans = partition.build_plans(m, 2)
        lm, part = partition.local_model(m, plans[0], 0, 2)
        h = rt.RhsHandle(lm, partition=part)
    with pytest.raises(rt.ShudRhsError) as e:
        rt.WaterBalance(h, 60)
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED
    assert len(str(e.value).split("shud_wb_create:", 1)[1].strip()) > 10
    h.close()
