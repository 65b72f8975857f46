"""ET-step prelude (include/shud_et.h).

CPU: the C restatement (oracle/shud_oracle_et.c) equals the independent pure-Python restatement
(tests/et_py.py) bit for bit over multi-step sequences covering lakes, LAI = 0, NA station elevation,
RH clamps, rain/snow/melt regimes, SWDOWN/SWNET, every TSR mode and the cryosphere day-mean queues; and the
reference's exits (CheckNonZero(ra), CheckNANi(qPotTran) -> 10) at the first element in loop order."""
import numpy as np
import pytest

import oracle
from et_py import PyEt
from shud_rhs import abi, et

KEYS = ["t_prcp", "t_temp", "t_lai", "t_mf", "t_rn", "t_wind", "t_rh", "qEleprep", "qPotEvap", "qPotTran",
        "qEleETP", "qEleNetPrep", "qEleE_IC", "yEleIS", "yEleSnow", "fu_surf", "fu_sub", "rn_factor"]


def _seq(n_steps):
    """(t, tsr_mode) sequence: a new forcing interval every 4 steps, one step without forcing time"""
    out = []
    for k in range(n_steps):
        mode = abi.SHUD_TSR_RECOMPUTE if k % 4 == 0 else abi.SHUD_TSR_CACHED
        if k == 6:
            mode = abi.SHUD_TSR_NO_TIME
        out.append((360.0 * k, mode))
    return out


def _bitwise(a, b):
    return np.array_equal(a, b) or bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("cryo,swnet,terrain", [(0, 0, 1), (1, 0, 1), (1, 1, 0)])
def test_oracle_et_vs_python(cryo, swnet, terrain):
    etm = et.synth_et(240, seed=5, terrain=bool(terrain), lake_frac=0.05)
    etm.params.update(cryosphere=cryo, radiation_input_mode=swnet, ft_surf_day=3, ft_sub_day=5)
    o, py = oracle.OracleEt(etm), PyEt(etm)
    rng = np.random.default_rng(1)
    y_is, y_snow = rng.uniform(0, 2e-4, 240), np.where(rng.random(240) < 0.5, 0.0, rng.uniform(0, 0.05, 240))
    o.set_state(y_is, y_snow)
    py.y_is[:], py.y_snow[:] = y_is, y_snow
    for k, (t, mode) in enumerate(_seq(10)):
        f = et.synth_forcing(t, 360.0, seed=k, tsr_mode=mode if terrain else abi.SHUD_TSR_OFF)
        assert o.step(f) == (0, -1)
        assert py.step(f) == (0, -1)
        got = o.get()
        for key in KEYS:
            assert _bitwise(got[key], py.out[key]), f"step {k} {key}"


@pytest.mark.parametrize("what", ["wind_nan", "temp_nan"])
def test_oracle_et_exits(what):
    etm = et.synth_et(200, seed=9, terrain=False)
    f = et.synth_forcing(0.0, 60.0, seed=2)
    st = f.station.copy()
    if what == "wind_nan":        # Uz NaN -> ra NaN -> CheckNonZero -> exit 10
        st[:, 4] = np.nan
    else:                         # TMP NaN -> qPotTran NaN (ra is fine) -> CheckNANi -> exit 10
        st[:, 2] = np.nan
    f.station = st
    lai = etm.arrays["ilc"]
    first_veg = int(np.nonzero((f.lai_row[lai] > 0) & (etm.arrays["ilake"] == 0))[0][0])
    o, py = oracle.OracleEt(etm), PyEt(etm)
    assert o.step(f) == (10, first_veg)
    assert py.step(f) == (10, first_veg)


# ---- the prelude pinned to the reference's own updateAllTimeSeries / updateforcing / ET ---------------------------
def _ref_prelude_check(rec, stride, tmp_path):
    """the project's own forcing path (the C++ host readers' rows, shud_project_forcing) into OracleEt over ccw
    with the cryosphere on, against what the reference dumped per ET step: bit for bit"""
    import refio
    from shud_rhs import host
    indir = refio.unpack_et(tmp_path)
    P = host.Project(indir, "ccw", cwd=str(tmp_path))
    c = P.control()
    assert c["cryosphere"] == 1 and c["et_step"] == 330.0
    etm = P.et_model()
    assert (etm.params["ft_surf_day"], etm.params["ft_sub_day"]) == (2, 3)
    assert np.array_equal(P.array("y_is"), rec["ic_is"]) and np.array_equal(P.array("y_snow"), rec["ic_snow"])
    oe = oracle.OracleEt(etm)
    oe.set_state(P.array("y_is"), P.array("y_snow"))
    names = dict(fu_surf="fu_surf", fu_sub="fu_sub")
    partial = 0
    for k in range(refio.ET_STEPS):
        t = float(rec["t"][k])
        assert t == c["start_time"] + k * c["et_step"]
        assert oe.step(P.forcing(t, t + c["et_step"])) == (0, -1)
        got = oe.get()
        for key in refio.ET_KEYS + ["t_temp", "t_prcp", "rn_factor"]:
            a, b = got[names.get(key, key)][::stride], rec[key][k]
            assert _bitwise(a, b), f"ET step {k} {key}: {int((a != b).sum())} of {a.size} entries differ"
        partial += int(((rec["fu_surf"][k] > 0) & (rec["fu_surf"][k] < 1)).sum())
    assert partial > 0 and rec["qEleNetPrep"].max() > 0 and rec["qEleE_IC"].max() > 0     # the run is not trivial
    assert np.unique(rec["fu_sub"][-1]).size > 1 or np.unique(rec["fu_sub"]).size > 2


def test_oracle_et_vs_recorded_reference(tmp_path):
    import sys
    from conftest import ORACLE_DIR
    sys.path.insert(0, f"{ORACLE_DIR}/ref")
    import refio
    _ref_prelude_check(refio.load_recording("ccw_et_prelude"), refio.ET_STRIDE, tmp_path)


def test_oracle_et_vs_live_reference(tmp_path):
    """a fresh run of the reference binary, every element; the committed recording must equal it.  Passes
    vacuously (not skipped) where oracle/_ref/ was not built: the recorded test carries the comparison."""
    import sys
    from conftest import ORACLE_DIR
    sys.path.insert(0, f"{ORACLE_DIR}/ref")
    import refio
    if not refio.live_status("ccw_et_prelude"):
        return
    ref_dir = tmp_path / "ref"
    live = refio.run_et_case(ref_dir, stride=1)
    _ref_prelude_check(live, 1, tmp_path / "own")
    rec = refio.load_recording("ccw_et_prelude")
    for key, v in rec.items():
        w = live[key][:, ::refio.ET_STRIDE] if live[key].ndim == 2 else live[key]
        assert _bitwise(v, w), f"recording ccw_et_prelude: {key} is stale"


# ---- the long sequence: full day-mean queues, exact thresholds (tests/et_long.py) --------------------------------
@pytest.mark.parametrize("n", [1, 63, 257, 1031])
def test_long_sequence_oracle_vs_python(n):
    import et_long
    etm, y_is, y_snow = et_long.et_model(n)
    o, py = oracle.OracleEt(etm), PyEt(etm)
    o.set_state(y_is, y_snow)
    py.y_is[:], py.y_snow[:] = y_is, y_snow
    hit = dict(snow_lo=0, snow_hi=0, melt0=0, cap=0, meltlim=0)
    for k, f in enumerate(et_long.forcings()):
        ic_before, sn_before = py.y_is.copy(), py.y_snow.copy()
        assert o.step(f) == (0, -1)
        assert py.step(f) == (0, -1)
        got = o.get()
        for key in KEYS:
            assert _bitwise(got[key], py.out[key]), f"step {k} {key}"
        T = py.out["t_temp"]
        na = (etm.arrays["iforc"] == 3) | (etm.arrays["z_surf"] == -9999.0)
        assert np.array_equal(T[na], f.station[etm.arrays["iforc"][na], 2])          # temp == t0 exactly
        hit["snow_lo"] += int((T == -3.0).sum())
        hit["snow_hi"] += int((T == 1.0).sum())
        hit["melt0"] += int((T == 0.0).sum())
        vg = etm.arrays["veg_frac"]
        lai = py.out["t_lai"]
        with np.errstate(divide="ignore", invalid="ignore"):
            hit["cap"] += int(((vg > 1e-10) & (lai > 1e-10) & (ic_before / vg > 0.0002 * lai)).sum())
        dt = f.t_next - f.t
        hit["meltlim"] += int(((sn_before > 0) & (T > 0) & (T * py.out["t_mf"] > sn_before / dt)).sum())
        if k == 0 or k == 9 or k == 10:      # CACHED before any RECOMPUTE; all-night RECOMPUTE and its CACHED step
            assert np.all(py.out["rn_factor"] == 0.0)
        if k == 1:
            assert np.any(py.out["rn_factor"] > 0.0)
    # every element's queues: seven pushes, the 2-day queue popped five times and the 3-day queue four times,
    # day means over a varying number of samples
    for acc, days in ((py.acc_s, 2), (py.acc_g, 3)):
        for a in acc:
            assert a.pushes == 7 >= 3 + 3 and a.pops == 7 - days and len(a.q) == days
            assert len(set(a.n_of_day[1:])) > 1
    if n >= 63:
        assert all(v > 0 for v in hit.values()), hit
    fu = py.out["fu_surf"]
    assert n < 63 or ((fu > 0) & (fu < 1)).any()
