"""GPU: the ET-step prelude on the device (shud_et_step, include/shud_et.h).

(1) Device prelude vs the CPU restatement (oracle/shud_oracle_et.c) over multi-step sequences: every output
    within the parity tolerance (OCML vs glibc exp/log ulps), all configurations (cryosphere queues, SWNET,
    terrain-radiation modes, lakes, LAI = 0).
(2) The prelude writes the RHS step inputs in place: RHS evaluations after shud_et_step equal the oracle RHS
    fed with the prelude's own outputs (both layouts), across ET steps and stateful RHS calls.
(3) The reference's exits from tReadForcing (CheckNonZero(ra), CheckNANi(qPotTran)) -> code 10, first element."""
import numpy as np
import pytest

import cases
import oracle
from conftest import assert_close, rhs_blocks
from shud_rhs import abi, et, workload

pytestmark = pytest.mark.gpu

KEYS = ["t_prcp", "t_temp", "t_lai", "t_mf", "t_rn", "t_wind", "t_rh", "qEleprep", "qPotEvap", "qPotTran",
        "qEleETP", "qEleNetPrep", "qEleE_IC", "yEleIS", "yEleSnow", "fu_surf", "fu_sub", "rn_factor"]


def _seq(n):
    out = []
    for k in range(n):
        mode = abi.SHUD_TSR_RECOMPUTE if k % 4 == 0 else abi.SHUD_TSR_CACHED
        if k == 6:
            mode = abi.SHUD_TSR_NO_TIME
        out.append((360.0 * k, mode))
    return out


@pytest.fixture(params=["packed", "soa"])
def layout(request, monkeypatch):
    monkeypatch.setenv("SHUD_RHS_PACKED", "1" if request.param == "packed" else "0")
    return request.param


@pytest.mark.parametrize("cryo,swnet,terrain", [(0, 0, 1), (1, 0, 1), (1, 1, 0)])
def test_device_et_vs_oracle_and_rhs_chain(cryo, swnet, terrain, layout):
    from shud_rhs import runtime as rt
    m, y = cases.variant(20000, seed=17)
    etm = et.synth_et(m.num_ele, seed=4, terrain=bool(terrain), lake_frac=0.03)
    etm.params.update(cryosphere=cryo, radiation_input_mode=swnet, ft_surf_day=3, ft_sub_day=5)
    h = rt.RhsHandle(m, mode=abi.SHUD_MODE_SERIAL)
    assert h.layout()["packed"] == (layout == "packed")
    h.set_step_inputs()
    h.et_attach(etm)
    oe = oracle.OracleEt(etm)
    orc = oracle.OracleRhs(m, abi.SHUD_MODE_SERIAL)
    orc.set_step_inputs()
    rng = np.random.default_rng(2)
    y_is = rng.uniform(0, 2e-4, m.num_ele)
    y_snow = np.where(rng.random(m.num_ele) < 0.5, 0.0, rng.uniform(0, 0.05, m.num_ele))
    h.et_set_state(y_is, y_snow)
    oe.set_state(y_is, y_snow)
    ys = [y, workload.random_state(m, seed=5)]
    for k, (t, mode) in enumerate(_seq(9)):
        f = et.synth_forcing(t, 360.0, seed=k, tsr_mode=mode if terrain else abi.SHUD_TSR_OFF)
        assert h.et_step(f) == abi.SHUD_OK
        assert oe.step(f) == (0, -1)
        got, ref = h.et_get(), oe.get()
        for key in KEYS:
            assert_close(got[key], ref[key], what=f"step {k} {key}")
        # the RHS now runs on the device-written step inputs; the oracle RHS gets the same values
        orc.set_step_inputs(step=dict(net_prep=got["qEleNetPrep"], pot_evap=got["qPotEvap"],
                                      pot_tran=got["qPotTran"], etp=got["qEleETP"], lai=got["t_lai"],
                                      fu_surf=got["fu_surf"], fu_sub=got["fu_sub"], e_ic=got["qEleE_IC"]))
        for c in range(2):
            yy = ys[(k + c) % 2]
            ref_dy, code, _, _ = orc.eval(t, yy)
            assert code == 0
            assert_close(h.eval(t, yy), ref_dy, what=f"rhs after ET step {k} call {c}", blocks=rhs_blocks(m))
    h.close()


@pytest.mark.parametrize("what,bit,slot", [("wind_nan", abi.EF_ET_RA, 5), ("temp_nan", abi.EF_ET_PT_NAN, 6)])
def test_device_et_exits(what, bit, slot):
    from shud_rhs import runtime as rt
    m, _ = cases.variant(5000, seed=3)
    etm = et.synth_et(m.num_ele, seed=9, terrain=False)
    h = rt.RhsHandle(m)
    h.set_step_inputs()
    h.et_attach(etm)
    f = et.synth_forcing(0.0, 60.0, seed=2)
    st = f.station.copy()
    st[:, 4 if what == "wind_nan" else 2] = np.nan
    f.station = st
    code, idx = oracle.OracleEt(etm).step(f)
    assert code == 10
    with pytest.raises(rt.ShudRhsError) as ei:
        h.et_step(f)
    e = ei.value.err
    assert e["exit_code"] == 10 and e["flags"] & bit and e["first_index"][slot] == idx, e
    h.close()


# ---- the long sequence: full day-mean queues (pop branch, ring wrap-around), exact thresholds ---------------------
def _sized_model(n):
    """a handle-able mesh of n elements (1, 63, 257) or a synthetic one of a few thousand"""
    if n == 1:
        return cases.single_element()[0]
    m0, _ = cases.ccw()
    if n <= m0.num_ele:
        return cases._subset(m0, np.arange(n))
    return cases.variant(n, seed=17)[0]


@pytest.mark.parametrize("n", [1, 63, 257, 4000])
def test_device_et_long_sequence(n, layout):
    """tests/et_long.py on the device against OracleEt (which tests/test_et.py holds to PyEt bit for bit, with the
    queue pushes and pops counted there): 28 steps, 7 day pushes, the 2-day queue pops 5 times and the 3-day queue
    4 times with its ring wrapping, sizes below / across one and several 256-thread blocks.
    t_*, rn_factor, yEleSnow, fu_surf, fu_sub use IEEE-exact operations only in the reference's order (the kernels
    are built with -ffp-contract=off): bit-equal, so a wrong ring slot or a wrong day count cannot hide inside a
    tolerance.  The outputs that pass through exp / log keep the parity tolerance."""
    import et_long
    from shud_rhs import runtime as rt
    m = _sized_model(n)
    ne = m.num_ele
    assert ne == n or (n == 4000 and 3000 < ne < 5000 and ne % 256 != 0)
    etm, y_is, y_snow = et_long.et_model(ne)
    h = rt.RhsHandle(m, mode=abi.SHUD_MODE_SERIAL)
    assert h.layout()["packed"] == (layout == "packed"), (n, h.layout())      # every size takes both layouts
    h.set_step_inputs(step=workload.random_step_inputs(m, seed=3))
    h.et_attach(etm)
    h.et_set_state(y_is, y_snow)
    oe = oracle.OracleEt(etm)
    oe.set_state(y_is, y_snow)
    fs = et_long.forcings(first_cached=False)
    cached = et_long.forcings()[0]
    with pytest.raises(rt.ShudRhsError) as ei:            # the handle refuses CACHED before any RECOMPUTE ...
        h.et_step(cached)
    assert ei.value.code == abi.SHUD_ERR_ARG              # ... before it touches its day-mean bookkeeping
    for k, f in enumerate(fs):
        assert h.et_step(f) == abi.SHUD_OK
        assert oe.step(f) == (0, -1)
        got, ref = h.et_get(), oe.get()
        for key in KEYS:
            if key in et_long.EXACT:
                same = (got[key] == ref[key]) | (np.isnan(got[key]) & np.isnan(ref[key]))
                assert same.all(), f"step {k} {key}: {(~same).sum()} of {ne} differ, first {np.argmax(~same)}"
            else:
                assert_close(got[key], ref[key], what=f"step {k} {key}")
    assert ((ref["fu_surf"] > 0) & (ref["fu_surf"] < 1)).any() or n == 1
    h.close()


def test_device_et_vs_recorded_reference(tmp_path, layout):
    """shud_et_step over ccw with the cryosphere on and short queues, fed by the C++ host's forcing rows, against
    what the reference's own updateforcing / ET dumped per step (tests/golden/ref/ccw_et_prelude: every third
    element, 22 steps of 330 min, both queues pop): the ET parity tolerance."""
    import sys
    from conftest import ORACLE_DIR, load_fixture
    sys.path.insert(0, f"{ORACLE_DIR}/ref")
    import refio
    from shud_rhs import host
    from shud_rhs import runtime as rt
    rec = refio.load_recording("ccw_et_prelude")
    indir = refio.unpack_et(tmp_path)
    P = host.Project(indir, "ccw", cwd=str(tmp_path))
    c = P.control()
    m, _ = load_fixture("ccw")
    h = rt.RhsHandle(m, mode=abi.SHUD_MODE_SERIAL)
    assert h.layout()["packed"] == (layout == "packed")
    h.set_step_inputs(step={"u_satn": np.zeros(m.num_ele)})
    h.et_attach(P.et_model())
    h.et_set_state(P.array("y_is"), P.array("y_snow"))
    worst = {}
    for k in range(refio.ET_STEPS):
        t = float(rec["t"][k])
        assert h.et_step(P.forcing(t, t + c["et_step"])) == abi.SHUD_OK
        got = h.et_get()
        for key in refio.ET_KEYS + ["t_temp", "t_prcp", "rn_factor"]:
            a, r = assert_close(got[key][::refio.ET_STRIDE], rec[key][k], what=f"ET step {k} {key}")
            worst[key] = max(worst.get(key, 0.0), r)
    print("REFPIN ccw_et_prelude", layout, {k: f"{v:.2e}" for k, v in worst.items()})
    h.close()
