"""GPU: the device RHS held to the REFERENCE model's own f(), from the recordings under tests/golden/ref/ alone
(oracle/ref/record.py wrote them from the reference binaries; tests/test_ref_pin.py holds the CPU oracle to the
same recordings bit for bit).  Every recorded call is evaluated in order on one handle, so the carried qEleE_IC /
u_satn / stale-gw state advances as in the reference process.  Tolerance: the project's own, conftest.RTOL / ATOL
with the sf / us / gw / riv cancellation blocks and the default max_cancel.  qhh (lakes) exists in serial mode and in
the packed layout only (the handle refuses the others: tests/test_gpu_parity.py test_lakes_unsupported_modes)."""
import os
import sys

import numpy as np
import pytest

from conftest import ORACLE_DIR, assert_close, rhs_blocks

sys.path.insert(0, os.path.join(ORACLE_DIR, "ref"))
import refio  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(c, mode, lay) for c, modes in refio.MODES.items() for mode in modes for lay in ("packed", "soa")
         if not (refio.RHS_CASES[c][0] == "qhh" and lay == "soa")]
IDS = [f"{refio.rhs_name(c, mode)}-{lay}" for c, mode, lay in CASES]
_MODELS = {}


def _model(case, tmp_path_factory):
    prj = refio.RHS_CASES[case][0]
    if prj not in _MODELS:                                # the synthetic project is rewritten here, not recorded
        _MODELS[prj] = refio.load_model(prj, tmp_path_factory.mktemp("syn") if prj == "syn" else None)
    return _MODELS[prj]


@pytest.mark.parametrize("case,mode,layout", CASES, ids=IDS)
def test_device_rhs_vs_recorded_reference(case, mode, layout, monkeypatch, tmp_path_factory):
    from shud_rhs import runtime as rt
    monkeypatch.setenv("SHUD_RHS_PACKED", "1" if layout == "packed" else "0")
    rec = refio.load_recording(refio.rhs_name(case, mode))
    m, y0 = _model(case, tmp_path_factory)
    states = refio.case_states(case, m, y0)
    if "states" in rec:
        assert np.array_equal(np.stack(states), rec["states"])
    assert rec["dy"].shape == (len(states), m.num_y)
    step, bc = refio.step_and_bc(rec)
    g = rt.RhsHandle(m, mode=mode)
    assert g.layout()["packed"] == (layout == "packed"), g.layout()
    g.set_step_inputs(step, bc)
    t = float(rec["t"][0])
    worst_abs = worst_rel = 0.0
    for k, y in enumerate(states):
        got = g.eval(t, y)
        a, r = assert_close(got, rec["dy"][k], what=f"{case} mode {mode} {layout} call {k}", blocks=rhs_blocks(m))
        worst_abs, worst_rel = max(worst_abs, a), max(worst_rel, r)
    print(f"REFPIN {case} mode={mode} {layout}: max |d| {worst_abs:.3e}  max rel {worst_rel:.3e}")
    g.close()
