"""CPU: the oracle pinned to the REFERENCE model's own right-hand side.

oracle/_ref/shud_ref_f and shud_ref_f_omp are the reference's own units (compiled in place from a reference
checkout by `make -C oracle`, with a vector-container stand-in for the SUNDIALS header they include) behind our
driver oracle/ref/shud_ref_driver.cpp.  The driver runs the reference's ET step(s), dumps the step inputs it then
holds, and evaluates the reference's f() on a list of states in one process.  Both restatements (OracleRhs in C,
NumpyRhs) must reproduce every DY bit for bit, in serial and OpenMP semantics, on ccw, qhh (lakes; C oracle
only: the numpy restatement and the OpenMP f have no lake), heihe and a synthetic project with element / river
boundary conditions, at the initial condition, at seeded random states and at a later wet ET step.

Live: where the binaries exist they are run in a child process on the unpacked archives, and the committed
recordings under tests/golden/ref/ must equal that fresh run (a stale recording fails).
Recorded: the same oracle-to-reference equality from the recordings alone; these never skip."""
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ORACLE_DIR

sys.path.insert(0, os.path.join(ORACLE_DIR, "ref"))
import refio  # noqa: E402

CASES = [(c, mode) for c, modes in refio.MODES.items() for mode in modes]
IDS = [refio.rhs_name(c, mode) for c, mode in CASES]


@pytest.fixture(scope="module")
def syn_dir(tmp_path_factory):
    """the synthetic BC project, written once (the files are deterministic)"""
    d = tmp_path_factory.mktemp("syn")
    refio.unpack("syn", d)
    return d


def _model(case, syn_dir):
    prj = refio.RHS_CASES[case][0]
    return refio.load_model(prj, syn_dir)


def _states(case, rec, m, y0):
    states = refio.case_states(case, m, y0)
    if "states" in rec:                                   # the recorded states are the ones the test rebuilds
        assert np.array_equal(np.stack(states), rec["states"])
    return states


def _differing(a, b):
    return int((~((a == b) | (np.isnan(a) & np.isnan(b)))).sum())


def _check_oracles(case, mode, rec, m, y0):
    import numpy_oracle
    import oracle
    states = _states(case, rec, m, y0)
    assert rec["dy"].shape == (len(states), m.num_y)
    step, bc = refio.step_and_bc(rec)
    t = float(rec["t"][0])
    impls = [oracle.OracleRhs] + ([] if m.num_lake else [numpy_oracle.NumpyRhs])
    for cls in impls:
        o = cls(m, mode)
        o.set_step_inputs(step, bc)
        for k, y in enumerate(states):
            r = o.eval(t, y)
            dy, code = (r[0], r[1]) if isinstance(r, tuple) else (r, 0)
            assert code == 0
            n = _differing(dy, rec["dy"][k])
            assert n == 0, f"{case} mode {mode} {cls.__name__} call {k}: {n} of {dy.size} entries differ"
            assert np.array_equal(dy, rec["dy"][k], equal_nan=True)
    # the carried state is real: a repeated state's second call differs from its first in serial mode
    if mode == 0 and case == "ccw_ic":
        assert not np.array_equal(rec["dy"][3], rec["dy"][4])


@pytest.mark.parametrize("case,mode", CASES, ids=IDS)
def test_oracles_equal_recorded_reference(case, mode, syn_dir):
    rec = refio.load_recording(refio.rhs_name(case, mode))
    m, y0 = _model(case, syn_dir)
    assert rec["threads"][0] == 1.0          # the team size the reference process observed, dumped by the driver
    _check_oracles(case, mode, rec, m, y0)


@pytest.mark.parametrize("case,mode", CASES, ids=IDS)
def test_oracles_equal_live_reference(case, mode, syn_dir, tmp_path):
    """a fresh run of the reference binary; passes vacuously (not skipped) on a machine without oracle/_ref/,
    where test_oracles_equal_recorded_reference carries the comparison.  Whether it ran shows in the output:
    a "REFPIN live comparison RAN" line, or a "NOT RUN" warning in pytest's summary."""
    if not refio.live_status(refio.rhs_name(case, mode)):
        return
    work = syn_dir if refio.RHS_CASES[case][0] == "syn" else tmp_path
    live = refio.run_rhs_case(case, mode, work)
    m, y0 = _model(case, syn_dir)
    _check_oracles(case, mode, live, m, y0)
    rec = refio.load_recording(refio.rhs_name(case, mode))
    for k, v in live.items():
        if k in rec:
            assert np.array_equal(rec[k], v, equal_nan=True), f"recording {refio.rhs_name(case, mode)}: {k} is stale"
    assert live["threads"][0] == 1.0 and set(rec) <= set(live)


@pytest.mark.parametrize("prj", ["ccw", "qhh", "heihe"])
def test_y0_fixture_is_the_references_ic(prj):
    """tests/golden/<prj>_y0.npy equals the vector the reference's LoadIC + SetIC2Y builds"""
    case = f"{prj}_ic"
    rec = refio.load_recording(refio.rhs_name(case, 0))
    y0 = np.load(os.path.join(GOLDEN, f"{prj}_y0.npy"))
    assert np.array_equal(y0, rec["y0"])
    assert int(rec["dims"][0]) == y0.size


def test_recordings_within_size_limit():
    for f in os.listdir(refio.REC_DIR):
        assert os.path.getsize(os.path.join(refio.REC_DIR, f)) <= refio.MAX_BYTES, f
