"""CPU: the oracle itself (no GPU).  Beside the comparison with the reference's own f() (tests/test_ref_pin.py),
which covers the reference's projects, the C restatement is pinned on every other mesh by (1) an independent numpy restatement that
must agree bit for bit, (2) identities the reference's algorithm guarantees (antisymmetric lateral
fluxes, conservative segment/junction exchange, statefulness pattern), (3) reference error exits."""
import numpy as np
import pytest

import cases
from shud_rhs import abi, workload


def _pair(m, mode):
    import numpy_oracle
    import oracle
    o = oracle.OracleRhs(m, mode)
    n = numpy_oracle.NumpyRhs(m, mode)
    o.set_step_inputs()
    n.set_step_inputs()
    return o, n


def _bit_equal(a, b):
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("case", ["ccw", "heihe", "variant", "riverless", "single_element"])
@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
def test_two_restatements_bit_identical(case, mode):
    m, y = getattr(cases, case)()
    o, n = _pair(m, mode)
    ys = [y] + cases.states(m, None, 2, seed=31)
    for yy in ys:
        for call in range(3):
            a, code, _, _ = o.eval(0.0, yy)
            assert code == 0
            b = n.eval(0.0, yy)
            assert _bit_equal(a, b), f"{case} mode {mode} call {call}"
    d = o.diagnostics()
    for k, v in n.diag.items():
        assert _bit_equal(v, d[k]), k


def test_thread_count_invariance():
    import oracle
    m, y = cases.variant(4000, seed=8)
    res = []
    for th in [1, 3, 8]:
        oracle.set_threads(th)
        o = oracle.OracleRhs(m, 0)
        o.set_step_inputs()
        res.append([o.eval(0.0, y)[0] for _ in range(2)])
    oracle.set_threads(0)
    for r in res[1:]:
        for a, b in zip(res[0], r):
            assert _bit_equal(a, b)


def test_serial_rhs_is_stateful_omp_is_not():
    """f_etFlux mutates qEleE_IC and reads the previous call's u_satn."""
    import oracle
    m, y0 = cases.ccw()
    y = workload.random_state(m, seed=4)
    o = oracle.OracleRhs(m, 0)
    o.set_step_inputs()
    d1, d2, d3 = (o.eval(0.0, y)[0] for _ in range(3))
    NE = m.num_ele
    assert not np.array_equal(d1[NE:2 * NE], d2[NE:2 * NE])     # DY_us changes between calls 1 and 2
    assert np.array_equal(d2, d3)                                # then settles at identical y
    p = oracle.OracleRhs(m, 1)
    p.set_step_inputs()
    e1, e2 = p.eval(0.0, y)[0], p.eval(0.0, y)[0]
    assert np.array_equal(e1, e2)


def test_lateral_fluxes_antisymmetric():
    """Q_ij = -Q_ji exactly for interior edges (fu_Sub = 1): MD_ElementFlux.cpp:54-80,122-138."""
    import oracle
    m, y0 = cases.heihe()
    m.step["fu_sub"] = np.ones(m.num_ele)
    o = oracle.OracleRhs(m, 0)
    o.set_step_inputs()
    o.eval(0.0, workload.random_state(m, seed=6))
    d = o.diagnostics()
    NE = m.num_ele
    nab = m.nabr.reshape(3, NE)
    qs, qg = d["qele_surf"].reshape(3, NE), d["qele_sub"].reshape(3, NE)
    n_checked = 0
    for j in range(3):
        for i in np.nonzero(nab[j] >= 0)[0]:
            k = nab[j, i]
            jj = int(np.nonzero(nab[:, k] == i)[0][0])
            assert qs[j, i] == -qs[jj, k]
            assert qg[j, i] == -qg[jj, k]
            n_checked += 1
    assert n_checked > 3 * NE // 2


def test_exchange_conservation():
    """PassValue (MD_f.cpp:217-257): segment exchange and junction sums conserve volume."""
    import oracle
    m, _ = cases.variant(6000, seed=12)
    o = oracle.OracleRhs(m, 0)
    o.set_step_inputs()
    o.eval(0.0, workload.random_state(m, seed=2))
    d = o.diagnostics()
    tot = np.abs(d["qseg_surf"]).sum() + np.abs(d["qseg_sub"]).sum()
    assert abs(d["qe2r_surf"].sum() + d["qriv_surf"].sum()) <= 1e-12 * tot
    assert abs(d["qe2r_sub"].sum() + d["qriv_sub"].sum()) <= 1e-12 * tot
    has = m.riv_down >= 0
    assert abs(d["qriv_up"].sum() + d["qriv_down"][has].sum()) <= 1e-12 * np.abs(d["qriv_down"]).sum()


def test_serial_vs_omp_documented_differences():
    """OMP skips f_etFlux and uses flux / u_TopArea for the river DY."""
    import oracle
    m, y0 = cases.ccw()
    y = workload.random_state(m, seed=8)
    s, p = oracle.OracleRhs(m, 0), oracle.OracleRhs(m, 1)
    s.set_step_inputs(); p.set_step_inputs()
    ds, dp = s.eval(0.0, y)[0], p.eval(0.0, y)[0]
    NE = m.num_ele
    assert not np.array_equal(ds[:NE], dp[:NE])
    dg = p.diagnostics()
    assert np.all(dg["q_es"] == 0.0) and np.all(dg["q_tu"] == 0.0)


@pytest.mark.parametrize("kind,code", [("et_negative", 10), ("effkh", 13), ("nan", 10)])
def test_reference_exit_codes(kind, code):
    import oracle
    m, y0 = cases.ccw()
    y = y0.copy()
    if kind == "et_negative":
        m.step["pot_evap"][[700, 300]] = -1e-3
        m.step["lai"][:] = 0.0
        y[[300, 700]] = 0.01
        want = 300
    elif kind == "effkh":
        m.par["macKsatH"][[900, 400]] = 1e15
        for i in (900, 400):
            y[2 * m.num_ele + i] = m.par["aquifer_depth"][i] - 0.5 * m.par["macD"][i]
        want = 400
    else:
        y[2 * m.num_ele + 500] = np.nan
        want = int(min(500, *[k for k in m.nabr.reshape(3, -1)[:, 500] if k >= 0]))
    o = oracle.OracleRhs(m, 0)
    o.set_step_inputs()
    _, got, idx, _ = o.eval(0.0, y)
    assert got == code and idx == want


def test_reader_ccw_heihe_shapes():
    from conftest import load_fixture
    for name, (ne, nr, ns) in [("ccw", (1147, 103, 567)), ("heihe", (1779, 723, 1309))]:
        m, y0 = load_fixture(name)
        assert (m.num_ele, m.num_riv, m.num_seg) == (ne, nr, ns)
        assert y0.size == 3 * ne + nr
        assert np.all(m.ele["area"] > 0)
        nab = m.nabr.reshape(3, ne)
        for j in range(3):                      # neighbour relation is symmetric
            for i in np.nonzero(nab[j] >= 0)[0][:200]:
                assert i in nab[:, nab[j, i]]
