"""GPU: ordered handles (include/shud_order.h).  The device side of an ordered handle runs in a breadth-first element
order; every host pointer stays in the caller's numbering.  An element-only renumbering changes no element's own
operation order and no river sum (test_gpu_renumber.py), so an ordered handle must return the BITS of a
plain one: DY, every diagnostic, the error exit.  The permute kernel is checked on its own at the block edges
(256 threads x 2 elements per lane), the integrator at the bound of the device-vs-CPU trajectory test, and the two
file surfaces (shud_out_add_mapped, shud_mon_set_ic_order) byte for byte.

Models: ccw, heihe, variant(3000, 5) (3024 elements) and variant(20000, 43) (20022): the smallest meshes with
partial last tiles and both boundary kinds; each also under a seeded random permutation as the caller's numbering."""
import glob
import os

import numpy as np
import pytest
import torch

import cases
import renumber as rn
import shud_gpu_run
import test_gpu_share as ts
from conftest import GOLDEN
from print_ctrl_py import PrintCtrlPy
from shud_rhs import abi
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu

MODES = [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP]
OMP_SKIPPED = ("q_es", "q_eu", "q_eg", "q_tu", "q_tg", "q_eta", "i_beta")       # as test_gpu_parity._compare_sequence
BASE = {"ccw": cases.ccw, "heihe": cases.heihe, "v3000": lambda: cases.variant(3000, seed=5),
        "v20000": lambda: cases.variant(20000, seed=43)}
NAMES = [f"{b}{s}" for b in BASE for s in ("", "_rand")]
_models = {}


def model(name):
    """(model, state), built once and never modified; `_rand`: under a seeded random element permutation"""
    if name not in _models:
        base = name[:-5] if name.endswith("_rand") else name
        m, y = BASE[base]()
        if name.endswith("_rand"):
            m, map_y = rn.renumber(m, pe=np.random.default_rng(len(name) + m.num_ele).permutation(m.num_ele))
            y = map_y(y)
        _models[name] = (m, y)
    return _models[name]


@pytest.fixture(params=["packed", "soa"])
def layout(request, monkeypatch):
    monkeypatch.setenv("SHUD_RHS_PACKED", "1" if request.param == "packed" else "0")
    return request.param


def _map_state(y, idx, NE):
    return np.concatenate([y[:NE][idx], y[NE:2 * NE][idx], y[2 * NE:3 * NE][idx], y[3 * NE:]])


# ---------------------------------------------------------------- ordered vs plain, host pointers
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_ordered_handle_same_bits_host(name, mode, layout):
    """RhsHandle(m, order="bfs") against RhsHandle(m): DY of three stateful host-pointer calls and every array of
    sync_diagnostics as uint64.  The handle's order is the planner's, and its layout is that of the applied model."""
    m, y = model(name)
    ys = [y] + cases.states(m, None, 2, seed=71)
    a, b = rt.RhsHandle(m, mode=mode), rt.RhsHandle(m, mode=mode, order="bfs")
    try:
        kind, perm, inv = b.order()
        assert kind == abi.SHUD_ORDER_BFS and np.array_equal(perm, rt.order_plan(m, "bfs"))
        assert np.array_equal(inv[perm], np.arange(m.num_ele)) and (perm != np.arange(m.num_ele)).any()
        ka, pa, ia = a.order()
        assert ka == abi.SHUD_ORDER_IDENTITY and np.array_equal(pa, np.arange(m.num_ele)) and np.array_equal(ia, pa)
        la, lb = a.layout(), b.layout()
        assert la["packed"] == lb["packed"] == (layout == "packed")
        if layout == "packed":
            applied = rt.order_apply(m, perm)
            assert lb.get("shared_edges", 0) == int((rn.share_assignment(applied)[1] >= 0).sum())
            if name.endswith("_rand") or name in ("ccw", "heihe"):
                assert lb["shared_edges"] > la.get("shared_edges", 0)       # the order is worth something
        a.set_step_inputs()
        b.set_step_inputs()
        for c, yy in enumerate(ys):
            ts._same_bits(a.eval(0.0, yy), b.eval(0.0, yy), f"{name} mode {mode} {layout} call {c}")
        da, db = a.diagnostics(), b.diagnostics()
        for k in abi.FLUXOUT_ORDER:
            if mode == abi.SHUD_MODE_OMP and k in OMP_SKIPPED:
                continue
            ts._same_bits(da[k], db[k], f"{name} mode {mode} {layout} diag {k}")
        assert a.num_calls() == b.num_calls() == 3
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("name", ["ccw_rand", "v3000"])
def test_ordered_handle_partial_step_inputs_and_cvrhs(name):
    """set_step_inputs with a subset of the [NE] arrays (the others keep their values) and new carried state between
    calls, then shud_rhs_cvrhs: the same bits as the plain handle"""
    m, y = model(name)
    a, b = rt.RhsHandle(m), rt.RhsHandle(m, order="bfs")
    try:
        for h in (a, b):
            h.set_step_inputs()
        ts._same_bits(a.eval(0.0, y), b.eval(0.0, y), "first")
        rng = np.random.default_rng(5)
        part = dict(net_prep=rng.uniform(0.0, 0.02, m.num_ele), u_satn=rng.uniform(0.0, 1.0, m.num_ele),
                    e_ic=rng.uniform(0.0, 1e-3, m.num_ele))
        out = []
        for h in (a, b):
            h.set_step_inputs(step=part, bc_tables={})
            yd = np.empty_like(y)
            assert rt.lib().shud_rhs_cvrhs(1.0, y.ctypes.data, yd.ctypes.data, h.h) == 0
            out.append(yd)
        ts._same_bits(out[0], out[1], "cvrhs after partial step inputs")
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- device pointers: the internal numbering
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["heihe", "v3000_rand"])
def test_device_pointer_eval_is_internal(name, mode, layout):
    """y carried to the internal numbering by permute(), a device-pointer eval, and DY read back as it is: the plain
    handle's DY gathered through perm, bit for bit; permute() back gives the plain DY itself.  A user-given order does
    the same."""
    m, y = model(name)
    NE = m.num_ele
    a = rt.RhsHandle(m, mode=mode)
    a.set_step_inputs()
    ref = a.eval(0.0, y)
    a.close()
    user = np.random.default_rng(11).permutation(NE).astype(np.int32)
    for order in ("bfs", user):
        b = rt.RhsHandle(m, mode=mode, order=order)
        try:
            b.set_step_inputs()
            kind, perm, inv = b.order()
            if not isinstance(order, str):
                assert kind == abi.SHUD_ORDER_USER and np.array_equal(perm, user)
            d = [b.device_alloc(8 * m.num_y) for _ in range(4)]
            b.h2d(d[0], y)
            b.permute(d[0], d[1], to="internal")
            b.eval_device(0.0, d[1], d[2])
            b.permute(d[2], d[3], to="caller")
            yi, dyi, dyc = (b.d2h(np.empty(m.num_y), p) for p in (d[1], d[2], d[3]))
            ts._same_bits(yi, _map_state(y, perm, NE), "y in the internal numbering")
            ts._same_bits(dyi, _map_state(ref, perm, NE), "DY in the internal numbering")
            ts._same_bits(dyc, ref, "DY carried back")
            for p in d:
                b.device_free(p)
        finally:
            b.close()


def _errors(handles, yy):
    """the full ShudErr of each handle for state yy (message included), cleared afterwards"""
    out = []
    for h in handles:
        try:
            h.eval(0.0, yy)
            out.append(None)
        except rt.ShudRhsError as e:
            out.append(dict(e.err))
            h.clear_error()
    return out


def test_error_exit_of_ordered_handle():
    """ShudErr of an ordered handle is that of the plain handle, field for field: flags, exit code, message and
    first_index, which is the lowest offending element in the CALLER's numbering (a minimum over caller indices, not
    the caller's number of the lowest internal element).
    a. NaN states at a caller element k that is lower than its neighbours (a NaN state also spoils the
       lateral fluxes of the neighbours): first_index of every raised bit is k.  The k chosen sit AFTER one of their
       neighbours in the internal order, so the mapped internal minimum would name that neighbour.
    b. two offending elements whose caller and internal orders disagree: the caller's lower one is named.
    c. test_error_exit_two_kinds: two error kinds at two elements."""
    m, y = model("v3000_rand")
    NE = m.num_ele
    nabr = np.asarray(m.nabr).reshape(3, NE)
    a, b = rt.RhsHandle(m), rt.RhsHandle(m, order="bfs")
    try:
        for h in (a, b):
            h.set_step_inputs()
        _, perm, inv = b.order()
        nb = np.where(nabr >= 0, nabr, NE + 1)
        lowest = (np.arange(NE) < nb.min(0)) & (nabr >= 0).all(0)             # k below all three neighbours
        later = (inv[np.maximum(nabr, 0)] < inv[None, :]).any(0)               # a neighbour comes first internally
        ks = np.nonzero(lowest & later)[0]
        assert ks.size >= 3
        for k in ks[[0, ks.size // 2, -1]]:
            yy = y.copy()
            yy[[k, NE + k, 2 * NE + k]] = np.nan        # surface, unsaturated and groundwater state of k
            ea, eb = _errors((a, b), yy)
            assert ea is not None and ea["exit_code"] != 0 and ea == eb, (k, ea, eb)
            raised = [bit for bit in range(4) if ea["flags"] & (1 << bit)]
            assert raised and all(eb["first_index"][bit] == k for bit in raised), (k, eb)
            ts._same_bits(a.eval(0.0, y), b.eval(0.0, y), f"after the error at {k}")
        # b. pairs far apart in the mesh, caller order against internal order
        rng = np.random.default_rng(3)
        done = 0
        while done < 3:
            k1, k2 = sorted(rng.choice(NE, 2, replace=False))
            if inv[k1] < inv[k2]:
                continue
            yy = y.copy()
            yy[[k1, k2, 2 * NE + k1, 2 * NE + k2]] = np.nan
            ea, eb = _errors((a, b), yy)
            assert ea is not None and ea == eb, (k1, k2, ea, eb)
            done += 1
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kh_first", [False, True])
def test_error_exit_two_kinds(kh_first):
    """two error kinds at two elements: KsatH = 1e12 at element k2 breaks effKH's range there on every call (exit
    code 13), a negative potential evaporation at k1 (a step input, carried through the handle's gather) gives a
    negative ET flux there (exit code 10); shud_rhs_get_error picks code and message by comparing the two first
    indices.  k1 and k2 are in opposite order in the caller's and the internal numbering, in both caller orders: the
    ordered handle's ShudErr is the plain handle's, field for field, and the code is that of the caller's lower one."""
    import copy
    m0, y = model("v3000_rand")
    NE = m0.num_ele
    inv = np.argsort(rt.order_plan(m0, "bfs"))
    rng = np.random.default_rng(8)
    ok = (np.asarray(m0.ibc) == 0) & (np.asarray(m0.par["VegFrac"]) < 1.0)
    while True:
        lo, hi = sorted(int(v) for v in rng.choice(NE, 2, replace=False))
        if inv[lo] > inv[hi] and ok[lo] and ok[hi]:
            break
    k2, k1 = (lo, hi) if kh_first else (hi, lo)
    m = copy.deepcopy(m0)
    m.par["KsatH"] = m.par["KsatH"].copy()
    m.par["KsatH"][k2] = 1e12
    m.finalize()
    a, b = rt.RhsHandle(m), rt.RhsHandle(m, order="bfs")
    try:
        assert np.array_equal(b.order()[2], inv)
        for h in (a, b):
            h.set_step_inputs()
        yy = y.copy()
        yy[2 * NE + k2] = 1.0                           # below the macropore zone: effKH = KsatH
        ea, eb = _errors((a, b), yy)                    # effKH alone
        assert ea is not None and ea["flags"] & abi.EF_EFFKH and ea["exit_code"] == 13 and ea == eb, (ea, eb)
        assert eb["first_index"][1] == k2
        pet = np.asarray(m.step["pot_evap"], dtype=np.float64).copy()
        pet[k1] = -1.0
        for h in (a, b):
            h.set_step_inputs(step=dict(pot_evap=pet), bc_tables={})
        ea, eb = _errors((a, b), yy)
        print("two kinds:", ea)
        assert ea is not None and ea["flags"] & abi.EF_EFFKH and ea["flags"] & abi.EF_ET_NEG, ea
        assert ea == eb, (ea, eb)
        assert eb["first_index"][1] == k2 and eb["first_index"][2] == k1
        assert eb["exit_code"] == (13 if kh_first else 10), eb
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- the permute kernel
def _subset_with_rivers(m, n):
    """elements [0, n) of m with m's whole river network and the segments that lie on kept elements"""
    r = cases._subset(m, np.arange(n))
    keep = np.nonzero(np.asarray(m.seg_ele) < n)[0]
    r.num_riv, r.num_seg = m.num_riv, keep.size
    r.riv = {k: v.copy() for k, v in m.riv.items()}
    r.riv_down, r.riv_bc = m.riv_down.copy(), m.riv_bc.copy()
    r.seg_ele, r.seg_riv = m.seg_ele[keep].copy(), m.seg_riv[keep].copy()
    r.seg_length, r.seg_cwr = m.seg_length[keep].copy(), m.seg_cwr[keep].copy()
    r.bc_tables = dict(m.bc_tables)
    return r.finalize()


def _bit_patterns(n, rng):
    """doubles whose bits matter: random words (NaN payloads among them), signed zeros, infinities, quiet and
    signalling-range NaNs with payloads"""
    u = rng.integers(0, 2 ** 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    special = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                        0x7FF8000000000001, 0xFFF8DEADBEEF0001, 0x7FF0000000000001, 0x0000000000000001], dtype=np.uint64)
    k = min(n, special.size)
    u[rng.choice(n, k, replace=False)] = special[:k]
    return u.view(np.float64)


@pytest.mark.parametrize("reaches", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_permute_known_answer(n, reaches):
    """shud_rhs_permute on handles of n elements with a user order, with and without reaches: state vectors, [NE] and
    [3*NE] arrays against numpy fancy indexing byte for byte (signed zeros and NaN payloads kept), the round trip the
    identity, the reach tail copied; on a plain handle every form is a copy.  n = 255 / 256 / 257 straddle the
    2-element lanes of a wave and an odd n puts the second and third block on an odd double (the 8-byte store path);
    3000 takes several blocks."""
    m0, _ = model("v3000")
    m = _subset_with_rivers(m0, n) if reaches else cases._subset(m0, np.arange(n))
    NE, NY = m.num_ele, m.num_y
    assert NE == n and (m.num_riv > 0) == reaches
    rng = np.random.default_rng(100 + n)
    user = rng.permutation(n).astype(np.int32)
    sizes = {"state": NY, "ele": NE, "ele3": 3 * NE}
    for order in (user, None):
        h = rt.RhsHandle(m, order=order)
        try:
            kind, perm, inv = h.order()
            assert np.array_equal(perm, user if order is not None else np.arange(n))
            d = [h.device_alloc(8 * (NY + 2)) for _ in range(3)]
            for what, size in sizes.items():
                src = _bit_patterns(size, rng)
                guard = np.full(NY + 2, -7.25)
                planes = 1 if what == "ele" else 3
                for to, idx in (("internal", perm), ("caller", inv)):
                    h.h2d(d[0], src)
                    h.h2d(d[1], guard)
                    h.permute(d[0], d[1], to=to, what=what)
                    got = h.d2h(np.empty(NY + 2), d[1])
                    want = np.concatenate([src[:planes * NE].reshape(planes, NE)[:, idx].reshape(-1), src[planes * NE:]])
                    assert got[:size].tobytes() == want.tobytes(), (what, to, n)
                    assert (got[size:] == -7.25).all(), (what, to, "wrote past the vector")
                    h.permute(d[1], d[2], to="caller" if to == "internal" else "internal", what=what)
                    assert h.d2h(np.empty(size), d[2]).tobytes() == src.tobytes(), (what, to, "round trip")
            for p in d:
                h.device_free(p)
        finally:
            h.close()


# ---------------------------------------------------------------- the integrator
def _ccw_run(order, nsteps=6):
    m, y0 = cases.ccw()
    h = rt.RhsHandle(m, order=order)
    h.set_step_inputs()
    # ccw.cfg.para, as test_gpu_ode.test_shud_ccw_integration_vs_oracle
    d = rt.OdeSolver(h, 0.0, y0, 1e-4, 1e-4, 1.0, 10.0, 1e-6, 1000000)
    ys = []
    for k in range(1, nsteps + 1):
        f, t, y = d.solve(10.0 * k)
        assert f == 0 and t == 10.0 * k
        ys.append(y)
    st = d.stats()
    flag, dky = d.get_dky(10.0 * nsteps, 1)
    assert flag == 0
    d.close()
    h.close()
    return ys, st, dky


def test_integrator_identity_and_bfs():
    """the ccw run of tests/test_gpu_ode.py.  order="identity": y, dky and ShudOdeStats bit-identical to a plain
    handle.  order="bfs": the integrator's vectors are in the internal numbering, which changes the order of its norm
    reductions, so y (returned in the caller's numbering) is compared with the plain run at the first-hour bound of
    the device-vs-CPU trajectory test (tests/traj.py `werr`, tests/test_gpu_ode.py::test_ccw_one_day_trajectory and
    _close_traj): |dy| <= 1e-6 (rtol |y| + atol) per state, rtol = atol = 1e-4."""
    plain, st0, dk0 = _ccw_run(None)
    ident, st1, dk1 = _ccw_run("identity")
    for a, b in zip(plain, ident):
        ts._same_bits(a, b, "identity order")
    ts._same_bits(dk0, dk1, "identity dky")
    assert st0 == st1, (st0, st1)
    bfs, st2, dk2 = _ccw_run("bfs")
    for k, (a, b) in enumerate(zip(plain, bfs)):
        werr = float(np.max(np.abs(a - b) / (1e-4 * np.abs(a) + 1e-4)))
        print(f"step {k}: weighted difference {werr:.3e}")
        assert werr <= 1e-6, (k, werr)


def test_solver_run_on_ordered_handle():
    """ShudSolver over RhsHandle(order="bfs") with the device ET prelude: on_output's y is in the caller's numbering
    (first-hour trajectory bound against the plain run, as above) and so are the ET prelude's host arrays"""
    from shud_rhs import et
    from shud_rhs.solver import ShudSolver, SolverControl
    m, y0 = model("v3000")
    etm = et.synth_et(m.num_ele, seed=6, terrain=True, lake_frac=0.0)
    ctl = SolverControl(reltol=1e-4, abstol=1e-4, init_step=0.5, max_step=20.0, et_step=10.0)

    def forcing(t, tout):
        return et.synth_forcing(t, tout - t, seed=int(t) + 1, tsr_mode=abi.SHUD_TSR_RECOMPUTE)

    runs = {}
    for order in (None, "bfs"):
        h = rt.RhsHandle(m, order=order)
        h.set_step_inputs()
        h.et_attach(etm)
        sol = ShudSolver(h, y0, ctl)
        outs = []
        sol.run(2, forcing=forcing, on_output=lambda i, t, y: outs.append(y.copy()))
        runs[order] = (outs, h.et_get())
        sol.close()
        h.close()
    for a, b in zip(*(runs[o][0] for o in (None, "bfs"))):
        assert float(np.max(np.abs(a - b) / (1e-4 * np.abs(a) + 1e-4))) <= 1e-6
    for k in ("qEleNetPrep", "qPotEvap", "qPotTran", "t_lai", "rn_factor"):         # ET prelude: per element, exact
        ts._same_bits(runs[None][1][k], runs["bfs"][1][k], f"ET {k}")


def test_water_balance_refused_on_ordered_handle():
    """shud_wb_create on an ordered handle: SHUD_ERR_UNSUPPORTED (its basin sums would run in another order)"""
    m, _ = model("ccw")
    h = rt.RhsHandle(m, order="bfs")
    try:
        with pytest.raises(rt.ShudRhsError) as e:
            rt.WaterBalance(h, 60)
        assert e.value.code == abi.SHUD_ERR_UNSUPPORTED
    finally:
        h.close()


# ---------------------------------------------------------------- files stay in the caller's numbering
@pytest.mark.parametrize("n", [257, 3000])
def test_out_add_mapped(tmp_path, n):
    """shud_out_add_mapped: source arange(n) (scaled per export), a seeded column map and a flag_io mask; the .dat and
    .csv bytes are those of the Print_Ctrl restatement fed the caller-order values src[col_src]"""
    rng = np.random.default_rng(n)
    col_src = rng.permutation(n).astype(np.int32)
    col_src[rng.choice(n, 5, replace=False)] = rng.integers(0, n, 5)         # a map, not only a permutation
    flags = (rng.random(n) < 0.6).astype(np.int32)
    src = torch.zeros(n, dtype=torch.float64, device="cuda")
    out = rt.Output(stream=torch.cuda.current_stream().cuda_stream or None)
    refs = []
    for k, fl in enumerate((flags, None)):
        out.add(tmp_path / f"dev{k}", src.data_ptr(), n, 60, k, flag_io=fl, ascii=True, col_src=col_src)
        refs.append(PrintCtrlPy(tmp_path / f"ref{k}", n, 60, k, flag_io=fl, ascii=True))
    for step in range(1, 7):
        host = np.arange(n, dtype=np.float64) * (1.0 + 0.125 * step)
        src.copy_(torch.from_numpy(host))
        torch.cuda.current_stream().synchronize()
        out.export(30.0 * step)
        for p in refs:
            p.print_data(host[col_src], 30.0 * step)
    assert [out.rows(k) for k in range(2)] == [3, 3]
    out.close()
    for k, p in enumerate(refs):
        p.close()
        assert open(tmp_path / f"dev{k}.dat", "rb").read() == open(tmp_path / f"ref{k}.dat", "rb").read(), k
        assert open(tmp_path / f"dev{k}.csv").read() == open(tmp_path / f"ref{k}.csv").read(), k
    with pytest.raises(rt.ShudRhsError):
        bad = col_src.copy()
        bad[3] = n
        rt.Output().add(tmp_path / "bad", src.data_ptr(), n, 60, 0, col_src=bad)


@pytest.mark.parametrize("ne", [1, 255, 257, 1025])
def test_ic_snapshot_in_caller_order(tmp_path, ne):
    """shud_mon_set_ic_order: the device arrays hold the internal numbering (caller arrays gathered through perm);
    the snapshot file is byte-identical to shud_mon_write_ic_host on the caller-order arrays"""
    rng = np.random.default_rng(ne)
    nr = 65
    perm = rng.permutation(ne).astype(np.int32)
    cols = [rng.normal(0.0, s, ne) for s in (1e-3, 0.05, 0.01, 6.0, 1e6)]
    riv = rng.uniform(0.0, 2.0, nr)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    d_cols, d_riv = [dev(c[perm]) for c in cols], dev(riv)
    mon = rt.RunMonitors(stream=torch.cuda.current_stream().cuda_stream or None)
    fn, ref = tmp_path / "syn.cfg.ic.update", tmp_path / "ref.cfg.ic"
    mon.add_ic(fn, 720, *d_cols, d_riv, None, ne, nr, 0)
    with pytest.raises(rt.ShudRhsError):
        mon.set_ic_order(np.full(ne, ne, dtype=np.int32))                 # not a permutation
    mon.set_ic_order(perm)
    assert mon.ic_update(1440.0) is True
    mon.flush()
    rt.write_ic_host(ref, 1440.0, *cols, riv)
    assert open(fn, "rb").read() == open(ref, "rb").read()
    mon.close()


# ---------------------------------------------------------------- shud_gpu --reorder bfs
def _ccw_project(root):
    """the ccw example project unpacked under root, its output intervals set to 60 minutes (the shipped 1440 would
    leave a run of a few hours without rows)"""
    import re
    import zipfile
    with zipfile.ZipFile(os.path.join(GOLDEN, "input", "ccw.zip")) as z:
        z.extractall(root)
    cfg = os.path.join(root, "input", "ccw", "ccw.cfg.para")
    txt = re.sub(r"^(DT_\w+)\s+\d+", r"\1\t60", open(cfg).read(), flags=re.M)
    open(cfg, "w").write(txt)
    return os.path.join(root, "input", "ccw")


def _run_shud_gpu(root, src, outdir, extra, env=None):
    return shud_gpu_run.run(["-q", "-o", outdir, "-C", root, "-e", "0.125", "--ic-snapshots"] + extra + [src, "ccw"],
                            env=env, check=False)


def test_shud_gpu_reorder(tmp_path):
    """shud_gpu --reorder bfs on ccw over three hours against the run without the flag: the same files, .dat headers
    (the 1024-byte text, StartTime, NumVar and the column numbers) and ccw.cfg.ic.bak byte-identical, the rows in the
    input's element numbering.  Values: the integrator's reductions run in another order, so the first hour's rows
    are compared at the first-hour bound of the device-vs-CPU trajectory test (tests/traj.py `werr` <= 1e-6 of the
    error weight rtol |v| + atol, rtol = atol = 1e-4) and the later rows at that test's bound for the rest of the day,
    twice the serial envelope of profiles/r04/traj/spread.json (2 x 13.1).  With SHUD_WB_DIAG=1 the flag is refused."""
    from shud_rhs import shudio
    root = str(tmp_path / "ref")
    src = _ccw_project(root)
    a, b = tmp_path / "plain", tmp_path / "bfs"
    ra = _run_shud_gpu(root, src, a, [])
    rb = _run_shud_gpu(root, src, b, ["--reorder", "bfs"])
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout + ra.stderr + rb.stdout + rb.stderr
    files = sorted(os.path.basename(f) for f in glob.glob(str(a / "*.dat")))
    assert len(files) >= 15 and files == sorted(os.path.basename(f) for f in glob.glob(str(b / "*.dat")))
    assert open(a / "ccw.cfg.ic.bak", "rb").read() == open(b / "ccw.cfg.ic.bak", "rb").read()
    worst = (0.0, "")
    for f in files:
        da, db = shudio.read_dat(str(a / f)), shudio.read_dat(str(b / f))
        nvar = da["data"].shape[1]
        nhead = 1024 + 16 + 8 * nvar
        assert open(a / f, "rb").read()[:nhead] == open(b / f, "rb").read()[:nhead], f
        assert da["data"].shape == db["data"].shape == (3, nvar) and np.array_equal(da["t"], db["t"]), f
        w = np.abs(da["data"] - db["data"]) / (1e-4 * np.abs(da["data"]) + 1e-4)
        worst = max(worst, (float(w.max()), f))
        print(f"{f}: weighted difference first hour {w[0].max():.3e}, later {w[1:].max():.3e}")
        assert w[0].max() <= 1e-6, (f, float(w[0].max()))
        assert w.max() <= 2.0 * 13.1, (f, float(w.max()))
    print("worst", worst)
    # the end-of-run restart file lists the elements in the input's numbering too
    ua = np.array(open(a / "ccw.cfg.ic.update").read().split()[9:9 + 6 * 1147], dtype=np.float64)
    ub = np.array(open(b / "ccw.cfg.ic.update").read().split()[9:9 + 6 * 1147], dtype=np.float64)
    # the same day bound on the printed values, plus the last printed digit
    assert ua.size == ub.size == 6 * 1147
    assert np.all(np.abs(ua - ub) <= 2.0 * 13.1 * (1e-4 * np.abs(ua) + 1e-4) + 1e-6)
    rw = _run_shud_gpu(root, src, tmp_path / "wb", ["--reorder", "bfs"], env={"SHUD_WB_DIAG": "1"})
    assert rw.returncode != 0 and "--reorder cannot be combined with SHUD_WB_DIAG" in rw.stderr
    assert not os.path.exists(tmp_path / "wb")
