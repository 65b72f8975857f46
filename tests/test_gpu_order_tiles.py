"""GPU: handles ordered by SHUD_ORDER_TILES (include/shud_order.h), the order that grows each 256-element sharing tile
breadth-first.  Everything an ordered handle promises holds for it as for the breadth-first order (test_gpu_order.py,
whose helpers are used here): the BITS of a plain handle on every host pointer (DY, every diagnostic, the error exit),
device pointers in the internal numbering, the integrator at the first-hour trajectory bound, and shud_gpu's files in
the input's numbering.  The kernels are the plain handle's; only the numbering they are fed differs.

Models: ccw, heihe, variant(3000, 5) (3024 elements, a partial last tile) also under a seeded random permutation,
ccw without rivers, one triangle (the plan is the identity), and variant(300, 5) (306 elements: one full tile and a
partial one)."""
import glob
import os

import numpy as np
import pytest

import cases
import renumber as rn
import shud_gpu_run
import test_gpu_order as tgo
import test_gpu_share as ts
from shud_rhs import abi
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu

MODES = [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP]
EXTRA = {"riverless": cases.riverless, "single": cases.single_element, "v300": lambda: cases.variant(300, seed=5)}
NAMES = ["ccw", "heihe", "v3000", "v3000_rand", "riverless", "single", "v300"]
_models = {}


def model(name):
    """(model, state), built once and never modified"""
    if name not in EXTRA:
        return tgo.model(name)
    if name not in _models:
        _models[name] = EXTRA[name]()
    return _models[name]


@pytest.fixture(params=["packed", "soa"])
def layout(request, monkeypatch):
    monkeypatch.setenv("SHUD_RHS_PACKED", "1" if request.param == "packed" else "0")
    return request.param


# ---------------------------------------------------------------- ordered vs plain, host pointers
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", NAMES)
def test_tiles_handle_same_bits_host(name, mode, layout):
    """RhsHandle(m, order="tiles") against RhsHandle(m): DY of three stateful host-pointer calls and every array of
    sync_diagnostics as uint64.  shud_rhs_order reports kind 3 and the planner's perm and its inverse; the layout is
    that of the applied model."""
    m, y = model(name)
    NE = m.num_ele
    assert name != "v300" or (NE > 256 and NE % 256 != 0)
    ys = [y] + cases.states(m, None, 2, seed=71)
    a, b = rt.RhsHandle(m, mode=mode), rt.RhsHandle(m, mode=mode, order="tiles")
    try:
        kind, perm, inv = b.order()
        assert kind == abi.SHUD_ORDER_TILES == 3 and np.array_equal(perm, rt.order_plan(m, "tiles"))
        assert np.array_equal(inv[perm], np.arange(NE))
        assert b.ordered == (NE > 1) == bool((perm != np.arange(NE)).any())
        la, lb = a.layout(), b.layout()
        assert la["packed"] == lb["packed"]
        if lb["packed"]:
            applied = rt.order_apply(m, perm)
            assert lb.get("shared_edges", 0) == int((rn.share_assignment(applied)[1] >= 0).sum())
            if name in ("ccw", "heihe", "v3000_rand"):
                assert lb["shared_edges"] > la.get("shared_edges", 0)       # the order is worth something
        a.set_step_inputs()
        b.set_step_inputs()
        for c, yy in enumerate(ys):
            ts._same_bits(a.eval(0.0, yy), b.eval(0.0, yy), f"{name} mode {mode} {layout} call {c}")
        da, db = a.diagnostics(), b.diagnostics()
        for k in abi.FLUXOUT_ORDER:
            if mode == abi.SHUD_MODE_OMP and k in tgo.OMP_SKIPPED:
                continue
            ts._same_bits(da[k], db[k], f"{name} mode {mode} {layout} diag {k}")
        assert a.num_calls() == b.num_calls() == 3
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- device pointers: the internal numbering
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["heihe", "v3000_rand", "v300"])
def test_tiles_device_pointer_eval_is_internal(name, mode, layout):
    """y carried to the internal numbering by permute(), a device-pointer eval, and DY read back as it is: the plain
    handle's host DY gathered through perm, bit for bit; permute() back gives the host DY itself"""
    m, y = model(name)
    NE = m.num_ele
    a = rt.RhsHandle(m, mode=mode)
    a.set_step_inputs()
    ref = a.eval(0.0, y)
    a.close()
    b = rt.RhsHandle(m, mode=mode, order="tiles")
    try:
        b.set_step_inputs()
        kind, perm, inv = b.order()
        assert kind == abi.SHUD_ORDER_TILES
        d = [b.device_alloc(8 * m.num_y) for _ in range(4)]
        b.h2d(d[0], y)
        b.permute(d[0], d[1], to="internal")
        b.eval_device(0.0, d[1], d[2])
        b.permute(d[2], d[3], to="caller")
        yi, dyi, dyc = (b.d2h(np.empty(m.num_y), p) for p in (d[1], d[2], d[3]))
        ts._same_bits(yi, tgo._map_state(y, perm, NE), "y in the internal numbering")
        ts._same_bits(dyi, tgo._map_state(ref, perm, NE), "DY in the internal numbering")
        ts._same_bits(dyc, ref, "DY carried back")
        for p in d:
            b.device_free(p)
    finally:
        b.close()


# ---------------------------------------------------------------- the error exit
def test_error_exit_of_tiles_handle():
    """two offending elements (NaN surface and groundwater states) whose order differs between the caller's and the
    internal numbering, as test_gpu_order.test_error_exit_of_ordered_handle part b: ShudErr of the handle ordered by
    tiles is the plain handle's field for field (flags, first_index in the CALLER's numbering, exit code, message)"""
    m, y = model("v3000_rand")
    NE = m.num_ele
    a, b = rt.RhsHandle(m), rt.RhsHandle(m, order="tiles")
    try:
        for h in (a, b):
            h.set_step_inputs()
        _, perm, inv = b.order()
        rng = np.random.default_rng(3)
        done = 0
        while done < 3:
            k1, k2 = sorted(rng.choice(NE, 2, replace=False))
            if inv[k1] < inv[k2]:
                continue
            yy = y.copy()
            yy[[k1, k2, 2 * NE + k1, 2 * NE + k2]] = np.nan
            ea, eb = tgo._errors((a, b), yy)
            assert ea is not None and ea["exit_code"] != 0 and ea["message"], ea
            assert ea == eb, (k1, k2, ea, eb)
            done += 1
        ts._same_bits(a.eval(0.0, y), b.eval(0.0, y), "after the errors")
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- the count on the device
def test_tiles_shared_edges_on_device():
    """variant(20000, 43) under the default_rng(43) permutation: the tiles handle shares what the CPU plan of the
    applied model counts (test_order_tiles.py puts a floor of 0.85 NE under it), and more than the bfs handle"""
    m, _ = cases.variant(20000, seed=43)
    m2, _ = rn.renumber(m, pe=np.random.default_rng(43).permutation(m.num_ele))
    t, f = rt.RhsHandle(m2, order="tiles"), rt.RhsHandle(m2, order="bfs")
    try:
        nt, nf = t.layout()["shared_edges"], f.layout()["shared_edges"]
        cpu = rt.plan_layout(rt.order_apply(m2, rt.order_plan(m2, "tiles")))["shared_edges"]
        print(f"NE {m2.num_ele}: shared edges tiles {nt}, bfs {nf}, CPU plan {cpu}")
        assert nt == cpu
        assert nt > nf
    finally:
        t.close()
        f.close()


# ---------------------------------------------------------------- the integrator
def test_integrator_under_tiles():
    """the ccw run of test_gpu_order.test_integrator_identity_and_bfs under order="tiles": the integrator's norms run
    in another element order, so y (in the caller's numbering) is held to the plain run at the first-hour bound of the
    device-vs-CPU trajectory test: |dy| <= 1e-6 (rtol |y| + atol) per state, rtol = atol = 1e-4"""
    plain, _, _ = tgo._ccw_run(None)
    tiles, _, _ = tgo._ccw_run("tiles")
    for k, (a, b) in enumerate(zip(plain, tiles)):
        werr = float(np.max(np.abs(a - b) / (1e-4 * np.abs(a) + 1e-4)))
        print(f"step {k}: weighted difference {werr:.3e}")
        assert werr <= 1e-6, (k, werr)


# ---------------------------------------------------------------- shud_gpu --reorder tiles
def test_shud_gpu_reorder_tiles(tmp_path):
    """shud_gpu --reorder tiles on ccw over three hours against the run without the flag, checked as
    test_gpu_order.test_shud_gpu_reorder checks --reorder bfs: the same files, .dat headers and ccw.cfg.ic.bak
    byte-identical, rows in the input's numbering at the first-hour bound (1e-6 of rtol |v| + atol) and, later, at
    twice the serial envelope (2 x 13.1).  An unknown order exits non-zero and names the accepted ones."""
    from shud_rhs import shudio
    root = str(tmp_path / "ref")
    src = tgo._ccw_project(root)
    a, b = tmp_path / "plain", tmp_path / "tiles"

    def run(outdir, extra, env=None):
        return shud_gpu_run.run(["-q", "-o", outdir, "-C", root, "-e", "0.125", "--ic-snapshots"] + extra +
                                [src, "ccw"], env=env, check=False)
    ra = run(a, [])
    rb = run(b, ["--reorder", "tiles"])
    assert ra.returncode == 0 and rb.returncode == 0, ra.stdout + ra.stderr + rb.stdout + rb.stderr
    files = sorted(os.path.basename(f) for f in glob.glob(str(a / "*.dat")))
    assert len(files) >= 15 and files == sorted(os.path.basename(f) for f in glob.glob(str(b / "*.dat")))
    assert open(a / "ccw.cfg.ic.bak", "rb").read() == open(b / "ccw.cfg.ic.bak", "rb").read()
    for f in files:
        da, db = shudio.read_dat(str(a / f)), shudio.read_dat(str(b / f))
        nvar = da["data"].shape[1]
        nhead = 1024 + 16 + 8 * nvar
        assert open(a / f, "rb").read()[:nhead] == open(b / f, "rb").read()[:nhead], f
        assert da["data"].shape == db["data"].shape == (3, nvar) and np.array_equal(da["t"], db["t"]), f
        w = np.abs(da["data"] - db["data"]) / (1e-4 * np.abs(da["data"]) + 1e-4)
        print(f"{f}: weighted difference first hour {w[0].max():.3e}, later {w[1:].max():.3e}")
        assert w[0].max() <= 1e-6, (f, float(w[0].max()))
        assert w.max() <= 2.0 * 13.1, (f, float(w.max()))
    ua = np.array(open(a / "ccw.cfg.ic.update").read().split()[9:9 + 6 * 1147], dtype=np.float64)
    ub = np.array(open(b / "ccw.cfg.ic.update").read().split()[9:9 + 6 * 1147], dtype=np.float64)
    assert ua.size == ub.size == 6 * 1147
    assert np.all(np.abs(ua - ub) <= 2.0 * 13.1 * (1e-4 * np.abs(ua) + 1e-4) + 1e-6)
    rn_ = run(tmp_path / "bad", ["--reorder", "nonsense"])
    assert rn_.returncode != 0 and "bfs" in rn_.stderr and "tiles" in rn_.stderr and "nonsense" in rn_.stderr
    assert not os.path.exists(tmp_path / "bad")
    rw = run(tmp_path / "wb", ["--reorder", "tiles"], env={"SHUD_WB_DIAG": "1"})
    assert rw.returncode != 0 and "--reorder cannot be combined with SHUD_WB_DIAG" in rw.stderr
