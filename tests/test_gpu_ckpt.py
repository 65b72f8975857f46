"""GPU: exact checkpoint / resume of a device run (include/shud_ckpt.h).

The yardstick is always an uninterrupted run: the CPU oracle's for the published problems (the comparison
tests/test_gpu_ode.py makes for the uninterrupted device run), the same build's uninterrupted run for the SHUD loop
(whose behaviour a checkpoint must not change).  Everything is compared bit for bit / byte for byte: the state after
every solver step, shud_rhs_num_calls, every field of the integrator's stats (n_sync included in the SHUD loop) and
every output file."""
import ctypes as C
import glob
import os
import re
import shutil
import zipfile

import numpy as np
import pytest

import oracle
import shud_gpu_run
from conftest import GOLDEN
import cases
from shud_rhs import abi, driver, partition, synth
from shud_rhs import runtime as rt
from test_gpu_ode import COUNTERS, _dev, device_order, kat  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
INTERVALS = (20, 30)                 # output intervals [min]: with 10-minute solver steps 30 does not divide 40 or 10


# ---------------------------------------------------------------- published problems against the oracle
@pytest.mark.parametrize("problem,n,rtol,atol,h0,touts", [
    ("robertson", 3, 1e-6, 1e-12, 1e-6, [0.4, 4.0, 40.0, 400.0, 4e3, 4e4, 4e5]),
    ("decay", 3, 1e-8, 1e-12, 1e-4, [0.1, 1.0, 5.0]),
    ("decayn", 7 * 300 + 37, 1e-6, 1e-10, 1e-5, [0.01, 1.0, 10.0]),
])
def test_split_equals_oracle_straight(kat, device_order, tmp_path, problem, n, rtol, atol, h0, touts):
    """integrate to the touts of tests/test_gpu_ode.py; snapshot after the third (the last but one where there are
    three), destroy the integrator, create a new one, restore, finish: every output and every counter but n_sync
    equals the oracle's uninterrupted run"""
    y0 = np.array([1.0, 0.0, 0.0]) if problem == "robertson" else 1.0 + 0.5 * np.sin(np.arange(n))
    split = min(3, len(touts) - 1)
    u, fn = _dev(kat, problem, n)
    o = oracle.OracleOde(problem, 0.0, y0, rtol, atol, h0, 0.0, 0.0)
    d = rt.OdeSolver(None, 0.0, y0, rtol, atol, h0, 0.0, 0.0, fn=fn)
    ck = rt.Checkpoint(stream=fn[2])
    path = tmp_path / "ode.ckpt"
    for k, tout in enumerate(touts):
        if k == split:
            ck.snapshot(path, touts[k - 1], k, d)
            ck.flush()
            d.close()
            d = rt.OdeSolver(None, 0.0, np.zeros(n), rtol, atol, h0, 0.0, 0.0, fn=fn)
            assert rt.Checkpoint.restore(path, d) == (touts[k - 1], k)
        fd, td, yd = d.solve(tout)
        fo, to, yo = o.solve(tout)
        assert fd == fo == 0 and td == to == tout
        assert np.array_equal(yd, yo), (tout, np.abs(yd - yo).max())
    sd, so = d.stats(), o.stats()
    for key in COUNTERS:
        assert sd[key] == so[key], (key, sd[key], so[key])
    info = rt.Checkpoint.info(path)
    assert info["have_rhs"] == 0 and info["ny"] == n and info["ode_reltol"] == rtol
    # another tolerance, another size: refused by name, and the integrator goes on
    d2 = rt.OdeSolver(None, 0.0, np.zeros(n), rtol * 2, atol, h0, 0.0, 0.0, fn=fn)
    with pytest.raises(rt.ShudRhsError, match="reltol"):
        rt.Checkpoint.restore(path, d2)
    assert d2.solve(touts[0])[0] == 0
    d2.close()
    ck.close()
    d.close()
    kat.shud_kat_ode_free(u)


# ---------------------------------------------------------------- the SHUD loop
def _unzip(prj, root, cryo=False):
    with zipfile.ZipFile(os.path.join(GOLDEN, "input", f"{prj}.zip")) as z:
        z.extractall(root)
    src = os.path.join(root, "input", prj)
    if cryo:                                             # the cryosphere settings of tests/golden/ref/ccw_cryo.cfg.*
        for ext in ("para", "calib"):
            shutil.copy(os.path.join(GOLDEN, "ref", f"ccw_cryo.cfg.{ext}"), os.path.join(src, f"{prj}.cfg.{ext}"))
    return src


def _project(kind, root):
    """-> (project directory, project name, cwd)"""
    root = str(root)
    if kind == "syn":
        synth.write_project(root, "syn", 2000, days=1.0, max_step=10.0, et_step=60.0, dt_out=60)
        return root, "syn", root
    prj = "qhh" if kind == "qhh" else "ccw"
    return _unzip(prj, root, cryo=kind == "cryo"), prj, root


class Run(driver.ProjectRun):
    """one process's worth of objects over a project: handle + ET prelude, output set (.dat and .csv controls at two
    intervals), optionally the monitors; resume=True opens the files of an earlier run"""

    def __init__(self, proj, outdir, mode=abi.SHUD_MODE_SERIAL, order=None, resume=False, monitors=False,
                 tweak=None):
        src, prj, cwd = proj
        # the projects' own tolerances (1e-4) let ccw and qhh take one internal step per solver step at order 1 for
        # hours; tighter ones make the integrator work inside every solver step, so the order rises within a few
        super().__init__(src, prj, outdir, cwd=cwd, mode=mode, order=order, tweak=tweak, resume=resume,
                         control=dict(reltol=1e-6, abstol=1e-6, init_step=1e-3),
                         override=lambda k, d: dict(interval=INTERVALS[k % 2], binary=True, ascii=k % 3 == 0),
                         flood=monitors and dict(path=os.path.join(str(outdir), "run.flood.csv"), riv_depth=0.0,
                                                 riv_type=1))
        self.states = []
        self.qcur = []                                   # the integrator's order after each solver step

    def start(self):
        y0 = self.P.array("y0").copy()
        if self.prj == "ccw":
            # ccw's shipped initial condition is so close to steady that the integrator stays at order 1 for hours
            # at any tolerance (qcur 1 after each of 12 solver steps at 1e-4 and at 1e-6): 5 cm of ponded water on every
            # element gives it a transient to resolve, so the order rises and the split crosses a real history
            y0[:self.m.num_ele] += 0.05
        return super().start(y0)

    def steps(self, n, each=None):
        def on_output(i, t, y):                          # (the flood monitor has run: ProjectRun.run)
            self.states.append(y.copy())
            self.qcur.append(self.sv.stats()["qcur"])
            if each:
                each(self)
        self.run(n, on_output=on_output)
        return self

    def snapshot(self, path):
        self.sv.snapshot(path, output=self.out, monitors=self.mon)
        self.sv.flush_snapshot()

    def result(self):
        """(states, num_calls, stats, {file: bytes}) and everything closed"""
        st, nc = self.sv.stats(), self.h.num_calls()
        self.close()
        files = {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(self.outdir, "*")))
                 if not f.endswith(".ckpt")}
        return self.states, nc, st, files


def _same(a, b):
    sa, na, ta, fa = a
    sb, nb, tb, fb = b
    assert len(sa) == len(sb)
    for k, (x, y) in enumerate(zip(sa, sb)):
        assert x.tobytes() == y.tobytes(), (k, np.abs(x - y).max())
    assert na == nb, (na, nb)
    assert ta == tb, {k: (ta[k], tb[k]) for k in ta if ta[k] != tb[k]}
    assert sorted(fa) == sorted(fb)
    for f in fa:
        assert fa[f] == fb[f], (f, len(fa[f]), len(fb[f]))


def _inside(ctl, k):
    """after k solver steps the run is strictly inside an (hourly) forcing interval, and the 30-minute controls'
    accumulators are half filled"""
    el = k * ctl.solver_step
    return el % 60.0 != 0.0 and el % INTERVALS[1] != 0.0


TOTAL = 12


def _split_point(run):
    """the issue's split after 4 of 8 solver steps asks for qcur >= 2 there; where a project's integrator is still at
    order 1 after 4 steps (ccw: the first steps already run at the maximal step size), the split moves to the first
    later step that meets every condition, in a run of TOTAL steps"""
    for k in range(4, TOTAL - 1):
        if run.qcur[k - 1] >= 2 and _inside(run.ctl, k):
            return k
    raise AssertionError(f"no solver step with qcur >= 2 inside a forcing interval: qcur {run.qcur}")


def _split_run(proj, tmp_path, split, total, **kw):
    """`split` steps, snapshot, everything closed, fresh objects, restore, the rest -> (result, path, qcur at the split)"""
    path = tmp_path / "run.ckpt"
    a = Run(proj, tmp_path / "split", **kw).start().steps(split)
    q = a.sv.stats()["qcur"]
    assert _inside(a.ctl, split)
    a.snapshot(path)
    states = a.states
    a.close()
    b = Run(proj, tmp_path / "split", resume=True, **kw).restore(path)
    assert b.sv.step == split
    b.states = states
    return b.steps(total - split).result(), path, q


CASES = {"ccw": ("ccw", {}), "omp": ("ccw", dict(mode=abi.SHUD_MODE_OMP)), "soa": ("ccw", {}),
         "tiles": ("ccw", dict(order="tiles")), "qhh": ("qhh", {}), "cryo": ("cryo", {}), "syn": ("syn", {})}


@pytest.mark.parametrize("case", list(CASES))
def test_split_equals_straight_shud_loop(case, tmp_path, monkeypatch):
    """TOTAL solver steps straight against 4 + snapshot + fresh process state + restore + the rest (the split after
    step 4 has qcur >= 2 in every case: 2 on qhh, 4 on ccw, 5 on the synthetic project), and against a split after the
    first solver step (order 1, etamax still in its start-up phase).  ccw runs with terrain radiation on (the
    reference's default), so every split lies inside a forcing interval whose solar samples the resumed project
    recomputes; cryo splits with both day-mean queues holding a day."""
    kind, kw = CASES[case]
    if case == "soa":
        monkeypatch.setenv("SHUD_RHS_PACKED", "0")
    proj = _project(kind, tmp_path / "prj")
    straight = Run(proj, tmp_path / "straight", **kw).start()
    if kind != "syn":
        assert straight.c["terrain_radiation"] == 1
    straight.steps(TOTAL)
    split = _split_point(straight)
    print(f"{case}: qcur after each solver step {straight.qcur}, split after step {split}")
    straight = straight.result()
    assert len(straight[3]) >= 10
    got, path, q = _split_run(proj, tmp_path / "a", split, TOTAL, **kw)
    assert q >= 2, q
    _same(got, straight)
    info = rt.Checkpoint.info(path)
    if case == "soa":
        assert info["layout"] == abi.SHUD_CKPT_LAYOUT_SOA
    else:
        assert info["layout"] in (abi.SHUD_CKPT_LAYOUT_PACKED, abi.SHUD_CKPT_LAYOUT_HYBRID)
    assert info["step"] == split and info["order_kind"] == (abi.SHUD_ORDER_TILES if case == "tiles" else 0)
    assert info["mode"] == kw.get("mode", abi.SHUD_MODE_SERIAL) and info["have_et"] == 1
    if case == "cryo":
        # section et.queues.host (csrc/shud_ckpt_parts.h): int32 head_surf, size_surf, head_sub, size_sub, n_of_day, pad,
        # then double time_start — a section of its own, so its layout does not move with the ET settings
        raw = np.zeros(8, dtype=np.uint64)
        nw = C.c_uint64()
        assert rt.lib().shud_ckpt_read_section(str(path).encode(), b"et.queues.host", raw.ctypes.data_as(abi.c_uint64_p),
                                               8, C.byref(nw)) == 0
        assert nw.value == 4
        q = np.frombuffer(raw.tobytes()[:24], dtype=np.int32)
        t_start = np.frombuffer(raw.tobytes()[24:32], dtype=np.float64)[0]
        assert q[1] >= 1 and q[3] >= 1 and 0 <= q[0] and 0 <= q[2] and q[5] == 0, q
        assert t_start >= 0.0, t_start                   # a day mean was pushed (the initial value is -9999)
    got1, _, _ = _split_run(proj, tmp_path / "b", 1, TOTAL, **kw)
    _same(got1, straight)


def test_snapshot_changes_nothing_and_refresh_diagnostics(tmp_path):
    """a run that snapshots after every solver step equals the run without a checkpoint object; and
    refresh_diagnostics directly after a restore gives the arrays it gave directly before the snapshot"""
    proj = _project("ccw", tmp_path / "prj")
    straight = Run(proj, tmp_path / "straight").start().steps(5).result()
    path = tmp_path / "every.ckpt"
    a = Run(proj, tmp_path / "every").start().steps(5, each=lambda r: r.snapshot(path))
    which = [abi.SHUD_ARR_Q_INFIL, abi.SHUD_ARR_QELE_SUB, abi.SHUD_ARR_QRIV_DOWN, abi.SHUD_ARR_Q_ETA]

    def diag(r):
        r.h.refresh_diagnostics()
        out = []
        for w in which:
            p, n = r.h.device_array(w)
            out.append(r.h.d2h(np.empty(n), p).tobytes())
        return out
    before = diag(a)
    _same(a.result(), straight)
    b = Run(proj, tmp_path / "every", resume=True).restore(path)
    assert diag(b) == before
    b.close()


def test_refusals_leave_objects_usable_and_cut_back(tmp_path, monkeypatch):
    proj = _project("ccw", tmp_path / "prj")
    straight = Run(proj, tmp_path / "straight", monitors=True).start().steps(6).result()
    assert len(straight[3]["run.flood.csv"]) > 100
    path = tmp_path / "run.ckpt"
    a = Run(proj, tmp_path / "split", monitors=True).start().steps(3)
    a.snapshot(path)
    # an output set with a NetCDF sink: refused, and the run goes on
    nc = rt.Output(stream=a.h.stream())
    nc.attach_nc("riv", a.m.num_riv, a.c["forc_start_time"], out_dir=str(tmp_path / "nc"))
    ck = rt.Checkpoint(stream=a.h.stream())
    with pytest.raises(rt.ShudRhsError, match="NetCDF") as e:
        ck.snapshot(tmp_path / "nc.ckpt", a.sv.t, a.sv.step, a.sv.ode, rhs=a.h, output=nc)
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED
    ck.close()
    nc.close()
    states = a.states
    a.steps(1)                                           # the killed run: a step past its last checkpoint ...
    a.close()
    for f, junk in (("ccw.eleysurf.dat", b"\x01" * 123), ("run.flood.csv", b"9.9\t1\t1\tjunk\n" * 7)):
        with open(tmp_path / "split" / f, "ab") as fh:   # ... and junk rows after it
            fh.write(junk)
    states = states[:3]

    def wrong(**kw):                                     # a handle the file does not belong to
        r = Run(proj if "proj" not in kw else kw.pop("proj"), tmp_path / "wrong", **kw).start()
        return r

    def refused(r, match):
        with pytest.raises(rt.ShudRhsError, match=match) as e:
            rt.Checkpoint.restore(path, r.sv.ode, rhs=r.h, output=r.out, monitors=r.mon)
        assert e.value.code == abi.SHUD_ERR_ARG
        r.steps(1)                                       # untouched and usable
        assert np.all(np.isfinite(r.states[-1]))
        r.close()

    refused(wrong(mode=abi.SHUD_MODE_OMP, monitors=True), "mode")
    monkeypatch.setenv("SHUD_RHS_PACKED", "0")
    refused(wrong(monitors=True), "layout")
    monkeypatch.delenv("SHUD_RHS_PACKED")
    refused(wrong(proj=_project("syn", tmp_path / "syn"), monitors=True), "NE")

    def ksat(m):
        m.par["KsatH"] = m.par["KsatH"].copy()
        m.par["KsatH"][17] = np.nextafter(m.par["KsatH"][17], np.inf)
    refused(wrong(tweak=ksat, monitors=True), "statics fingerprint")
    # a corrupted payload: refused with the section's name; then the true file, into the same objects
    raw = bytearray(open(path, "rb").read())
    info = rt.Checkpoint.info(path)
    sec = [s for s in info["sections"] if s[0] == "ode.zn"][0]
    raw[info["header_bytes"] + 8 * sec[1] + 8 * 1000 + 1] ^= 4
    bad = tmp_path / "bad.ckpt"
    open(bad, "wb").write(raw)
    b = Run(proj, tmp_path / "split", resume=True, monitors=True).start()
    with pytest.raises(rt.ShudRhsError, match="ode.zn"):
        rt.Checkpoint.restore(bad, b.sv.ode, rhs=b.h, output=b.out, monitors=b.mon)
    b.sv.close()
    b.restore(path)
    b.states = states
    _same(b.steps(3).result(), straight)                 # the junk and the killed run's rows are gone


def test_partitioned_handle_and_water_balance_refused(kat, tmp_path):
    """SHUD_ERR_UNSUPPORTED with a message, on snapshot and on restore, for a partitioned handle (built on one GPU as
    tests/test_gpu_wb.py does) and for a run that names a water-balance object; the objects stay usable"""
    m, y0 = cases.variant(n=2000)
    _, _, plans = partition.build_plans(m, 2)
    lm, part = partition.local_model(m, plans[0], 0, 2)
    h = rt.RhsHandle(lm, partition=part)
    u, fn = _dev(kat, "decay", 3)                        # (shud_ode_create itself refuses a partitioned handle)
    d = rt.OdeSolver(None, 0.0, np.ones(3), 1e-6, 1e-10, 1e-3, 0.0, 0.0, fn=fn)
    assert d.solve(0.1)[0] == 0
    ck = rt.Checkpoint(stream=fn[2])
    good = tmp_path / "ode.ckpt"
    ck.snapshot(good, 0.1, 1, d)                         # a valid file for the restore to get as far as the handle
    ck.flush()
    with pytest.raises(rt.ShudRhsError, match="partitioned handles cannot be checkpointed") as e:
        ck.snapshot(tmp_path / "p.ckpt", 0.1, 1, d, rhs=h)
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED and not os.path.exists(tmp_path / "p.ckpt")
    with pytest.raises(rt.ShudRhsError, match="partitioned handles cannot be checkpointed") as e:
        rt.Checkpoint.restore(good, d, rhs=h)
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED
    # still usable: the handle packs its halo and evaluates (the ghost buffers filled by hand, as the external-
    # transport tests of tests/test_gpu_partition.py do with copies), the integrator steps on
    d_y = h.device_alloc(8 * h.num_y)
    d_dy = h.device_alloc(8 * h.num_y)
    h.h2d(d_y, partition.local_state(y0, m, part))
    h.set_step_inputs()
    h.eval_pack(d_y)
    _, _, gele, griv = h.halo_buffers()
    n_eg, n_rg = lm.num_ele - part.n_own_ele, lm.num_riv - part.n_own_riv
    if n_eg:
        h.h2d(gele, np.full(3 * n_eg, 0.1))
    if n_rg:
        h.h2d(griv, np.full(n_rg, 0.1))
    h.eval_compute(0.0, d_y, d_dy)
    h.synchronize()
    assert h.num_calls() == 1 and np.all(np.isfinite(h.d2h(np.empty(h.num_y), d_dy)))
    assert d.solve(0.2)[0] == 0
    h.device_free(d_y)
    h.device_free(d_dy)
    h.close()
    # a water-balance object in the run
    mc, yc = cases.ccw()
    hc = rt.RhsHandle(mc)
    hc.set_step_inputs()
    hc.prepare_outputs()
    d_yc = hc.device_alloc(8 * hc.num_y)
    hc.h2d(d_yc, yc)
    hc.summary(d_yc)                                     # (shud_wb_create wants the summary arrays filled)
    wb = rt.WaterBalance(hc, 60)
    with pytest.raises(rt.ShudRhsError, match="water-balance") as e:
        ck.snapshot(tmp_path / "w.ckpt", 0.1, 1, d, wb=wb)
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED and not os.path.exists(tmp_path / "w.ckpt")
    with pytest.raises(rt.ShudRhsError, match="water-balance") as e:
        parts =abi.ShudCkptParts(None, d.h, None, None, wb.h)
        rt._check(rt.lib().shud_ckpt_restore(str(good).encode(), C.byref(parts), None, None), "shud_ckpt_restore")
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED
    assert d.solve(0.3)[0] == 0
    wb.close()
    hc.device_free(d_yc)
    hc.close()
    ck.close()
    d.close()
    kat.shud_kat_ode_free(u)


def test_error_word_refused(tmp_path):
    proj = _project("syn", tmp_path / "prj")
    a = Run(proj, tmp_path / "o").start().steps(1)
    y = a.states[-1].copy()
    y[3] = np.nan
    a.h.eval(a.sv.t, y, raise_on_physics=False)
    assert a.h.get_error()["flags"] != 0
    with pytest.raises(rt.ShudRhsError, match="error word"):
        a.snapshot(tmp_path / "e.ckpt")
    assert not os.path.exists(tmp_path / "e.ckpt")
    a.close()


# ---------------------------------------------------------------- shud_gpu --checkpoint / --resume
def test_shud_gpu_checkpoint_resume(tmp_path):
    root = str(tmp_path / "ref")
    src = _unzip("ccw", root)
    cfg = os.path.join(src, "ccw.cfg.para")
    # 60-minute outputs: the checkpoint after 3 ten-minute steps carries half-filled accumulators, the row comes at 6
    txt = re.sub(r"^(DT_\w+)\s+\d+", r"\1\t60", open(cfg).read(), flags=re.M)
    open(cfg, "w").write(txt)

    def run(outdir, extra, env=None):
        return shud_gpu_run.run(["-o", outdir, "-C", root, "-e", "0.125", "--flood", "--ic-snapshots"] + extra +
                                [src, "ccw"], env=env, check=False)
    a, b, ck = tmp_path / "straight", tmp_path / "split", str(tmp_path / "p.ckpt")
    r0 = run(a, ["-n", "6"])
    r1 = run(b, ["-n", "3", "--checkpoint", ck])
    r2 = run(b, ["--resume", ck, "-n", "6"])
    for r in (r0, r1, r2):
        assert r.returncode == 0, r.stdout + r.stderr
    assert "resumed from" in r2.stdout and rt.Checkpoint.info(ck)["step"] == 3
    fa = sorted(os.path.basename(f) for f in glob.glob(str(a / "*")))
    print(fa, r0.stdout[-600:], r0.stderr[-300:])
    assert len(fa) >= 15 and fa == sorted(os.path.basename(f) for f in glob.glob(str(b / "*")))
    for f in fa:
        assert open(a / f, "rb").read() == open(b / f, "rb").read(), f
    rw = run(tmp_path / "wb", ["-n", "3", "--checkpoint", ck], env={"SHUD_WB_DIAG": "1"})
    assert rw.returncode != 0 and "SHUD_WB_DIAG" in rw.stderr and "checkpoint" in rw.stderr
