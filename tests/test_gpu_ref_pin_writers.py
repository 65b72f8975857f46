"""GPU: the device output path, run monitors and water balance held to the files the REFERENCE model's own writers
left, from the recordings under tests/golden/ref/ alone (oracle/ref/record.py writers; tests/test_ref_pin_writers.py
holds the CPU oracle and the Python restatements to the same recordings byte for byte).

The handle is driven as the recording was: the recorded step inputs per ET() call, eval_device on every scripted
RHS input, summary on the state handed to Model_Data::summary, refresh_diagnostics, Output.export(t),
RunMonitors.flood(t) / ic_update(t), and WaterBalance.sample / maybe_write where the recording had SHUD_WB_DIAG.
Serial semantics (the recordings are the serial reference's), packed and SoA layouts; qhh (lakes) in the packed
layout only (the handle refuses the other).

Byte-identical: every header, every file of copied values (element / river / lake storages with their BC
overrides, interception and snow storages fed through et_set_state, the ET step's precipitation and potential ET
inputs), the row times of every file, every restart file, the flood file's rows and its time / ID / type / stage /
bank columns.  Flux files: each row under the rule tests/test_gpu_parity.py applies to that diagnostic array
against the oracle (conftest.assert_close, the `blocks` allowance for the near-cancelling sums), the absolute term
scaled by the file's tau (1440 for a flux); the flood file's discharge column under that rule plus 1e-6 (two
roundings to six decimals).  rn_h / rn_t / rn_factor are left out: a handle without a terrain-radiation ET step
has nothing to put there."""
import json
import os

import numpy as np
import pytest

import ref_writers as rw
from conftest import ATOL, assert_close
from ref_writers import refio
from shud_rhs import abi

pytestmark = pytest.mark.gpu
RUNS = [("ccw_w", "packed"), ("ccw_w", "soa"), ("syn_w", "packed"), ("syn_w", "soa"), ("qhh_w", "packed")]
SUMS = ("qele_surf_tot", "qele_sub_tot", "qe2r_surf", "qe2r_sub", "qriv_up", "qriv_surf", "qriv_sub")
COPIED = set(rw.ARR_STATE) | set(rw.ARR_ET) | {abi.SHUD_ARR_Q_LAKE_RIVOUT}
_DEV = {}


def _device_run(case, layout, monkeypatch, tmp_path_factory):
    """drive one handle through the recorded schedule, once per (case, layout) -> dict(dir, decl, ic, wb rows ...)"""
    if (case, layout) in _DEV:
        return _DEV[(case, layout)]
    from shud_rhs import driver, runtime as rt
    monkeypatch.setenv("SHUD_RHS_PACKED", "1" if layout == "packed" else "0")
    L = rw.load(case, tmp_path_factory)
    rec, m, prj = L["rec"], L["m"], L["prj"]
    outdir = tmp_path_factory.mktemp(f"dev_{case}_{layout}")
    P = rw.project(L)
    c = P.control()
    NE, NR, NL = m.num_ele, m.num_riv, getattr(m, "num_lake", 0) or 0
    _, h = driver.device_model(P, model=m)
    assert h.layout()["packed"] == (layout == "packed"), h.layout()
    h.et_set_state(rec["ic_is"], rec["ic_snow"])
    d_y, d_s, d_dy = (h.device_alloc(8 * m.num_y) for _ in range(3))
    h.h2d(d_s, L["y0"])
    h.summary(d_s)                                       # LoadIC / SetIC2Y: the arrays before the first f()
    h.prepare_outputs()
    out = rt.Output(stream=h.stream())
    # rn_h / rn_t / rn_factor: a handle without a terrain-radiation ET step has nothing to put there
    decl = driver.add_outputs(P, h, out, outdir, c=c, override=lambda k, d: None if d["array"] in rw.ARR_RN else {})
    mon = driver.monitors(P, h, outdir, prj, flood=True, ic=True)
    flood_path, ic_path = outdir / f"{prj}.flood.csv", outdir / f"{prj}.cfg.ic.update"
    ics = []

    def ic_update(t):                                    # PrintInit(Init_update, t): every written file is kept
        if mon.ic_update(t):
            mon.flush()
            ics.append(open(ic_path, "rb").read())

    env = refio.WRITER_CASES[case]["env"]
    wb, wb_rows, wb_terms = None, [], []
    if env.get("SHUD_WB_DIAG"):
        wb = driver.water_balance(P, h, outdir, prj, c=c)
    # PrintInit at StartTime comes before any f(): the reference's arrays hold the initial condition as read, no
    # boundary head yet, which the device's summary arrays already carry.  As the host driver does (shud_gpu.cpp),
    # that first file is written from the host's arrays.
    y0p, t0 = P.array("y0"), float(rec["dims"][4])
    if mon.ic_update(t0):
        mon.flush()
        rt.write_ic_host(ic_path, t0, P.array("y_is"), P.array("y_snow"), y0p[:NE], y0p[NE:2 * NE], y0p[2 * NE:3 * NE],
                         y0p[3 * NE:3 * NE + NR], y0p[3 * NE + NR:] if NL else None)
        ics.append(open(ic_path, "rb").read())
    after_summary, bc, et_cur = False, {}, None
    for op in L["ops"]:
        if op[0] == "et":
            et_cur = op[1]
            h.set_step_inputs(refio.writer_step(rec, et_cur), bc)
            h.et_set_state(rec["et:y_is"][et_cur], rec["et:y_snow"][et_cur])
            if wb:
                wb.on_et_update()
        elif op[0] == "summary":
            h.h2d(d_s, op[1])
            h.summary(d_s)
            after_summary = True
        elif op[0] == "f":
            _, t, y, j = op
            bc = refio.writer_bc(rec, j)
            if bc:
                h.set_step_inputs({}, bc)
            h.h2d(d_y, y)
            h.eval_device(t, d_y, d_dy)
            if wb and after_summary:                     # shud.cpp:141-147: f() on the accepted state, then sample
                h.refresh_diagnostics()
                dg = h.diagnostics()
                wb.sample(t, d_dy)
                r = wb.read(arrays=False)
                wb_terms.append((t, dg, bc, et_cur, np.array(r["basin_rate"]), np.array(r["basin_acc"])))
        else:
            _, t, _, k = op
            h.refresh_diagnostics()
            if wb and wb.maybe_write(t):
                wb_rows.append((t, np.array(wb.read(arrays=False)["basin_row"])))
            out.export(t)
            mon.flood(t)
            ic_update(t)
            after_summary = False
    out.close()
    mon.flush()
    flood = open(flood_path, "rb").read()
    mon.close()
    if wb:
        wb.close()
    for p in (d_y, d_s, d_dy):
        h.device_free(p)
    h.close()
    P.close()
    _DEV[(case, layout)] = dict(L=L, dir=outdir, decl=decl, ics=ics, flood=flood, wb_rows=wb_rows, wb_terms=wb_terms,
                                control=c)
    return _DEV[(case, layout)]


def _report(name, data):
    """the measured deviations (largest absolute, largest relative), as DESIGN §2's table has them"""
    print("REFPIN-W " + json.dumps({name: data}))


@pytest.mark.parametrize("case,layout", RUNS, ids=[f"{c}-{lay}" for c, lay in RUNS])
def test_output_files_vs_reference(case, layout, monkeypatch, tmp_path_factory):
    D = _device_run(case, layout, monkeypatch, tmp_path_factory)
    ref, c = D["L"]["files"], D["control"]
    worst = {}
    for d in D["decl"]:
        base = os.path.basename(d["basename"])
        got, want = open(d["basename"] + ".dat", "rb").read(), ref[base + ".dat"]
        gh, gi, gt, gd = rw.dat_rows(got)
        wh, wi, wt, wd = rw.dat_rows(want)
        assert gh == wh, f"{base}.dat: header"
        assert gt.tobytes() == wt.tobytes(), f"{base}.dat: row times {gt} != {wt}"
        if d["array"] in COPIED:
            assert got == want, f"{base}.dat: a file of copied values differs from the reference's"
            if c["ascii"]:
                assert open(d["basename"] + ".csv", "rb").read() == ref[base + ".csv"], f"{base}.csv"
            continue
        tau = 1440.0 if d["iflux"] else 1.0
        name = {abi.SHUD_ARR_Q_TRANS: "q_trans", abi.SHUD_ARR_Q_EVAPO: "q_evapo"}.get(d["array"]) or rw.ARR_DIAG[d["array"]]
        wa = wr = 0.0
        for r in range(gt.size):
            a, rel = assert_close(gd[r], wd[r], atol=ATOL * tau, what=f"{case} {layout} {base}.dat row {r}",
                                  blocks=[slice(None)] if name in SUMS else None)
            wa, wr = max(wa, a), max(wr, rel)
        worst[base.split(".", 1)[1]] = (wa, wr)
        if c["ascii"]:                                   # the text header and the row times of the .csv
            gl, wl = open(d["basename"] + ".csv", "rb").read().split(b"\n"), ref[base + ".csv"].split(b"\n")
            assert len(gl) == len(wl) and gl[:7] == wl[:7], f"{base}.csv"
            assert [ln.split(b"\t")[0] for ln in gl] == [ln.split(b"\t")[0] for ln in wl], f"{base}.csv"
    families = {}
    for k, (a, r) in worst.items():
        fam = k.rstrip("123")
        fa, fr = families.get(fam, (0.0, 0.0))
        families[fam] = (max(fa, a), max(fr, r))
    _report(f"{case}-{layout}", families)
    copied = [d for d in D["decl"] if d["array"] in COPIED]
    assert len(copied) >= 4 and len(worst) >= (1 if case == "qhh_w" else 10)
    if case == "qhh_w":                                  # the lake stage of the last RHS input, not summary's vector;
        assert any(d["array"] == abi.SHUD_ARR_Y_LAKE_STG for d in copied)     # qEleEvapo = qPotEvap on lake elements
        lake = np.asarray(D["L"]["m"].ilake) > 0
        ev = rw.dat_rows(ref["qhh.elevetev.dat"])[3]
        assert "elevetev" in worst and lake.any() and (ev[:, lake] != 0).any()


@pytest.mark.parametrize("case,layout", RUNS, ids=[f"{c}-{lay}" for c, lay in RUNS])
def test_monitor_files_vs_reference(case, layout, monkeypatch, tmp_path_factory):
    D = _device_run(case, layout, monkeypatch, tmp_path_factory)
    L = D["L"]
    ref, prj = L["files"], L["prj"]
    # restart files: every .cfg.ic.update the reference wrote, in order
    want = [ref[k] for k in sorted((k for k in ref if ".cfg.ic.update." in k), key=lambda s: int(s.rsplit(".", 1)[1]))]
    assert len(D["ics"]) == len(want) >= 2
    for n, (a, b) in enumerate(zip(D["ics"], want)):
        assert a == b, f"{case} {layout}: restart file {n} differs from the reference's"
    # flood file: the row set and the time / ID / type / stage / bank columns as bytes, the discharge as numbers
    gl, wl = D["flood"].split(b"\n"), ref[f"{prj}.flood.csv"].split(b"\n")
    assert gl[0] == wl[0] and len(gl) == len(wl)
    gq, wq = [], []
    for a, b in zip(gl[1:], wl[1:]):
        if not b:
            assert not a
            continue
        fa, fb = a.split(b"\t"), b.split(b"\t")
        assert fa[:5] == fb[:5], (a, b)
        gq.append(float(fa[5]))
        wq.append(float(fb[5]))
    if wq:
        a, r = assert_close(np.array(gq), np.array(wq), atol=ATOL + 1e-6, what=f"{case} {layout} flood discharge")
        _report(f"{case}-{layout}-flood", {"discharge": (a, r), "rows": len(wq)})
    assert (len(wq) > 0) == (case != "qhh_w")


@pytest.mark.parametrize("layout", ["packed", "soa"])
def test_basin_rows_within_fsum_bound(layout, monkeypatch, tmp_path_factory):
    """syn + BC with SHUD_WB_DIAG: every basin rate of every sample, on the device and in the reference's recorded
    row alike, lies within the bound every summation order meets, |sum - fsum(terms)| <= (n - 1) 2^-53 sum|terms|,
    carried through the row's Euler accumulation acc += rate dt (one rounding per multiply and per add: 2^-52 of
    the accumulated magnitude per sample).  The device's terms are its own diagnostics, the reference's the
    oracle's (bit-equal to the reference's arrays, tests/test_ref_pin_writers.py).  Qout goes through Manning's
    equation (cbrt: OCML on the device, glibc in the reference), so its terms are not reproducible on the host to
    the last bit and it is left to tests/test_gpu_wb.py."""
    import math

    import wb_py
    D = _device_run("syn_w", layout, monkeypatch, tmp_path_factory)
    L = D["L"]
    rec, m = L["rec"], L["m"]
    assert (np.asarray(m.ibc) < 0).any() and (np.asarray(m.riv_bc) < 0).any()
    ref_rows = rw.dat_rows(L["files"]["syn.basinwbfull.dat"])
    assert len(D["wb_rows"]) == ref_rows[2].size >= 2
    cols = {"P": 1, "ET": 2, "Qedge": 4, "Qbc": 5, "Qss": 6, "noncons": 7}
    rate_i = {"P": abi.SHUD_WB_P, "ET": abi.SHUD_WB_ET, "Qedge": abi.SHUD_WB_QEDGE, "Qbc": abi.SHUD_WB_QBC,
              "Qss": abi.SHUD_WB_QSS, "noncons": abi.SHUD_WB_NONCONS}
    import oracle
    trace = rw.replay_oracle(L, oracle.OracleRhs(m, abi.SHUD_MODE_SERIAL))
    o_samples = []                                      # (t, diag, bc, et) of the f() before every sample
    after = False
    for op in trace:
        if op[0] == "summary":
            after = True
        elif op[0] == "f" and after:
            o_samples.append((op[1], op[4], op[6], op[5]))
            after = False
    assert len(o_samples) == len(D["wb_terms"])

    def terms_of(diag, bc, et, ic_raw):
        keep = m.bc_tables
        m.bc_tables = bc
        try:
            tm = wb_py.sample_terms(m, ic_raw, diag, rec["et:prcp"][et], np.zeros(m.num_riv))
        finally:
            m.bc_tables = keep
        tm["Qbc"] = np.concatenate([tm["Qbc"], tm["Qbc_riv"]])
        tm["noncons"], tm["Qedge"] = tm["noncons_edges"], tm["Qedge_edges"]
        return tm

    acc = {side: {k: [0.0, 0.0] for k in cols} for side in ("dev", "ref")}      # [exact integral, bound]
    last_t, row = float(rec["dims"][4]), 0
    for (t, dg, bc, et, rate, _), (to, do, bco, eto) in zip(D["wb_terms"], o_samples):
        assert t == to and et == eto
        dt = t - last_t
        last_t = t
        for side, diag in (("dev", dg), ("ref", do)):
            tm = terms_of(diag, bc, et, rec["et:e_ic"][et])
            for k in cols:
                v = np.asarray(tm[k], dtype=np.float64).ravel()
                v = v[v != 0.0] if k in ("Qbc", "noncons", "Qedge") else v
                s_abs = math.fsum(np.abs(v).tolist())
                bound = max(v.size - 1, 0) * 2.0 ** -53 * s_abs
                exact = math.fsum(v.tolist())
                if side == "dev":
                    assert abs(rate[rate_i[k]] - exact) <= bound, (k, t, rate[rate_i[k]], exact, bound)
                acc[side][k][0] += exact * dt
                acc[side][k][1] += (bound + 2.0 ** -52 * s_abs) * dt
        hit = [r for r in D["wb_rows"] if r[0] == t]
        if hit and row < ref_rows[2].size and not (row and D["wb_rows"][row - 1][0] == t):
            for k, col in cols.items():
                for side, got in (("dev", hit[0][1][col]), ("ref", ref_rows[3][row][col])):
                    exact, bound = acc[side][k]
                    print(f"basin row {row} {k} {side}: {got!r} exact {exact!r} |d| {abs(got - exact):.3e} bound {bound:.3e}")
                    assert abs(got - exact) <= bound, (side, k, row, got, exact, bound)
                    acc[side][k] = [0.0, 0.0]
            row += 1
    assert row == ref_rows[2].size
