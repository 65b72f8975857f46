"""CPU: the output writers, run monitors and water-balance diagnostics pinned to the REFERENCE model's own code.

oracle/_ref/shud_ref_f (driver mode w) runs SHUD()'s own loop (src/Model/shud.cpp:69-157: initialize_output,
WaterBalanceDiag, PrintInit, InitFloodAlert, the solver-step / ET-step loop, summary, sample / maybeWrite,
ExportResults, FloodWarning) with every CVode() call replaced by a scripted state, so the reference's Print_Ctrl,
FloodAlert, PrintInit and WaterBalanceDiag write their own files.  Those files, byte for byte, and the flux arrays
the reference held at every ExportResults are the recordings tests/golden/ref/<case>*.npz.

Held to them here, bit for bit / byte for byte:
  * every diagnostic array of OracleRhs after the scripted f() calls (the flux arrays of the last f());
  * print_ctrl_py.PrintCtrlPy fed the oracle's arrays on the project's own output plan (shud_project_outputs):
    every .dat and .csv, and with them the plan (file set, columns, interval, iflux, mask, header);
  * mon_py (flood file, restart files and their schedule) and the C formatters of shud_mon_fmt.cpp;
  * wb_py.WaterBalancePy in the reference's summation order and wb_quad_py: the six water-balance files,
    SHUD_WB_DIAG_TRAPZ on and off, and env_truthy / choose_interval / write_gate through them.
Live: where the reference binaries exist a fresh run must equal the committed recording (never skipped: the
outcome shows as "REFPIN live comparison RAN" or as a "NOT RUN" warning)."""
import numpy as np
import pytest

import mon_py
import ref_writers as rw
import wb_py
from ref_writers import refio
from shud_rhs import abi
from shud_rhs import runtime as rt

CASES = rw.CASES
EVENT_CASES = [c for c in CASES if "same_events_as" not in refio.WRITER_CASES[c]]
WB_CASES = [c for c in CASES if refio.WRITER_CASES[c]["env"].get("SHUD_WB_DIAG")]
FULL_FILE_CASES = [c for c in CASES if refio.WRITER_CASES[c].get("files") != "wb"]
_TRACE = {}


def _trace(case, tmp_path_factory):
    """the recorded schedule through OracleRhs, once per case (read-only afterwards)"""
    import oracle
    L = rw.load(case, tmp_path_factory)
    if case not in _TRACE:
        _TRACE[case] = rw.replay_oracle(L, oracle.OracleRhs(L["m"], abi.SHUD_MODE_SERIAL))
    return L, _TRACE[case]


@pytest.mark.parametrize("case", EVENT_CASES)
def test_oracle_flux_arrays_equal_reference(case, tmp_path_factory):
    """the flux arrays the reference holds at ExportResults (those of its last f() call) against
    OracleRhs.diagnostics(): values, NaN pattern and signed zeros"""
    L, trace = _trace(case, tmp_path_factory)
    rec, m = L["rec"], L["m"]
    n_x = 0
    for op in trace:
        if op[0] != "x":
            continue
        _, t, st, k, diag, et, _ = op
        n_x += 1
        for key in refio.W_SUMMARY_KEYS:
            assert rw.same_bits(st[key], rec[f"x:{key}"][k]), (case, k, key)
        for key in refio.W_FLUX_KEYS:
            if f"x:{key}" not in rec:
                continue
            want = rec[f"x:{key}"][k]
            if key == "q_trans":
                got = rw.export_values(L, abi.SHUD_ARR_Q_TRANS, 0, st, diag, et, k)
            elif key == "q_evapo":
                got = rw.export_values(L, abi.SHUD_ARR_Q_EVAPO, 0, st, diag, et, k)
            elif key == "q_lake_rivout":
                got = np.zeros(want.size)
            else:
                got = diag[refio.W_DIAG_NAME.get(key, key)]
            bad = int((~(((got == want) & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want)))).sum()) \
                if got.shape == want.shape else -1
            assert bad == 0, f"{case} export {k} (t={t}) {key}: {bad} of {want.size} entries differ"
    assert n_x == int(rec["control"][0])
    if case == "qhh_w":                                   # the recorded lake stage is the last RHS input's
        f_lake = [op[2][-1] for op in trace if op[0] == "f"]
        assert rec["x:y_lake"][0, 0] == f_lake[0] != L["rec"]["script_y"][1][-1]


@pytest.mark.parametrize("case", FULL_FILE_CASES)
def test_print_ctrl_files_and_output_plan(case, tmp_path_factory, tmp_path):
    """PrintCtrlPy over shud_project_outputs' declarations reproduces the reference's .dat / .csv set byte for byte:
    the same files (suffix, n_all, interval, iflux, column, mask), headers, row times and rows"""
    L, trace = _trace(case, tmp_path_factory)
    decl, c = rw.restate_outputs(L, trace, tmp_path)
    ref = {k: v for k, v in L["files"].items() if k.endswith((".dat", ".csv")) and "wb" not in k.split(".")[1]
           and not k.endswith(".flood.csv")}
    import os
    got = {f: open(tmp_path / f, "rb").read() for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == sorted(ref), sorted(set(got) ^ set(ref))
    assert len(decl) == int(L["rec"]["wb_flags"][2])     # CS.NumPrint
    for d in decl:                                        # the declaration alone gives the reference's header
        name = os.path.basename(d["basename"]) + ".dat"
        sel = np.arange(d["n_all"]) if d["flag_io"] is None else np.nonzero(d["flag_io"])[0]
        head, icol, _, _ = rw.dat_rows(ref[name])
        assert np.array_equal(icol, sel + 1.0), name
        assert np.frombuffer(head, np.float64, 2, 1024).tolist() == [float(c["forc_start_time"]), float(sel.size)]
    for f in sorted(ref):
        assert got[f] == ref[f], f"{case}: {f} differs from the reference's file"
    if case == "ccw_w":
        assert bool(c["ascii"]) and any(f.endswith(".csv") for f in ref)
        assert b"-nan" in ref["ccw.rivystage.csv"] and b"inf" in ref["ccw.rivystage.csv"]
        # mixed intervals on one schedule: 60 min gives 6 rows, 120 and 180 min two each, at different times
        rows = {d["interval"]: rw.dat_rows(ref[os.path.basename(d["basename"]) + ".dat"])[2].tolist() for d in decl}
        assert rows == {60: [0.0, 60.0, 120.0, 240.0, 240.0, 300.0], 120: [0.0, 240.0], 180: [0.0, 180.0]}
    if case == "syn_w":                                   # .cfg.output masks: fewer columns than elements / reaches
        assert rw.dat_rows(ref["syn.eleysurf.dat"])[1].size < L["m"].num_ele
        assert rw.dat_rows(ref["syn.rivystage.dat"])[1].size < L["m"].num_riv


@pytest.mark.parametrize("case", FULL_FILE_CASES)
def test_flood_file(case, tmp_path_factory):
    L, trace = _trace(case, tmp_path_factory)
    P = rw.project(L)
    rtype = P.riv_type()
    P.close()
    depth = L["m"].riv["riv_depth"]
    calls = rw.flood_calls(trace)
    txt, total, last = mon_py.flood_file(calls, depth, rtype)
    ref = L["files"][f"{L['prj']}.flood.csv"]
    assert txt == ref
    flags = [int(mon_py.flood_rows(t, s, depth, rtype, q)[1] > 0) for t, s, q in calls]
    assert flags == L["rec"]["x:flood"][:, 0].astype(int).tolist()      # FloodWarning's return value per call
    # the C formatter of shud_mon_fmt.cpp through its Python entry, call by call
    got = rt.lib().shud_mon_flood_header()
    for t, stage, q in calls:
        idx = np.nonzero(stage > depth)[0]
        got += rt.format_flood_rows(t, idx, rtype, stage[idx], depth, q[idx])
    assert got == ref
    if case == "ccw_w":
        counts = [mon_py.flood_rows(t, s, depth, rtype, q)[1] for t, s, q in calls]
        assert any(0 < n < L["m"].num_riv for n in counts) and 0 in counts
        assert calls[0][1][0] == depth[0] and b"\n60.4\t1\t" not in ref      # a stage at the bank is no flood
        assert b"\tinf\t" in ref and b"nan" not in ref                         # inf > bank; NaN compares false


@pytest.mark.parametrize("case", FULL_FILE_CASES)
def test_restart_files(case, tmp_path_factory, tmp_path):
    L, trace = _trace(case, tmp_path_factory)
    ref = {k: v for k, v in L["files"].items() if ".cfg.ic." in k}
    got = rw.restate_ic_files(L, trace)
    assert sorted(got) == sorted(ref) and len(ref) >= 3, (sorted(got), sorted(ref))
    for f in sorted(ref):
        assert got[f] == ref[f], f
    # shud_mon_write_ic_host (shud_mon_fmt.cpp) writes the same bytes
    step = int(L["rec"]["control"][3])
    n = 0
    for kind, t, a in rw.ic_schedule(L, trace):
        if mon_py.ic_due(t, step):
            fn = tmp_path / "c.ic"
            rt.write_ic_host(fn, t, *a[:6], a[6] if len(a[6]) else None)
            assert open(fn, "rb").read() == ref[f"{L['prj']}.cfg.ic.{kind}.{n}"], (kind, t)
            n += 1
    if case == "ccw_w":
        assert sum(".update." in f for f in ref) >= 3 and any(b"-nan" in v for v in ref.values())
    if case == "qhh_w":
        assert all(b"LakeStage" in v for v in ref.values())


@pytest.mark.parametrize("case", WB_CASES)
def test_water_balance_files(case, tmp_path_factory, tmp_path):
    """wb_py in the reference's summation order ("seq") and wb_quad_py reproduce every water-balance file; the
    interval and the rows are the reference's (choose_interval through shud_project_wb_interval, write_gate)"""
    L, trace = _trace(case, tmp_path_factory)
    env = refio.WRITER_CASES[case]["env"]
    wb, quad, interval = rw.restate_wb(L, trace, tmp_path / L["prj"])
    assert L["rec"]["wb_flags"][:2].tolist() == [1.0, float(wb_py.env_truthy(env.get("SHUD_WB_DIAG_QUAD")))]
    ref = {k: v for k, v in L["files"].items() if "wb" in k.split(".")[1]}
    assert len(ref) == (6 if quad else 5)
    P = rw.project(L)
    decl = {d["basename"].rsplit(".", 1)[1]: d for d in P.outputs(str(tmp_path))}
    P.close()
    assert interval == wb_py.choose_interval(decl["elevetic"]["interval"] if "elevetic" in decl else 0,
                                             decl["eleysurf"]["interval"] if "eleysurf" in decl else 0)
    t_x = [op[1] for op in trace if op[0] == "x"]
    gate, last = [], -1
    for t in t_x:
        g = wb_py.write_gate(t, interval, last)
        if g is not None:
            gate.append(float(g - interval))
            last = g
    assert len(gate) >= 2 and (len(gate) < len(t_x) or refio.WRITER_CASES[case]["script"] != "ccw")
    for f in sorted(ref):
        got = open(tmp_path / f, "rb").read()
        assert rw.dat_rows(ref[f])[2].tolist() == gate, f
        assert got == ref[f], f"{case}: {f} differs from the reference's file"


def test_trapz_changes_the_files(tmp_path_factory):
    a, b = rw.load("ccw_wb", tmp_path_factory)["files"], rw.load("ccw_wb_trapz", tmp_path_factory)["files"]
    assert sorted(a) == sorted(b) and a["ccw.basinwbfull.dat"] != b["ccw.basinwbfull.dat"]


@pytest.mark.parametrize("case", CASES)
def test_recording_equals_live_reference(case, tmp_path):
    """a fresh run of the reference binary must equal the committed recording (a stale one fails); passes vacuously
    (not skipped) without oracle/_ref/ or with a driver there that predates mode w, with a NOT RUN warning"""
    if not refio.live_status(f"writers {case}", refio.have_writer_ref):
        return
    live = refio.run_writer_case(case, tmp_path)
    rec = refio.load_recording(case)
    assert set(rec) <= set(live), set(rec) - set(live)
    assert {k for k in live if k.startswith("file:")} == {k for k in rec if k.startswith("file:")}
    for k, v in rec.items():
        assert v.shape == live[k].shape and np.array_equal(v, live[k], equal_nan=v.dtype.kind == "f"), \
            f"recording {case}: {k} is stale"
