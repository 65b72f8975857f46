"""Shared by tests/test_ref_pin_writers.py (CPU) and tests/test_gpu_ref_pin_writers.py (GPU): the recordings the
reference's own output writers, monitors and water-balance diagnostics left (oracle/ref/record.py writers, driver
mode w: SHUD()'s loop with a scripted solver), and the replay of the recorded schedule through the CPU oracle and
the Python restatements (print_ctrl_py, mon_py, wb_py, wb_quad_py).  Not a test module."""
import os
import sys

import numpy as np

import mon_py
import wb_py
import wb_quad_py
from conftest import ORACLE_DIR
from print_ctrl_py import PrintCtrlPy
from shud_rhs import abi, host
from shud_rhs.driver import header_kw

sys.path.insert(0, os.path.join(ORACLE_DIR, "ref"))
import refio  # noqa: E402

CASES = list(refio.WRITER_CASES)
# SHUD_ARR_* -> the oracle diagnostic of the same array (RhsHandle.diagnostics() has the same names)
ARR_DIAG = {abi.SHUD_ARR_QELE_SURF_TOT: "qele_surf_tot", abi.SHUD_ARR_QELE_SUB_TOT: "qele_sub_tot",
            abi.SHUD_ARR_QELE_SURF: "qele_surf", abi.SHUD_ARR_QELE_SUB: "qele_sub",
            abi.SHUD_ARR_QE2R_SURF: "qe2r_surf", abi.SHUD_ARR_QE2R_SUB: "qe2r_sub", abi.SHUD_ARR_Q_INFIL: "q_infil",
            abi.SHUD_ARR_Q_EXFIL: "q_exfil", abi.SHUD_ARR_Q_RECHARGE: "q_recharge", abi.SHUD_ARR_Q_ETA: "q_eta",
            abi.SHUD_ARR_Q_E_IC: "e_ic", abi.SHUD_ARR_QRIV_DOWN: "qriv_down", abi.SHUD_ARR_QRIV_UP: "qriv_up",
            abi.SHUD_ARR_QRIV_SURF: "qriv_surf", abi.SHUD_ARR_QRIV_SUB: "qriv_sub",
            abi.SHUD_ARR_LAKE_TOPAREA: "lake_toparea", abi.SHUD_ARR_Q_LAKE_EVAP: "q_lake_evap",
            abi.SHUD_ARR_Q_LAKE_PRCP: "q_lake_prcp", abi.SHUD_ARR_Q_LAKE_RIVIN: "q_lake_rivin",
            abi.SHUD_ARR_Q_LAKE_SURF: "q_lake_surf", abi.SHUD_ARR_Q_LAKE_SUB: "q_lake_sub"}
ARR_ET = {abi.SHUD_ARR_Q_PRCP: "prcp", abi.SHUD_ARR_Q_NET_PRCP: "net_prep", abi.SHUD_ARR_Q_ETP: "etp",
          abi.SHUD_ARR_Y_ELE_IS: "y_is", abi.SHUD_ARR_Y_ELE_SNOW: "y_snow"}
ARR_RN = {abi.SHUD_ARR_RN_H: "rn_h", abi.SHUD_ARR_RN_T: "rn_t", abi.SHUD_ARR_RN_FACTOR: "rn_factor"}
ARR_STATE = {abi.SHUD_ARR_Y_ELE_SURF: "y_surf", abi.SHUD_ARR_Y_ELE_UNSAT: "y_unsat", abi.SHUD_ARR_Y_ELE_GW: "y_gw",
             abi.SHUD_ARR_Y_RIV_STG: "y_riv", abi.SHUD_ARR_Y_LAKE_STG: "y_lake"}
WB_FILES = [ext for _, ext in wb_py.LABELS] + [wb_quad_py.QUAD_EXT]
_CACHE = {}


def load(case, tmp_factory):
    """-> dict(rec, m, y0, ops, prj, dir): the recording (events of `same_events_as` where the case stores only its
    files), the model, the replayable operations and the unpacked project directory (settings fixture applied)"""
    if case in _CACHE:
        return _CACHE[case]
    c = refio.WRITER_CASES[case]
    work = tmp_factory.mktemp(case)
    rec = refio.load_recording(case)
    if "same_events_as" in c:
        rec = {**refio.load_recording(c["same_events_as"]), **rec}
    refio.unpack_writer(case, work)
    m, y0 = refio.load_model(c["prj"], work)
    script = refio.writer_script(case, m, y0)
    assert [s[0] for s in script] == rec["script_kind"].tolist() and [s[1] for s in script] == rec["script_t"].tolist()
    rec["script_y"] = np.stack([s[2] for s in script])
    out = dict(rec=rec, m=m, y0=y0, ops=refio.writer_ops(rec), prj=c["prj"], work=str(work), case=case,
               dir=os.path.join(str(work), "input", c["prj"]), files=refio.writer_files(rec))
    _CACHE[case] = out
    return out


def project(L):
    return host.Project(L["dir"], L["prj"], cwd=L["work"])


def same_bits(a, b):
    """equal bit patterns but for NaN payloads: values, signed zeros and the NaN pattern"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all(nan | ((a == b) & (np.signbit(a) == np.signbit(b)))))


def summary(m, y, bc):
    """Model_Data::summary(udata) (MD_update.cpp:190-216): the BC heads are those of the last f() call"""
    keep = m.bc_tables
    m.bc_tables = bc
    try:
        ysf, yus, ygw, yriv = wb_py.host_summary(m, y)
    finally:
        m.bc_tables = keep
    return {"y_surf": ysf, "y_unsat": yus, "y_gw": ygw, "y_riv": yriv}


def replay_oracle(L, rhs):
    """run the recorded schedule through `rhs` (OracleRhs) -> list of operations with results:
       ("f", t, y, dy, diag, et index, bc)     ("x", t, state dict, k, diag of the last f, et index, bc)
    state: summary(y_out) plus y_lake, the lake entries of the last f() input (f_update, MD_update.cpp:175)."""
    rec, m = L["rec"], L["m"]
    nl = getattr(m, "num_lake", 0) or 0
    out, et, bc, diag, last_y = [], None, {}, None, None
    for op in L["ops"]:
        if op[0] == "et":
            et = op[1]
            rhs.set_step_inputs(refio.writer_step(rec, et), bc)
        elif op[0] == "summary":
            out.append(("summary", op[1]))
        elif op[0] == "f":
            _, t, y, j = op
            bc = refio.writer_bc(rec, j)
            if bc:
                rhs.set_step_inputs({}, bc)
            dy, code, _, _ = rhs.eval(t, y)
            assert code == 0
            diag, last_y = rhs.diagnostics(), y
            out.append(("f", t, y, dy, diag, et, bc))
        else:
            _, t, y_out, k = op
            st = summary(m, y_out, bc)
            st["y_lake"] = last_y[m.num_y - nl:].copy() if nl else np.zeros(0)
            out.append(("x", t, st, k, diag, et, bc))
    return out


def export_values(L, arr, col, st, diag, et, k):
    """the array a Print_Ctrl of declaration (arr, col) points at, at ExportResults"""
    rec, m = L["rec"], L["m"]
    NE = m.num_ele
    if arr in ARR_STATE:
        return st[ARR_STATE[arr]]
    if arr in ARR_ET:
        return rec[f"et:{ARR_ET[arr]}"][et]
    if arr in ARR_RN:                                    # the handle has no terrain-radiation arrays: the recording's
        return rec[f"x:{ARR_RN[arr]}"][k]
    lake = np.asarray(m.ilake) > 0 if getattr(m, "ilake", None) is not None else np.zeros(NE, dtype=bool)
    if arr == abi.SHUD_ARR_Q_TRANS:                      # MD_ET.cpp:388; a lake element: MD_ElementFlux.cpp:14
        return np.where(lake, 0.0, diag["q_tg"] + diag["q_tu"])
    if arr == abi.SHUD_ARR_Q_EVAPO:                      # MD_ET.cpp:389; a lake element: qPotEvap (:15)
        return np.where(lake, rec["et:pot_evap"][et], diag["q_eu"] + diag["q_eg"] + diag["q_es"])
    if arr == abi.SHUD_ARR_Q_LAKE_RIVOUT:
        return np.zeros(m.num_lake)                      # zeroed by f_update and never written
    v = diag[ARR_DIAG[arr]]
    return v[col * NE:(col + 1) * NE] if arr in (abi.SHUD_ARR_QELE_SURF, abi.SHUD_ARR_QELE_SUB) else v


def restate_outputs(L, trace, outdir, ctl_cls=PrintCtrlPy):
    """every Print_Ctrl file from the project's own output plan (shud_project_outputs) -> (decl, control)"""
    P = project(L)
    c = P.control()
    decl = P.outputs(str(outdir))
    ctl = [ctl_cls(d["basename"], d["n_all"], d["interval"], d["iflux"], start_time=c["forc_start_time"],
                   flag_io=d["flag_io"], binary=bool(c["binary"]), ascii=bool(c["ascii"]), **header_kw(c))
           for d in decl]
    for op in trace:
        if op[0] != "x":
            continue
        _, t, st, k, diag, et, _ = op
        for d, p in zip(decl, ctl):
            p.print_data(export_values(L, d["array"], d["column"], st, diag, et, k), t)
    for p in ctl:
        p.close()
    P.close()
    return decl, c


def flood_calls(trace):
    return [(op[1], op[2]["y_riv"], op[4]["qriv_down"]) for op in trace if op[0] == "x"]


def ic_schedule(L, trace):
    """the PrintInit calls of SHUD(): (kind, t, arrays) with arrays = (is, snow, surf, unsat, gw, riv, lake):
    .bak at 0 before the loop, .update at the top of every solver step and after the loop"""
    rec = L["rec"]
    x0 = {k: rec[f"x0:{k}"][0] for k in refio.W_SUMMARY_KEYS}
    cur = (rec["ic_is"], rec["ic_snow"], x0["y_surf"], x0["y_unsat"], x0["y_gw"], x0["y_riv"], x0["y_lake"])
    t = float(rec["dims"][4])
    calls = [("bak", 0.0, cur), ("update", t, cur)]
    for op in trace:
        if op[0] == "x":
            _, t, st, k, _, et, _ = op
            cur = (rec["et:y_is"][et], rec["et:y_snow"][et], st["y_surf"], st["y_unsat"], st["y_gw"], st["y_riv"],
                   st["y_lake"])
            calls.append(("update", t, cur))
    return calls


def restate_ic_files(L, trace, due=mon_py.ic_due, ic_file=mon_py.ic_file):
    """{file name: bytes} of the numbered restart-file copies the driver left"""
    step = int(L["rec"]["control"][3])
    out, n = {}, 0
    for kind, t, a in ic_schedule(L, trace):
        if due(t, step):
            out[f"{L['prj']}.cfg.ic.{kind}.{n}"] = ic_file(t, *a[:6], a[6] if len(a[6]) else None)
            n += 1
    return out


def restate_wb(L, trace, prefix, order="seq", wb_cls=wb_py.WaterBalancePy, quad_cls=wb_quad_py.QuadMonitorPy,
               environ=None):
    """the water-balance files of the recorded run through wb_py / wb_quad_py -> (restatement, quad or None)"""
    rec, m = L["rec"], L["m"]
    env = refio.WRITER_CASES[L["case"]]["env"] if environ is None else environ
    assert wb_py.env_truthy(env.get("SHUD_WB_DIAG"))
    P = project(L)
    c = P.control()
    interval = P.wb_interval()
    P.close()
    hdr = dict(forc_start_time=c["forc_start_time"], **header_kw(c))
    x0 = {k: rec[f"x0:{k}"][0] for k in refio.W_SUMMARY_KEYS}
    t0 = float(rec["dims"][4])
    state0 = (x0["y_surf"], x0["y_unsat"], x0["y_gw"], x0["y_riv"], rec["ic_snow"], rec["ic_is"])
    keep = m.bc_tables
    wb = wb_cls(m, interval, state0, start_time=t0, trapz=wb_py.env_truthy(env.get("SHUD_WB_DIAG_TRAPZ")),
                prefix=prefix, order=order, **hdr)
    quad = None
    if wb_py.env_truthy(env.get("SHUD_WB_DIAG_QUAD")):
        quad = quad_cls(wb, start_time=t0, prefix=prefix, **hdr)
    et_seen, y_out, after_summary = None, None, False
    try:
        for op in trace:
            if op[0] == "summary":
                after_summary = True
            elif op[0] == "f":
                _, t, y, dy, diag, et, bc = op
                m.bc_tables = bc
                if et != et_seen:                        # onETUpdate: qEleE_IC right after ET()
                    wb.on_et_update(rec["et:e_ic"][et])
                    et_seen = et
                if after_summary:                        # the f() of shud.cpp:141, then sample(t, DY)
                    last = (t, dy, diag, et)
                elif quad is not None:                   # a CV_ONE_STEP return: f(), onCvodeMonitorStep(t)
                    quad.step(t, wb_quad_py.quad_rates(m, wb.ic_raw, diag, rec["et:prcp"][et], order=order))
            elif op[0] == "x":
                _, t, st, k, _, et, bc = op
                m.bc_tables = bc
                ts, dy, diag, et_s = last
                wb.sample(ts, dy, diag, rec["et:prcp"][et_s], rec["et:net_prep"][et_s], st["y_riv"])
                state = (st["y_surf"], st["y_unsat"], st["y_gw"], st["y_riv"], rec["et:y_snow"][et],
                         rec["et:y_is"][et])
                (quad or wb).maybe_write(t, state)
                after_summary = False
    finally:
        m.bc_tables = keep
    wb.close()
    if quad is not None:
        quad.close()
    return wb, quad, interval


def dat_rows(raw):
    """(header bytes, icol, t [rows], data [rows, numvar]) of a .dat file's bytes"""
    nv = int(np.frombuffer(raw, np.float64, 1, 1032)[0])
    off = 1040 + 8 * nv
    body = np.frombuffer(raw, np.float64, (len(raw) - off) // 8, off).reshape(-1, nv + 1)
    return raw[:off], np.frombuffer(raw, np.float64, nv, 1040), body[:, 0], body[:, 1:]
