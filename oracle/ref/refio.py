"""TEST INFRASTRUCTURE ONLY — runs the reference binaries of oracle/_ref/ (built by `make -C oracle ref` where a
reference checkout exists) as child processes and reads their dumps; defines the pinned cases and the layout of
the recordings under tests/golden/ref/.  Used by oracle/ref/record.py and the CPU tests tests/test_ref_pin.py,
tests/test_ref_pin_writers.py, tests/test_kat.py, tests/test_et.py.  GPU tests read the recordings only
(load_recording) and rebuild the scripted states (writer_script)."""
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.dirname(HERE)
ROOT = os.path.dirname(ORACLE)
REF_DIR = os.path.join(ORACLE, "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden")
REC_DIR = os.path.join(GOLDEN, "ref")
MAX_BYTES = 441499                       # the largest fixture committed before the recordings (qhh_model.npz)
BIN = {0: os.path.join(REF_DIR, "shud_ref_f"), 1: os.path.join(REF_DIR, "shud_ref_f_omp")}   # by SHUD_MODE_*
KAT_LIB = os.path.join(REF_DIR, "libshud_ref_kat.so")
STEP_KEYS = ["net_prep", "pot_evap", "pot_tran", "etp", "lai", "fu_surf", "fu_sub", "e_ic", "u_satn", "ugw_stale",
             "prcp"]
BC_KEYS = ["ele_ybc", "ele_qbc", "riv_ybc", "riv_qbc"]
ET_KEYS = ["qEleNetPrep", "qPotEvap", "qPotTran", "qEleETP", "t_lai", "fu_surf", "fu_sub", "yEleIS", "yEleSnow",
           "qEleE_IC"]
END_DAY = {"ccw": 9, "qhh": 29, "heihe": 239}      # inside the 240 forcing rows each archive keeps
SYN_N = 2000                            # the synthetic BC project (the size tests/test_gpu_host.py uses)

sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))


def have_ref():
    return all(os.path.exists(p) for p in (BIN[0], BIN[1], KAT_LIB))


def have_writer_ref():
    """the driver under oracle/_ref/ has mode w (its usage line says so).  Binaries built from an older driver, e.g.
    carried over to a machine without a reference checkout to rebuild them from, count as not there."""
    if not have_ref():
        return False
    r = subprocess.run([BIN[0]], capture_output=True, text=True, timeout=60)
    return "f|et|w" in r.stderr


def live_status(what, have=None):
    """-> True where the reference binaries exist.  Either way the outcome is visible in the test output: a line
    on stdout when the live comparison runs, a warning (pytest lists it in its summary) when it does not."""
    if (have or have_ref)():
        print(f"REFPIN live comparison RAN: {what}")
        return True
    import warnings
    warnings.warn(f"REFPIN live comparison NOT RUN (no reference binaries under oracle/_ref/): {what}")
    return False


def read_dump(path):
    """the driver's records -> list of (name, float64 array), in file order"""
    raw = open(path, "rb").read()
    out, off = [], 0
    while off < len(raw):
        name = raw[off:off + 16].split(b"\0", 1)[0].decode()
        n = int(np.frombuffer(raw, np.int64, 1, off + 16)[0])
        out.append((name, np.frombuffer(raw, np.float64, n, off + 24).copy()))
        off += 24 + 8 * n
    return out


# ---- projects -------------------------------------------------------------------------------------------------
def unpack(prj, workdir, para=None, calib=None, end=None, cfg_output=False):
    """<workdir>/input/<prj>/ as the reference expects it: the committed archive of ccw / qhh / heihe, or the
    synthetic BC project "syn".  para: a replacement <prj>.cfg.para (file path); end: its END [day] (default: the
    last day the archive's forcing covers); cfg_output: the synthetic project gets a .cfg.output column mask.
    -> the input directory"""
    d = os.path.join(str(workdir), "input", prj)
    if prj == "syn":
        from shud_rhs import synth
        synth.write_project(d, "syn", SYN_N, days=1.0, max_step=30.0, et_step=10.0, dt_out=60, bc=True,
                            cfg_output=cfg_output)
        # the reference resolves the forcing csv against the path line of .tsd.forc
        with open(os.path.join(d, "syn.tsd.forc")) as f:
            lines = f.read().splitlines()
        lines[1] = "./input/syn/"
        with open(os.path.join(d, "syn.tsd.forc"), "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        with zipfile.ZipFile(os.path.join(GOLDEN, "input", f"{prj}.zip")) as z:
            z.extractall(str(workdir))
    pp = os.path.join(d, f"{prj}.cfg.para")
    if para is not None:
        with open(para) as f, open(pp, "w") as g:
            g.write(f.read())
    if calib is not None:
        with open(calib) as f, open(os.path.join(d, f"{prj}.cfg.calib"), "w") as g:
            g.write(f.read())
    if prj in END_DAY or end is not None:
        # the archives' forcing series are trimmed to 240 rows; the reference refuses (exit 13, "Forcing data
        # coverage is insufficient") a run whose END lies past them, so END is moved inside the kept rows
        with open(pp) as f:
            lines = [ln for ln in f.read().splitlines() if ln.split() and ln.split()[0].upper() != "END"]
        with open(pp, "w") as f:
            f.write("\n".join(lines + [f"END\t{END_DAY[prj] if end is None else end}"]) + "\n")
    return d


def load_model(prj, workdir=None):
    """-> (ShudModel, y0) of a pinned project: the committed fixtures, or the synthetic project read back by
    shudio (the same deterministic files the reference was run on)."""
    from shud_rhs import ShudModel, shudio
    if prj != "syn":
        return (ShudModel.load(os.path.join(GOLDEN, f"{prj}_model.npz")),
                np.load(os.path.join(GOLDEN, f"{prj}_y0.npy")))
    d = os.path.join(str(workdir), "input", "syn")
    if not os.path.exists(os.path.join(d, "syn.sp.mesh")):
        unpack("syn", workdir)
    m, ex = shudio.load_project(d, "syn")
    return m, ex["y0"]


# ---- the pinned RHS cases: (project, number of ET steps run before f, states) ------------------------------------
# states: "ic" = the initial condition, an int = workload.random_state(m, seed).  A state listed twice in a row
# shows the carried qEleE_IC / u_satn of the serial f (the second call differs from the first, the third not).
RHS_CASES = {
    "ccw_ic":   ("ccw", 1, ["ic", "ic", "ic", 101, 101, 102, 103]),
    "ccw_et":   ("ccw", None, ["ic", 104, 104, 105]),        # a later ET step (n_et below: first wet hour)
    "qhh_ic":   ("qhh", 1, ["ic", "ic", "ic"]),              # lakes on: serial mode only (the OMP f has no lake)
    "heihe_ic": ("heihe", 1, ["ic", "ic", 301, 301]),
    "syn_ic":   ("syn", 1, ["ic", "ic", 201, 201, 202]),
    "syn_et":   ("syn", None, ["ic", 203, 203]),
}
# ccw: 68 hourly ET steps, t = 4020 min, a wet hour after earlier rain (net_prep, prcp and e_ic all non-zero);
# syn: 63 ten-minute steps, t = 620 min, a wet daylight hour with the BC tables on their 11th row
N_ET_LATER = {"ccw_et": 68, "syn_et": 63}
MODES = {"ccw_ic": (0, 1), "ccw_et": (0, 1), "qhh_ic": (0,), "heihe_ic": (0, 1),
         "syn_ic": (0, 1), "syn_et": (0, 1)}


def case_states(case, m, y0):
    from shud_rhs import workload
    return [y0.copy() if s == "ic" else workload.random_state(m, seed=s) for s in RHS_CASES[case][2]]


def run_ref(mode, kind, workdir, prj, n_et, states=None, threads=1):
    """run shud_ref_f / shud_ref_f_omp in `workdir` (which holds input/<prj>/) -> list of records"""
    out = os.path.join(str(workdir), f"ref_{kind}_{mode}.bin")
    sp = "-"
    if states is not None:
        sp = os.path.join(str(workdir), f"states_{mode}.bin")
        np.ascontiguousarray(np.stack(states), dtype=np.float64).tofile(sp)
    # the driver sets the reference's CS.num_threads to `threads` itself (the .cfg.para's NUM_OPENMP would win
    # over -n and OMP_NUM_THREADS otherwise) and dumps the team size it really got as "threads"
    r = subprocess.run([BIN[mode], kind, out, sp, str(n_et), str(threads), prj], cwd=str(workdir),
                       capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(f"{BIN[mode]} {prj}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return read_dump(out)


def run_rhs_case(case, mode, workdir):
    """-> dict of arrays: y0, t, the step inputs, BC rows, states [K, NY], dy [K, NY]"""
    prj, n_et, _ = RHS_CASES[case]
    n_et = N_ET_LATER[case] if n_et is None else n_et
    if not os.path.exists(os.path.join(str(workdir), "input", prj)):
        unpack(prj, workdir)
    m, y0 = load_model(prj, workdir)
    states = case_states(case, m, y0)
    d = dict(run_ref(mode, "f", workdir, prj, n_et, states))
    k = int(d.pop("ncalls")[0])
    assert k == len(states)
    rec = {key: d[key] for key in ["dims", "threads", "y0", "t"] + STEP_KEYS + [b for b in BC_KEYS if b in d]}
    rec["dy"] = np.stack([d[f"dy{i}"] for i in range(k)])
    rec["states"] = np.stack(states)
    return rec


# ---- the ET prelude against the reference: ccw with the cryosphere on and short day-mean queues ------------------
# settings-only fixtures: CRYOSPHERE 1, LSM_STEP 330 (.cfg.para); Fzn_surfday 2, Fzn_subday 3 and freeze
# thresholds inside ccw's January temperatures (.cfg.calib).  22 ET steps of 330 min: the queues are pushed at
# steps 0, 5, 10, 15, 20, so the surface queue (2 days) pops three times and the subsurface queue (3 days) twice.
ET_PARA = os.path.join(REC_DIR, "ccw_cryo.cfg.para")
ET_CALIB = os.path.join(REC_DIR, "ccw_cryo.cfg.calib")
ET_STEPS = 22
ET_STRIDE = 3                            # the recording keeps every third element (ET is element-local)


def unpack_et(workdir):
    return unpack("ccw", workdir, para=ET_PARA, calib=ET_CALIB)


def run_et_case(workdir, stride=ET_STRIDE):
    """-> dict: t [ET_STEPS], ic_is, ic_snow and per ET_KEYS an array [ET_STEPS, NE // stride (rounded up)]"""
    if not os.path.exists(os.path.join(str(workdir), "input", "ccw")):
        unpack_et(workdir)
    recs = run_ref(0, "et", workdir, "ccw", ET_STEPS)
    d = dict(recs[:5])
    out = {"dims": d["dims"], "threads": d["threads"], "ic_is": d["ic_is"], "ic_snow": d["ic_snow"],
           "t": np.array([v[0] for k, v in recs if k == "t"])}
    for key in ET_KEYS + ["t_temp", "t_prcp", "rn_factor"]:
        out[key] = np.stack([v[::stride] for k, v in recs if k == key])
        assert out[key].shape[0] == ET_STEPS
    return out


# ---- recordings: tests/golden/ref/<name>.npz, split per array where one file would pass MAX_BYTES ----------------
def save_recording(name, rec):
    os.makedirs(REC_DIR, exist_ok=True)
    for f in os.listdir(REC_DIR):
        if f == name + ".npz" or f.startswith(name + ".part"):
            os.remove(os.path.join(REC_DIR, f))
    path = os.path.join(REC_DIR, name + ".npz")
    np.savez_compressed(path, **rec)
    if os.path.getsize(path) <= MAX_BYTES:
        return [path]
    os.remove(path)
    paths, part, items = [], {}, []
    for key, v in rec.items():                       # 2-D arrays (dy, states) go row by row
        v = np.asarray(v)
        items += [(f"{key}@{i}", v[i]) for i in range(v.shape[0])] if v.ndim == 2 else [(key, v)]

    def flush():
        p = os.path.join(REC_DIR, f"{name}.part{len(paths)}.npz")
        np.savez_compressed(p, **part)
        assert os.path.getsize(p) <= MAX_BYTES, p
        paths.append(p)
        part.clear()

    size = 0
    for key, v in items:
        if part and size + v.nbytes > MAX_BYTES * 0.9:     # uncompressed bound: compressed is never larger by much
            flush()
            size = 0
        part[key] = v
        size += v.nbytes
    if part:
        flush()
    return paths


def load_recording(name):
    files = sorted(f for f in os.listdir(REC_DIR) if f == name + ".npz" or f.startswith(name + ".part"))
    if not files:
        raise FileNotFoundError(f"no recording {name} under {REC_DIR}")
    flat = {}
    for f in files:
        with np.load(os.path.join(REC_DIR, f), allow_pickle=False) as z:
            flat.update({k: z[k] for k in z.files})
    rec, rows = {}, {}
    for k, v in flat.items():
        if "@" in k:
            key, i = k.split("@")
            rows.setdefault(key, {})[int(i)] = v
        else:
            rec[k] = v
    for key, r in rows.items():
        rec[key] = np.stack([r[i] for i in range(len(r))])
    return rec


def rhs_name(case, mode):
    return f"{case}_f_{'omp' if mode else 'serial'}"


def step_and_bc(rec):
    """(step dict, bc_tables dict) of an RHS recording, as OracleRhs / RhsHandle.set_step_inputs take them"""
    return {k: rec[k] for k in STEP_KEYS}, {k: rec[k] for k in BC_KEYS if k in rec}


# ---- leaf equations ----------------------------------------------------------------------------------------------
def ref_kat_child(ids_and_grids):
    """ref_kat over {name: (id, x[n, k])} in a child process (the reference's leaves may exit()) -> {name: out}"""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        np.savez(os.path.join(tmp, "in.npz"), **{f"{k}@{i}": x for k, (i, x) in ids_and_grids.items()})
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "kat", tmp], capture_output=True, text=True,
                           timeout=300)
        if r.returncode != 0:
            raise RuntimeError(f"ref_kat child: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        with np.load(os.path.join(tmp, "out.npz")) as z:
            return {k: z[k] for k in z.files}


def _kat_main(tmp):
    import ctypes as C
    lib = C.CDLL(KAT_LIB)
    lib.ref_kat.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
    lib.ref_kat.restype = C.c_int
    out = {}
    with np.load(os.path.join(tmp, "in.npz")) as z:
        for key in z.files:
            name, fn = key.split("@")
            x = np.ascontiguousarray(z[key], dtype=np.float64)
            assert lib.ref_kat_nin(int(fn)) == x.shape[1], key
            o = np.zeros(x.shape[0])
            assert lib.ref_kat(int(fn), x.ctypes.data, x.shape[0], o.ctypes.data) == 0
            out[name] = o
    np.savez(os.path.join(tmp, "out.npz"), **out)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "kat":
    _kat_main(sys.argv[2])


# ---- output writers, monitors and water balance: driver mode w ---------------------------------------------------
# SHUD()'s whole loop with CVODE replaced by a script of states (shud_ref_driver.cpp).  The files the reference
# wrote into its output directory are stored byte for byte ("file:<name>", uint8), next to the events the driver
# dumped: per ET() call the step inputs ("et:<key>" [n_et, NumEle]), per f() call its time and BC rows, per
# ExportResults the arrays the reference then held ("x:<key>" [n_x, n]).  Settings-only fixtures: <case>.cfg.para.
EV_ET, EV_F, EV_X = 0, 1, 2
W_ET_KEYS = STEP_KEYS + ["y_is", "y_snow"]
W_SUMMARY_KEYS = ["y_surf", "y_unsat", "y_gw", "y_riv", "y_lake"]
W_FLUX_KEYS = ["qele_surf", "qele_sub", "qele_surf_tot", "qele_sub_tot", "q_infil", "q_exfil", "q_recharge", "q_es",
               "q_eu", "q_eg", "q_tu", "q_tg", "q_eta", "q_trans", "q_evapo", "e_ic_f", "u_satn_f", "qe2r_surf",
               "qe2r_sub", "qriv_down", "qriv_up", "qriv_surf", "qriv_sub", "q_lake_surf", "q_lake_sub",
               "q_lake_rivin", "q_lake_rivout", "q_lake_evap", "q_lake_prcp", "lake_toparea"]
W_RN_KEYS = ["rn_h", "rn_t", "rn_factor"]
W_X_KEYS = W_SUMMARY_KEYS + W_FLUX_KEYS + W_RN_KEYS
# dumped flux array -> OracleRhs.diagnostics() name (identical unless listed)
W_DIAG_NAME = {"e_ic_f": "e_ic", "u_satn_f": "u_satn"}
W_NOT_IN_DIAG = ["q_trans", "q_evapo", "q_lake_rivout"]          # sums / negations the tests restate
# qhh keeps the arrays the lake outputs and the restart file's lake block need (4773 elements: size)
QHH_X_KEEP = W_SUMMARY_KEYS + ["qriv_down", "qriv_up", "qriv_surf", "qriv_sub", "q_lake_surf", "q_lake_sub",
                               "q_lake_rivin", "q_lake_rivout", "q_lake_evap", "q_lake_prcp", "lake_toparea",
                               "qele_surf_tot", "qele_sub_tot", "q_eta", "q_trans", "q_evapo", "e_ic_f"] + W_RN_KEYS
WRITER_CASES = {
    # name: project, .cfg.para fixture, END [day], environment, script, solver steps; keep: the x keys kept (default
    # all); files "wb": only the water-balance files are kept (the others are ccw_w's business)
    "ccw_w": dict(prj="ccw", para="ccw_w.cfg.para", end=0.25, env={}, script="ccw_nonfinite", steps=6),
    "ccw_wb": dict(prj="ccw", para="ccw_wb.cfg.para", end=0.25, env={"SHUD_WB_DIAG": "1"}, script="ccw", steps=6,
                   keep=W_SUMMARY_KEYS, files="wb"),
    "ccw_wb_trapz": dict(prj="ccw", para="ccw_wb.cfg.para", end=0.25,
                         env={"SHUD_WB_DIAG": "1", "SHUD_WB_DIAG_TRAPZ": "1"}, script="ccw", steps=6,
                         keep=W_SUMMARY_KEYS, files="wb", same_events_as="ccw_wb"),
    "ccw_wb_quad": dict(prj="ccw", para="ccw_wb.cfg.para", end=0.25,
                        env={"SHUD_WB_DIAG": "1", "SHUD_WB_DIAG_TRAPZ": "1", "SHUD_WB_DIAG_QUAD": "on"},
                        script="ccw_quad", steps=6, keep=W_SUMMARY_KEYS, files="wb"),
    "syn_w": dict(prj="syn", para="syn_w.cfg.para", end=0.17, env={"SHUD_WB_DIAG": "true"}, script="syn", steps=4),
    "qhh_w": dict(prj="qhh", para="qhh_w.cfg.para", end=1.09, env={}, script="qhh", steps=2, keep=QHH_X_KEEP),
}
WB_ENV = ("SHUD_WB_DIAG", "SHUD_WB_DIAG_TRAPZ", "SHUD_WB_DIAG_QUAD")


def _over_bank(m, y, frac, seed):
    """y with a fraction `frac` of the reaches above their bank depth and the rest below it"""
    NE, NR = m.num_ele, m.num_riv
    rng = np.random.default_rng(seed)
    depth = m.riv["riv_depth"]
    over = rng.random(NR) < frac
    y = y.copy()
    y[3 * NE:3 * NE + NR] = np.where(over, depth + rng.uniform(0.01, 0.5, NR), np.minimum(y[3 * NE:3 * NE + NR], 0.5 * depth))
    return y


def writer_script(case, m, y0):
    """the scripted solver of a WRITER_CASES entry -> list of (kind, t, y): kind 0 a CVode(CV_NORMAL) return, 2 a
    CV_ONE_STEP return, 1 the state handed to summary().  Solver steps of 60 min from StartTime T0:
      step 1  two returns inside the step (T0+59.9995, then T0+60.4: floor(t + 0.001) and (long)t off the grid),
              y_out differs from the last RHS input, one reach exactly at its bank depth (the flood test is `>`)
      step 2  t = T0+120 - 5e-11 (inside ZERO of the step's end: floor(t) = 119 but floor(t + 0.001) = 120)
      step 3  y_out differs; "nonfinite" scripts put nan, -nan, inf and -inf into four river stages
      step 4  the return overshoots to T0+300; no reach above its bank
      step 5  nothing to integrate (t is already T0+300): summary on a new state, the same t exported twice
      step 6  t = T0+360"""
    from shud_rhs import workload
    kind = WRITER_CASES[case]["script"]
    NE, NR = m.num_ele, m.num_riv
    if kind == "qhh":
        rng = np.random.default_rng(77)
        nl = m.num_lake

        def wiggle(dlake):
            y = y0 * (1.0 + 0.01 * rng.uniform(-1, 1, y0.size))
            y[-nl:] = y0[-nl:] + dlake
            return y
        a, b, c = wiggle(0.0), wiggle(0.37), wiggle(-0.21)
        return [(0, 1500.0, a), (1, 0.0, b), (0, 1560.0, c), (1, 0.0, c)]
    rs = lambda s: workload.random_state(m, seed=s)                            # noqa: E731
    if kind == "syn":
        # LSM_STEP 30 under a solver step of 60: two CVode returns per step (the ET sub-step rule); y_out differs
        # from the last RHS input on every other step; some reaches over their bank
        out = []
        for k in range(4):
            a, b = rs(500 + 2 * k), _over_bank(m, rs(501 + 2 * k), 0.2, 20 + k)
            out += [(0, 60.0 * k + 30.0, a), (0, 60.0 * k + 60.0, b),
                    (1, 0.0, _over_bank(m, rs(520 + k), 0.2, 30 + k) if k % 2 == 0 else b)]
        return out
    A, B, C, D, E = rs(401), _over_bank(m, rs(402), 0.3, 1), _over_bank(m, rs(403), 0.3, 2), \
        _over_bank(m, rs(404), 0.2, 3), rs(405)
    F, G, H, I = _over_bank(m, rs(406), 0.3, 4), _over_bank(m, rs(407), 0.0, 5), _over_bank(m, rs(408), 0.3, 6), \
        _over_bank(m, rs(409), 0.1, 7)
    C[3 * NE] = m.riv["riv_depth"][0]
    if kind == "ccw_nonfinite":
        F[3 * NE + 1:3 * NE + 5] = [np.nan, np.copysign(np.nan, -1.0), np.inf, -np.inf]
    if kind == "ccw_quad":
        out, subs = [], [(7.3, 21.9, 48.25, 60.0), (11.0, 60.0 - 1e-3, 60.0), (0.5, 1.0, 30.0, 60.0)]
        states = [A, B, D, E, G, I]
        for k in range(6):
            for j, dt in enumerate(subs[k % 3]):
                out.append((2, 60.0 * k + dt, 0.5 * (states[k] + states[(k + j) % 6])))
            out.append((1, 0.0, (C, D, F, G, H, I)[k]))
        return out
    return [(0, 59.9995, A), (0, 60.4, B), (1, 0.0, C), (0, 120.0 - 5e-11, D), (1, 0.0, D), (0, 180.0, E),
            (1, 0.0, F), (0, 300.0, G), (1, 0.0, G), (1, 0.0, H), (0, 360.0, I), (1, 0.0, I)]


def unpack_writer(case, workdir):
    c = WRITER_CASES[case]
    para = os.path.join(REC_DIR, c["para"])
    if c["prj"] == "syn":
        return unpack("syn", workdir, para=para, cfg_output=True, end=c["end"])
    return unpack(c["prj"], workdir, para=para, end=c["end"])


def run_writer_case(case, workdir):
    """run the driver's mode w in `workdir` -> the recording (dict of arrays)"""
    import shutil
    c = WRITER_CASES[case]
    prj = c["prj"]
    shutil.rmtree(os.path.join(str(workdir), "output"), ignore_errors=True)
    unpack_writer(case, workdir)
    m, y0 = load_model(prj, workdir)
    script = writer_script(case, m, y0)
    sp = os.path.join(str(workdir), "script.bin")
    with open(sp, "wb") as f:
        for kind, t, y in script:
            np.concatenate([[float(kind), float(t)], y]).astype(np.float64).tofile(f)
    out = os.path.join(str(workdir), "ref_w.bin")
    env = {k: v for k, v in os.environ.items() if k not in WB_ENV}
    env.update(c["env"])
    r = subprocess.run([BIN[0], "w", out, sp, "0", "1", prj], cwd=str(workdir), capture_output=True, text=True,
                       timeout=600, env=env)
    if r.returncode != 0:
        raise RuntimeError(f"{BIN[0]} w {case}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    recs = read_dump(out)
    head = dict(recs[:7])
    if "wb_flags" not in head:
        raise RuntimeError(f"{BIN[0]} has no mode w: it was built from an older oracle/ref/shud_ref_driver.cpp; "
                           "run `make -C oracle`")
    rec = {k: head[k] for k in ("dims", "threads", "ic_is", "ic_snow", "wb_flags", "control")}
    assert int(rec["control"][0]) == c["steps"], rec["control"]
    keep = c.get("keep")
    ev_kind, ev_t, groups, cur = [], [], {}, None
    for name, v in recs:
        if name in ("ev_et", "ev_f", "ev_x", "ev_x0"):
            cur = {"ev_et": "et", "ev_f": "f", "ev_x": "x", "ev_x0": "x0"}[name]
            if name != "ev_x0":
                ev_kind.append({"et": EV_ET, "f": EV_F, "x": EV_X}[cur])
                ev_t.append(v[0])
        elif cur is not None and name not in ("ic_copies",):
            if cur == "x" and keep is not None and name not in keep + ["flood"]:
                continue
            groups.setdefault(f"{cur}:{name}", []).append(v)
    rec["ev_kind"], rec["ev_t"] = np.array(ev_kind, dtype=np.int64), np.array(ev_t)
    for k, rows in groups.items():
        rec[k] = np.stack(rows)
    rec["script_kind"] = np.array([s[0] for s in script], dtype=np.int64)
    rec["script_t"] = np.array([s[1] for s in script])
    rec["script_y"] = np.stack([s[2] for s in script])
    if "same_events_as" in c:                      # only the files differ: the events are the other case's
        rec = {k: v for k, v in rec.items() if k.startswith("file:") or k in ("wb_flags", "control")}
    outdir = os.path.join(str(workdir), "output", f"{prj}.out")
    wb_only = c.get("files") == "wb"
    for fn in sorted(os.listdir(outdir)):
        if fn.endswith((".cfg.ic.bak", ".cfg.ic.update", ".time.csv")):
            continue                               # the restart files are kept as the numbered copies
        if wb_only and "wb" not in fn.split(".")[1]:
            continue
        if fn.endswith((".dat", ".csv")) or ".cfg.ic." in fn:
            rec[f"file:{fn}"] = np.frombuffer(open(os.path.join(outdir, fn), "rb").read(), dtype=np.uint8)
    return rec


def writer_files(rec):
    """{file name: bytes} of a writers recording"""
    return {k[5:]: v.tobytes() for k, v in rec.items() if k.startswith("file:")}


def writer_ops(rec):
    """the recorded run as a list of operations, in order:
       ("et", i)              step inputs et:*[i] become current (ET() returned)
       ("f", t, y, j)         f(t, y) with the BC rows f:*[j]
       ("x", t, y_out, k)     summary(y_out) was made before the f of a water-balance run; ExportResults(t), x:*[k]"""
    ops, si, n = [], 0, {EV_ET: 0, EV_F: 0, EV_X: 0}
    kind, ty, yy = rec["script_kind"], rec["script_t"], rec["script_y"]
    y_out = None
    for ek, et_ in zip(rec["ev_kind"], rec["ev_t"]):
        ek = int(ek)
        if ek == EV_ET:
            ops.append(("et", n[ek]))
        elif ek == EV_F:
            if kind[si] == 1:
                y_out = yy[si]
                ops.append(("summary", y_out))
            else:
                assert ty[si] == et_
            ops.append(("f", float(et_), yy[si], n[ek]))
            si += 1
        else:
            if y_out is None:
                assert kind[si] == 1
                y_out = yy[si]
                ops.append(("summary", y_out))
                si += 1
            ops.append(("x", float(et_), y_out, n[ek]))
            y_out = None
        n[ek] += 1
    assert si == len(kind)
    return ops


def writer_step(rec, i):
    return {k: rec[f"et:{k}"][i] for k in STEP_KEYS}


def writer_bc(rec, j):
    return {k: rec[f"f:{k}"][j] for k in BC_KEYS if f"f:{k}" in rec}
