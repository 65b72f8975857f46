"""TEST INFRASTRUCTURE ONLY — runs the reference binaries of oracle/_ref/ (built by `make -C oracle ref` where a
reference checkout exists) as child processes and reads their dumps; defines the pinned cases and the layout of
the recordings under tests/golden/ref/.  Used by oracle/ref/record.py and the CPU tests tests/test_ref_pin.py,
tests/test_kat.py, tests/test_et.py.  GPU tests read the recordings only (load_recording)."""
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


def live_status(what):
    """-> True where the reference binaries exist.  Either way the outcome is visible in the test output: a line
    on stdout when the live comparison runs, a warning (pytest lists it in its summary) when it does not."""
    if have_ref():
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
def unpack(prj, workdir, para=None, calib=None):
    """<workdir>/input/<prj>/ as the reference expects it: the committed archive of ccw / qhh / heihe, or the
    synthetic BC project "syn".  para: a replacement <prj>.cfg.para (file path).  -> the input directory"""
    d = os.path.join(str(workdir), "input", prj)
    if prj == "syn":
        from shud_rhs import synth
        synth.write_project(d, "syn", SYN_N, days=1.0, max_step=30.0, et_step=10.0, dt_out=60, bc=True)
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
    if prj in END_DAY:
        # the archives' forcing series are trimmed to 240 rows; the reference refuses (exit 13, "Forcing data
        # coverage is insufficient") a run whose END lies past them, so END is moved inside the kept rows
        with open(pp) as f:
            lines = [ln for ln in f.read().splitlines() if ln.split() and ln.split()[0].upper() != "END"]
        with open(pp, "w") as f:
            f.write("\n".join(lines + [f"END\t{END_DAY[prj]}"]) + "\n")
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
