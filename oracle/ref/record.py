"""Regenerate the recordings under tests/golden/ref/ from the reference binaries of oracle/_ref/ (built by
`make -C oracle` where a reference checkout exists): run on the unpacked tests/golden/input/*.zip archives and on
the synthetic BC project, each in a temporary directory.  The recordings are data the reference's programs wrote;
the tests compare against them on machines without the binaries, and against a fresh run where they exist.

    python oracle/ref/record.py            # everything
    python oracle/ref/record.py rhs|kat|et|writers

Every run uses a team of 1 thread: the driver overrides the reference's CS.num_threads (the archives' .cfg.para
carry NUM_OPENMP 8, which would win over -n and OMP_NUM_THREADS) and dumps the team size it observed, which is
stored as `threads`.  More threads are not used: f_applyDY_omp shares its scratch variables across the team."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests"))
import refio  # noqa: E402


def record_rhs():
    for case, modes in refio.MODES.items():
        with tempfile.TemporaryDirectory() as tmp:
            for mode in modes:
                rec = refio.run_rhs_case(case, mode, tmp)
                assert rec["threads"][0] == 1.0, rec["threads"]
                if refio.RHS_CASES[case][0] == "qhh":
                    del rec["states"]                       # the initial condition only: tests/golden/qhh_y0.npy
                paths = refio.save_recording(refio.rhs_name(case, mode), rec)
                print(case, mode, [f"{os.path.basename(p)} {os.path.getsize(p)}" for p in paths])


def record_kat():
    from kat_grids import ET_KAT, KAT, grid
    ids = {**KAT, **ET_KAT}
    out = refio.ref_kat_child({n: (ids[n], grid(n)) for n in ids})
    paths = refio.save_recording("kat", out)
    print("kat", [f"{os.path.basename(p)} {os.path.getsize(p)}" for p in paths])


def record_et():
    with tempfile.TemporaryDirectory() as tmp:
        rec = refio.run_et_case(tmp)
        paths = refio.save_recording("ccw_et_prelude", rec)
        print("et", [f"{os.path.basename(p)} {os.path.getsize(p)}" for p in paths])


def record_writers():
    """SHUD()'s loop with a scripted solver: output files, restart files, flood file, water-balance files"""
    full = {}
    for case, c in refio.WRITER_CASES.items():
        with tempfile.TemporaryDirectory() as tmp:
            rec = full[case] = refio.run_writer_case(case, tmp)
        files = refio.writer_files(rec)
        prj = c["prj"]
        if "same_events_as" in c:
            assert set(rec) <= set(full[c["same_events_as"]])
        else:
            flood, nriv = rec["x:flood"][:, 0], int(rec["dims"][2])
            if case in ("ccw_w", "syn_w"):
                # the flood file: some calls with rows for some reaches but not all, one call with none
                rows = np.array([ln.split(b"\t")[0] for ln in files[f"{prj}.flood.csv"].split(b"\n")[1:] if ln])
                per_call = [int((rows == (b"%.1f" % t)).sum()) for t in rec["ev_t"][rec["ev_kind"] == refio.EV_X]]
                assert any(0 < n < nriv for n in per_call), per_call
                if case == "ccw_w":
                    assert (flood == 0).any() and b"-nan" in files["ccw.flood.csv"] + files["ccw.rivystage.csv"]
                    assert b"inf" in files["ccw.flood.csv"]
            if case == "qhh_w":                    # y_rhs and y_out differ in the lake entry of an exported step
                ops = refio.writer_ops(rec)
                fy = [op[2][-1] for op in ops if op[0] == "f"]
                xy = [op[2][-1] for op in ops if op[0] == "x"]
                assert fy[0] != xy[0] and fy[1] == xy[1]
            del rec["script_y"]                     # rebuilt by refio.writer_script (deterministic)
        paths = refio.save_recording(case, rec)
        print(case, [f"{os.path.basename(p)} {os.path.getsize(p)}" for p in paths])


if __name__ == "__main__":
    if not refio.have_ref():
        sys.exit("oracle/_ref/ holds no reference binaries: run `make -C oracle` with a reference checkout")
    what = sys.argv[1:] or ["rhs", "kat", "et", "writers"]
    if "writers" in what and not refio.have_writer_ref():
        sys.exit("oracle/_ref/shud_ref_f predates the driver's mode w: run `make -C oracle`")
    for w in what:
        {"rhs": record_rhs, "kat": record_kat, "et": record_et, "writers": record_writers}[w]()
