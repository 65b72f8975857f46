"""shud_gpu on a synthetic 2000-element project (one day) with the water-balance diagnostics off and on: the
per-phase wall times of its loop, and the basin residual of the diagnostic run relative to the accumulated
precipitation (basinwbfull.dat column 9 against column 2, summed over the rows).  A fourth run adds the quad monitor
(SHUD_WB_DIAG_QUAD=1): its phase time and the residuals of basinwbfull.dat and basinwbfull_quad.dat of that one run.

usage: python tools/wb_e2e.py [--n-ele 2000] [--days 1.0] [--workdir DIR]      -> one JSON line"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))

from shud_rhs import shudio, synth  # noqa: E402


def run(src, out, env):
    r = subprocess.run([os.path.join(ROOT, "shud-up_amd", "shud_gpu"), "-q", "-o", out, "-C", src, src, "syn"],
                       capture_output=True, text=True, timeout=600, env=env)
    if r.returncode:
        sys.exit(r.stdout + r.stderr)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"shud_gpu"')][-1]
    return json.loads(line)["shud_gpu"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ele", type=int, default=2000)
    ap.add_argument("--days", type=float, default=1.0)
    ap.add_argument("--workdir", default=None)
    a = ap.parse_args()
    work = a.workdir or tempfile.mkdtemp(prefix="wb_e2e_")
    src = os.path.join(work, "in")
    synth.write_project(src, "syn", a.n_ele, days=a.days, max_step=10.0, et_step=60.0, dt_out=60)
    base = {k: v for k, v in os.environ.items() if not k.startswith("SHUD_WB_DIAG")}
    res = {}
    for name, env in (("off", base), ("on", dict(base, SHUD_WB_DIAG="1")),
                      ("on_trapz", dict(base, SHUD_WB_DIAG="1", SHUD_WB_DIAG_TRAPZ="1")),
                      ("on_quad", dict(base, SHUD_WB_DIAG="1", SHUD_WB_DIAG_QUAD="1"))):
        out = os.path.join(work, "out_" + name)
        j = run(src, out, env)
        res[name] = {"loop_s": j["loop_s"], "phases_s": j["loop_phases_s"],
                     "phases_sum_s": sum(j["loop_phases_s"].values()), "rhs_evals": j["rhs_evals"]}
        if name != "off":
            b = shudio.read_dat(os.path.join(out, "syn.basinwbfull.dat"))["data"]
            res[name]["basin"] = {"rows": int(b.shape[0]), "P_m3": float(b[:, 1].sum()),
                                  "dS_m3": float(b[:, 0].sum()), "resid_m3": float(b[:, 8].sum()),
                                  "resid_over_P": float(b[:, 8].sum() / b[:, 1].sum()),
                                  "max_row_resid_over_P": float(abs(b[:, 8]).max() / b[:, 1].sum()),
                                  "rows_m3": [[float(x) for x in row] for row in b[:3]]}
            if name == "on_quad":
                # the same run's two basin files: Euler at the solver steps against the trapezoid at the
                # integrator's own steps; first row and whole run
                q = shudio.read_dat(os.path.join(out, "syn.basinwbfull_quad.dat"))["data"]
                res[name]["quad_steps"] = j["quad_steps"]
                res[name]["cvode_steps"] = j["cvode_steps"]
                res[name]["quad"] = {"rows": int(q.shape[0]), "first_row_m3": [float(x) for x in q[0]],
                                     "first_row_resid_m3": float(q[0, 8]), "basin_first_row_resid_m3": float(b[0, 8]),
                                     "first_row_ratio": float(abs(q[0, 8]) / abs(b[0, 8])) if b[0, 8] else None,
                                     "resid_m3": float(q[:, 8].sum()), "basin_resid_m3": float(b[:, 8].sum()),
                                     "resid_over_P": float(q[:, 8].sum() / q[:, 1].sum())}
            for key in ("elewb3_resid", "elewb3_budget_resid", "elewbfull_resid", "elewbfull_budget_resid"):
                e = shudio.read_dat(os.path.join(out, f"syn.{key}.dat"))["data"]
                res[name][key + "_max_abs_m"] = float(abs(e).max())
    print(json.dumps({"wb_e2e": {"num_ele": a.n_ele, "days": a.days, **res}}), flush=True)


if __name__ == "__main__":
    main()
