"""Time of one water-balance sample pass (shud_wb_sample: element pass + reach pass + finalize) on a synthetic
mesh, with HIP events on the handle's stream (shud_wb_time_samples), and the bandwidth that time means for the
bytes the element pass moves (counted from its loads and stores, csrc/shud_wb.hip: 236 B per element, 300 B with
the trapezoid rule's previous-rate arrays).  Also holds three basin sums of the timed mesh to the bound every
summation order meets, |gpu - fsum(terms)| <= (n - 1) 2^-53 sum|terms| (at 10M elements the finalize kernel's
loop makes three trips; tests/test_gpu_wb.py holds all nine sums to the bound up to 4.25M elements).
The quad monitor's pass (shud_wb_time_quad, 116 B per element) is timed in the same process between two timings of
the sample pass, and two of its rates are held to the same bound.

usage: python tools/wb_sample_time.py [--n-ele 10000000] [--reps 20]      -> one JSON line (Euler and trapezoid)"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))

from shud_rhs import abi, runtime, synth, workload  # noqa: E402

BYTES_EULER, BYTES_TRAPZ = 236, 300
BYTES_QUAD = 116          # k_wb_quad: area 8, flags 4, qElePrep 8, ic_raw 8, qEs..qTg 40, QeleSurf + QeleSub 48


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ele", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    t0 = time.time()
    m = synth.synth_model(a.n_ele)
    m.step = workload.random_step_inputs(m)
    y = workload.random_state(m)
    NE = m.num_ele
    print(f"[wb] syn mesh NE={NE} NR={m.num_riv} built in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    h = runtime.RhsHandle(m)
    h.set_step_inputs()
    d_y, d_f = h.device_alloc(8 * m.num_y), h.device_alloc(8 * m.num_y)
    h.h2d(d_y, y)
    h.eval_device(0.0, d_y, d_f)
    h.summary(d_y)
    h.refresh_diagnostics()
    wb = runtime.WaterBalance(h, 60)
    wb.on_et_update()
    wb.sample(1.0, d_f)                                        # DY = the RHS of this state
    g = wb.read(arrays=False)
    d = h.diagnostics()
    sy, area = m.par["Sy"], m.ele["area"]
    terms = {"P": m.step["prcp"] * area,
             "ET": (d["e_ic"] + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * area,
             "storage": (y[:NE] + sy * y[NE:2 * NE] + sy * y[2 * NE:3 * NE] + 0.0 + 0.0) * area}
    got = {"P": g["basin_rate"][abi.SHUD_WB_P], "ET": g["basin_rate"][abi.SHUD_WB_ET], "storage": g["storage"][0]}
    checks = {}
    for k, v in terms.items():
        ref, s_abs = math.fsum(v), math.fsum(np.abs(v))
        bound = (v.size - 1) * 2.0 ** -53 * s_abs
        checks[k] = {"gpu": got[k], "fsum": ref, "abs_diff": abs(got[k] - ref), "bound": bound,
                     "ok": bool(abs(got[k] - ref) <= bound and s_abs > 0)}
    # element-level closure: with DY = f(y) of the sampled state the DY-based and the flux-budget rates integrate
    # the same water, so after one sample (dt = 1) the two accumulators differ by rounding only (information)
    ga = wb.read()
    scale = float(np.abs(ga["acc3"]).max())
    closure = {"max_abs_acc3": scale,
               "max_abs_acc3_minus_budget": float(np.abs(ga["acc3"] - ga["acc3_budget"]).max()),
               "max_abs_accfull_minus_budget": float(np.abs(ga["accfull"] - ga["accfull_budget"]).max())}
    del ga
    ms = wb.time_samples(d_f, a.reps)
    wb.close()
    wb = runtime.WaterBalance(h, 60, trapz=True)
    wb.on_et_update()
    ms_t = wb.time_samples(d_f, a.reps)
    wb.close()
    # the quad monitor's pass (shud_wb_quad_step: rates only, nothing stored per element) and, in the same process
    # and on the same arrays, the sample pass again right before and after it
    wb = runtime.WaterBalance(h, 60)
    wb.quad_enable()
    wb.on_et_update()
    ms_s1 = wb.time_samples(d_f, a.reps)
    ms_q = wb.time_quad(a.reps)
    ms_s2 = wb.time_samples(d_f, a.reps)
    ms_q2 = wb.time_quad(a.reps)
    qrate = wb.read_quad()["rate"]
    wb.close()
    for k, idx in (("P", abi.SHUD_WB_P), ("ET", abi.SHUD_WB_ET)):
        ref, s_abs = math.fsum(terms[k]), math.fsum(np.abs(terms[k]))
        bound = (terms[k].size - 1) * 2.0 ** -53 * s_abs
        checks["quad_" + k] = {"gpu": qrate[idx], "fsum": ref, "abs_diff": abs(qrate[idx] - ref), "bound": bound,
                               "ok": bool(abs(qrate[idx] - ref) <= bound and s_abs > 0)}
    quad = {"ms_per_pass": [ms_q, ms_q2], "bytes_per_element": BYTES_QUAD,
            "TBps": BYTES_QUAD * NE / (min(ms_q, ms_q2) * 1e-3) / 1e12,
            "sample_ms_same_process": [ms_s1, ms_s2],
            "sample_TBps_same_process": BYTES_EULER * NE / (min(ms_s1, ms_s2) * 1e-3) / 1e12}
    out = {"wb_sample": {"num_ele": NE, "num_riv": m.num_riv, "reps": a.reps, "quad": quad,
                         "euler": {"ms_per_sample": ms, "bytes_per_element": BYTES_EULER,
                                   "TBps": BYTES_EULER * NE / (ms * 1e-3) / 1e12},
                         "trapz": {"ms_per_sample": ms_t, "bytes_per_element": BYTES_TRAPZ,
                                   "TBps": BYTES_TRAPZ * NE / (ms_t * 1e-3) / 1e12},
                         "sum_checks": checks, "closure": closure}}
    h.device_free(d_y)
    h.device_free(d_f)
    h.close()
    print(json.dumps(out), flush=True)
    sys.exit(0 if all(c["ok"] for c in checks.values()) else 3)


if __name__ == "__main__":
    main()
