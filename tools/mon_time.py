"""Measurements of the run monitors (include/shud_mon.h).

  flood  time of one flood pass (count, scan, scatter, copy of the count word; shud_mon_time_flood, HIP events) on
         NR reaches with 0 %, 1 % and 100 % of them above their bank, beside the time of a plain device->host copy of
         the two NR-double arrays into pinned memory (what a host-side scan would need after every solver step) and
         the record bytes a flood pass sends instead.
  e2e    shud_gpu loop_s on a synthetic project (bench.py's end-to-end project: --n-ele 100000, one day), runs
         interleaved round by round: both flags, no flags and, with --parent DIR (a build of the parent commit:
         shud_gpu and its two libraries), the parent without flags.

usage: python tools/mon_time.py flood [--n-riv 970000] [--reps 50]
       python tools/mon_time.py e2e [--n-ele 100000] [--rounds 3] [--parent DIR]        -> one JSON line each"""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))


def flood(a):
    import torch
    from shud_rhs import runtime
    nr = a.n_riv
    rng = np.random.default_rng(3)
    stage = torch.zeros(nr, dtype=torch.float64, device="cuda")
    q = torch.from_numpy(rng.normal(0.0, 1e4, nr)).cuda()
    pin = torch.empty(2 * nr, dtype=torch.float64).pin_memory()
    mon = runtime.RunMonitors()
    tmp = tempfile.mkdtemp()
    mon.add_flood(os.path.join(tmp, "t.flood.csv"), stage, q, nr, np.ones(nr), np.ones(nr, dtype=np.int32))
    out = {"num_riv": nr, "reps": a.reps, "cases": {}}
    for name, frac in (("0pct", 0.0), ("1pct", 0.01), ("100pct", 1.0)):
        s = np.full(nr, 0.5)
        s[rng.uniform(0, 1, nr) < frac] = 1.5
        stage.copy_(torch.from_numpy(s))
        torch.cuda.synchronize()
        ms = [mon.time_flood(a.reps) for _ in range(3)]
        n = int((s > 1.0).sum())
        out["cases"][name] = {"flooded": n, "ms_per_pass": ms, "record_bytes": 24 * n + 4}
    # the approach this replaces: both arrays to the host after every step
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    copies = []
    for _ in range(3):
        torch.cuda.synchronize()
        e0.record()
        for _ in range(a.reps):
            pin[:nr].copy_(stage, non_blocking=True)
            pin[nr:].copy_(q, non_blocking=True)
        e1.record()
        e1.synchronize()
        copies.append(e0.elapsed_time(e1) / a.reps)
    out["plain_d2h"] = {"bytes": 16 * nr, "ms_per_step": copies}
    # end to end with the writer: one flood() call and the flush that waits for its rows
    import time
    for name, frac in (("0pct", 0.0), ("1pct", 0.01)):
        s = np.full(nr, 0.5)
        s[rng.uniform(0, 1, nr) < frac] = 1.5
        stage.copy_(torch.from_numpy(s))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mon.flood(60.0)
        t1 = time.perf_counter()
        mon.flush()
        t2 = time.perf_counter()
        out["cases"][name]["enqueue_ms"] = 1e3 * (t1 - t0)
        out["cases"][name]["enqueue_to_written_ms"] = 1e3 * (t2 - t0)
    mon.close()
    print(json.dumps({"mon_flood": out}), flush=True)


def e2e(a):
    from shud_rhs import synth
    d = tempfile.mkdtemp(prefix="mon_e2e_")
    synth.write_project(d, "syn", a.n_ele, days=1.0, extra_para={"Update_IC_STEP": a.update_ic_step})
    print(f"[mon] project written: {d}", file=sys.stderr, flush=True)
    variants = [("flags", os.path.join(ROOT, "shud-up_amd", "shud_gpu"), ["--flood", "--ic-snapshots"]),
                ("noflags", os.path.join(ROOT, "shud-up_amd", "shud_gpu"), [])]
    if a.parent:
        variants.append(("parent", os.path.join(a.parent, "shud_gpu"), []))
    res = {k: [] for k, _, _ in variants}
    for r in range(a.rounds):
        for name, exe, flags in variants:
            p = subprocess.run(["timeout", "-k", "10", "300", exe, *flags, "-q", "-o", os.path.join(d, f"out_{name}"),
                                "-C", d, d, "syn"], capture_output=True, text=True)
            if p.returncode != 0:
                print(p.stdout[-500:] + p.stderr[-500:], file=sys.stderr)
                sys.exit(p.returncode)                       # nothing more on the GPU after a failed run
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('{"shud_gpu"')]
            j = json.loads(line[-1])["shud_gpu"]
            res[name].append({k: j[k] for k in ("loop_s", "wall_s", "solver_steps", "loop_phases_s", "flood_rows",
                                                "ic_snapshots", "monitors_writer_s") if k in j})
            print(f"[mon] round {r} {name}: loop_s {j['loop_s']}", file=sys.stderr, flush=True)
    same = all(open(os.path.join(d, "out_flags", f), "rb").read() == open(os.path.join(d, "out_noflags", f), "rb").read()
               for f in os.listdir(os.path.join(d, "out_noflags")))
    print(json.dumps({"mon_e2e": {"num_ele": a.n_ele, "update_ic_step": a.update_ic_step, "rounds": a.rounds,
                                  "dat_identical_flags_vs_noflags": same, "runs": res}}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    f = sub.add_parser("flood")
    f.add_argument("--n-riv", type=int, default=970_000)
    f.add_argument("--reps", type=int, default=50)
    e = sub.add_parser("e2e")
    e.add_argument("--n-ele", type=int, default=100_000)
    e.add_argument("--rounds", type=int, default=3)
    e.add_argument("--update-ic-step", type=int, default=720)
    e.add_argument("--parent", default=None)
    a = ap.parse_args()
    flood(a) if a.cmd == "flood" else e2e(a)


if __name__ == "__main__":
    main()
