#!/usr/bin/env python3
"""ckpt_bench.py — what an exact checkpoint (include/shud_ckpt.h) costs a device run on an MI355X.

One process, the synthetic model at --n-ele, the device integrator over its RHS handle (random state and ET-step
inputs, CV_ONE_STEP internal steps as in bench.py's integrator figure).  Measured:
  pack         ms and bytes of the snapshot's one device pass (shud_ckpt_time_pack: HIP events around --reps passes),
               beside the box's STREAM copy probe (libshud_stream.so through bench.stream_probe) in the same process
  stepping     ms per internal step over windows of --window steps, three variants interleaved round-robin --rounds
               times (medians, and the per-round differences against `none`; before every window the previous
               file's drain and its write-back from the page cache are waited for): `none` no snapshot; `snapshot`
               one shud_ckpt_snapshot at the window's start, stepping on while it drains; `plain_host` instead of it a synchronous device->pageable-host copy of as many
               bytes, section by section (the section sizes of the file just written) — the variant a checkpoint
               without the device pass and the pinned ring would be; it lives here, not in the library
  flush        seconds from a snapshot call until shud_ckpt_flush returns (the file complete and renamed), with the
               file's size
Writes one JSON file (--out) and prints it.

    python tools/ckpt_bench.py --n-ele 10000000 --out profiles/ckpt/syn10M.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ele", type=int, default=10000000)
    ap.add_argument("--reps", type=int, default=10, help="pack passes per timed window")
    ap.add_argument("--window", type=int, default=10, help="internal steps per window (one snapshot per window)")
    ap.add_argument("--rounds", type=int, default=7, help="interleaved rounds over the variants")
    ap.add_argument("--dir", default=None, help="directory of the checkpoint file (default: a temporary one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    from shud_rhs import runtime, synth, workload

    if not torch.cuda.is_available():
        sys.exit("ckpt_bench: no GPU (nothing is measured without one)")
    torch.cuda.set_device(0)
    gm = synth.synth_model(args.n_ele)
    gm.step = workload.random_step_inputs(gm)
    y = workload.random_state(gm)
    sp = bench.stream_probe(0)
    h = runtime.RhsHandle(gm)
    h.set_step_inputs()
    ode = runtime.OdeSolver(h, 0.0, y, 1e-4, 1e-4, 1e-2, 30.0)
    d_y = h.device_alloc(8 * h.num_y)
    ck = runtime.Checkpoint(stream=h.stream())
    work = args.dir or tempfile.mkdtemp(prefix="ckpt_bench_")
    path = os.path.join(work, "bench.ckpt")

    def steps(n):
        for _ in range(n):
            flag, _ = ode.solve_device(1.0e9, d_y, one_step=True)
            if flag < 0:
                sys.exit(f"ckpt_bench: the integrator failed with flag {flag}")

    steps(3)                                             # past the start-up step
    h.synchronize()
    pack_ms, pack_bytes = ck.time_pack(args.reps, ode, rhs=h)
    # flush time and the section sizes
    t0 = time.perf_counter()
    ck.snapshot(path, 0.0, 0, ode, rhs=h)
    t_call = time.perf_counter() - t0
    ck.flush()
    t_flush = time.perf_counter() - t0
    info = runtime.Checkpoint.info(path)
    sizes = [8 * s[2] for s in info["sections"] if not s[0].endswith(".host") and s[0] != "dev.tails"]
    d_src = torch.empty(max(sizes), dtype=torch.uint8, device="cuda")
    host = np.empty(max(sizes), dtype=np.uint8)

    def plain_host():
        for nb in sizes:                                 # synchronous, pageable destination
            h.d2h(host[:nb], d_src.data_ptr())

    rows = {"none": [], "snapshot": [], "plain_host": []}
    for _ in range(args.rounds):
        for name in rows:
            ck.flush()                                   # the previous window's drain is not part of this one,
            os.sync()                                    # nor the write-back of its file from the page cache
            h.synchronize()
            t = time.perf_counter()
            if name == "snapshot":
                ck.snapshot(path, 0.0, 0, ode, rhs=h)
            elif name == "plain_host":
                plain_host()
            steps(args.window)
            h.synchronize()
            rows[name].append((time.perf_counter() - t) * 1e3 / args.window)
    ck.flush()
    med = {k: float(statistics.median(v)) for k, v in rows.items()}
    copy = sp.get("stream_copy_GBs")
    out = {"n_ele": gm.num_ele, "n_riv": gm.num_riv, "ny": h.num_y, "window": args.window, "rounds": args.rounds,
           "box": {k: sp.get(k) for k in ("stream_copy_GBs", "stream_read_GBs")},
           "pack": {"ms": pack_ms, "bytes_copied": pack_bytes, "GBs_read_plus_written": 2 * pack_bytes / pack_ms / 1e6,
                    "frac_of_stream_copy": (2 * pack_bytes / pack_ms / 1e6 / copy) if copy else None,
                    "sections": len(sizes)},
           "stepping_ms_per_step": med, "stepping_ms_per_step_all": rows,
           # paired by round (each round's window against that round's `none` window), median of the pairs
           "added_ms_per_step_paired": {k: {"by_round": [a - b for a, b in zip(rows[k], rows["none"])],
                                            "median": float(statistics.median(a - b for a, b in zip(rows[k], rows["none"])))}
                                        for k in ("snapshot", "plain_host")},
           "flush": {"snapshot_call_s": t_call, "until_flush_s": t_flush, "file_bytes": os.path.getsize(path),
                     "file_GBs": os.path.getsize(path) / t_flush / 1e9}}
    runtime.Checkpoint.verify(path)
    ck.close()
    ode.close()
    h.device_free(d_y)
    h.close()
    os.unlink(path)
    txt = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")
    print(txt)


if __name__ == "__main__":
    main()
