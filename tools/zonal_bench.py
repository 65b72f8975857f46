"""Device time of the zonal per-export pass (csrc/shud_out.hip k_zone_partial + k_zone_final) for 19 zonal controls
against k_accumulate for 19 plain controls over the same sources, at N elements (default 1M and 10M) and NZ zones
(default 1, 1 000, 100 000), with the STREAM copy of the same box (shud-up_amd/libshud_stream.so) beside them.

    python tools/zonal_bench.py [--n 1000000,10000000] [--nz 1,1000,100000] [--reps 20] [--rounds 3] [--out FILE]

One process; the two passes are timed with device events in interleaved rounds (zonal, plain, zonal, ...); the best
round of each is quoted and every round is recorded.  --reps is the count at 10M elements or more; smaller sizes run
proportionally more passes per window (200 at 1M), so every timed window is tens of milliseconds long.
Memberships: "blocks" (zone z owns a run of consecutive elements, as sub-basins of a locality-ordered mesh do) and "random" (land-cover classes scattered over the mesh; only at the middle NZ).  15 of the
19 zonal controls are area-weighted means, 4 are sums, as shud_gpu --zones registers them on a full output list.
Per member the zonal pass reads 8 B of source, 4 B of member index and 8 B of weight (12 B unweighted); k_accumulate
reads 8 B of source and reads and writes 8 B of accumulator (24 B).  interval_end: device time of the export that ends
an interval of all 19 zonal controls minus one that ends none (19 k_snap / k_snap_wmean launches over NZ values).
pcie_bytes: what crosses PCIe per interval, NZ * 8 per zonal control against N * 8 per plain one.  One JSON line per
(N, NZ, membership)."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
NCTRL, NMEAN = 19, 15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000,10000000")
    ap.add_argument("--nz", default="1,1000,100000")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from nc_bench import copy_gbs
    from shud_rhs import runtime as rt
    lib = ctypes.CDLL(os.path.join(ROOT, "shud-up_amd", "libshud_stream.so"))
    lib.shud_stream_copy_v.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    big = copy_gbs(lib, torch, 1 << 27, 20)
    nzs = [int(x) for x in args.nz.split(",")]
    rng = np.random.default_rng(1)
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        reps = args.reps * max(1, 10_000_000 // n)
        srcs = [torch.rand(n, dtype=torch.float64, device="cuda") for _ in range(NCTRL)]
        area = rng.uniform(50.0, 150.0, n)
        with tempfile.TemporaryDirectory() as d:
            plain = rt.Output()
            for k in range(NCTRL):                               # no file: only the per-export pass is timed
                plain.add(os.path.join(d, f"p{k}"), srcs[k].data_ptr(), n, 60, 1, start_time=20000101, binary=False)
            for nz in nzs:
                kinds = ["blocks"] + (["random"] if nz == nzs[len(nzs) // 2] and nz > 1 else [])
                for kind in kinds:
                    zone = (np.arange(n, dtype=np.int64) * nz // n + 1).astype(np.int32)
                    if kind == "random":
                        zone = rng.permutation(zone)
                    zd = os.path.join(d, f"z_{nz}_{kind}")
                    os.makedirs(zd)
                    out = rt.Output()
                    for k in range(NCTRL):
                        mean = k < NMEAN
                        out.add_zonal(os.path.join(zd, f"z{k}"), srcs[k].data_ptr(), n, 60, 1, zone, n_zone=nz,
                                      weight=area if mean else None, op="mean" if mean else "sum", start_time=20000101)
                    zonal_ms, plain_ms = [], []
                    for _ in range(args.rounds):
                        zonal_ms.append(out.time_pass("zonal", reps))
                        plain_ms.append(plain.time_pass("plain", reps))

                    def export_ms(t):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        torch.cuda.synchronize()
                        e0.record()
                        out.export(t)
                        e1.record()
                        torch.cuda.synchronize()
                        return e0.elapsed_time(e1)
                    export_ms(30.0)                              # warm-up
                    mid = min(export_ms(30.0) for _ in range(3))
                    end = min(export_ms(60.0 * (j + 1)) for j in range(3))
                    out.close()
                    zb = n * (NMEAN * 20 + (NCTRL - NMEAN) * 12)
                    pb = n * NCTRL * 24
                    res = {"elements": n, "zones": nz, "membership": kind, "controls": NCTRL, "reps": reps,
                           "stream_copy_1GiB_GBs": round(big, 1),
                           "zonal_pass_us": round(min(zonal_ms) * 1e3, 1), "zonal_pass_bytes": zb,
                           "zonal_pass_GBs": round(zb / (min(zonal_ms) * 1e-3) / 1e9, 1),
                           "accumulate_us": round(min(plain_ms) * 1e3, 1), "accumulate_bytes": pb,
                           "accumulate_GBs": round(pb / (min(plain_ms) * 1e-3) / 1e9, 1),
                           "zonal_over_accumulate": round(min(zonal_ms) / min(plain_ms), 3),
                           "interval_end_us": round((end - mid) * 1e3, 1),
                           "pcie_bytes_zonal": NCTRL * nz * 8, "pcie_bytes_plain": NCTRL * n * 8,
                           "rounds_zonal_us": [round(x * 1e3, 1) for x in zonal_ms],
                           "rounds_accumulate_us": [round(x * 1e3, 1) for x in plain_ms]}
                    lines.append(json.dumps({"zonal_bench": res}))
                    print(lines[-1], flush=True)
            plain.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
