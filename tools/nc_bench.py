"""Device time of the NetCDF interval-end kernels (csrc/shud_out.hip k_snap_nc / k_snap_nc_sel) against the STREAM copy of
the same box (shud-up_amd/libshud_stream.so), at N positions (default 1M and 10M).

    python tools/nc_bench.py [--n 1000000,10000000] [--reps 200] [--out FILE]

Per position the kernel reads the 8-byte accumulator, writes 8 bytes of zero back and 4 bytes of slab (NETCDF), plus 8
bytes of snapshot in BOTH mode: 20 / 28 bytes.  The copy moves 16 bytes per double.  Both are timed with device events
over back-to-back launches on buffers of the same footprint, so both see the same cache state; the 1 GiB copy (beyond
every cache) is printed beside them.  One JSON line per size."""
import argparse
import ctypes
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))


def copy_gbs(lib, torch, n, reps):
    a = torch.ones(n, dtype=torch.float64, device="cuda")
    b = torch.empty_like(a)
    st = torch.cuda.current_stream().cuda_stream
    best = 0.0
    for v in (0, 1, 2):
        for _ in range(3):
            lib.shud_stream_copy_v(a.data_ptr(), b.data_ptr(), 8 * n, st, v)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            lib.shud_stream_copy_v(a.data_ptr(), b.data_ptr(), 8 * n, st, v)
        e1.record()
        torch.cuda.synchronize()
        best = max(best, 2 * 8 * n * reps / (e0.elapsed_time(e1) * 1e-3) / 1e9)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1000000,10000000")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from shud_rhs import runtime as rt
    lib = ctypes.CDLL(os.path.join(ROOT, "shud-up_amd", "libshud_stream.so"))
    lib.shud_stream_copy_v.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int]
    big = copy_gbs(lib, torch, 1 << 27, 20)
    lines = []
    for n in (int(x) for x in args.n.split(",")):
        src = torch.rand(n, dtype=torch.float64, device="cuda")
        flags = np.ones(n, dtype=np.int32)
        flags[::7] = 0
        res = {"positions": n, "reps": args.reps, "stream_copy_1GiB_GBs": round(big, 1),
               "stream_copy_same_footprint_GBs": round(copy_gbs(lib, torch, n, args.reps), 1)}
        with tempfile.TemporaryDirectory() as d:
            for mode, legacy, fl, nbytes in (("netcdf_all", False, None, 20), ("both_all", True, None, 28),
                                             ("netcdf_6of7", False, flags, None), ("both_6of7", True, flags, None)):
                os.makedirs(os.path.join(d, mode))
                out = rt.Output()
                out.attach_nc("riv", n, 20000101, out_dir=os.path.join(d, mode), history="bench")
                out.add(os.path.join(d, mode, "b.rivqdown"), src.data_ptr(), n, 60, 1, start_time=20000101, flag_io=fl,
                        nc="riv", legacy=legacy)
                ms = out.time_nc(0, args.reps)
                if nbytes is None:      # 6 of 7 positions selected: 4 B index + 4 B slab everywhere, the rest per column
                    nsel = int(flags.sum())
                    total = 8 * n + (16 + (8 if legacy else 0)) * nsel
                else:
                    total = nbytes * n
                res[mode] = {"us": round(ms * 1e3, 2), "bytes": total, "GBs": round(total / (ms * 1e-3) / 1e9, 1),
                             "us_of_a_copy_of_these_bytes": round(total / (res["stream_copy_same_footprint_GBs"] * 1e9)
                                                                  * 1e6, 2)}
                out.close()
        lines.append(json.dumps({"nc_bench": res}))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
