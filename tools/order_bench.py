#!/usr/bin/env python3
"""order_bench.py — what the element numbering is worth to the RHS on an MI355X (include/shud_order.h).

One process per mesh size, four handles on the same synthetic model, measured interleaved (round-robin, `--rounds`
times, medians reported):
  generator   the generator's own numbering (grid rows): what every speed figure of record is taken on
  random      a seeded random element permutation of it (shud_order_apply): a numbering that says nothing
  random_bfs  that permuted model through an ordered handle (order="bfs"): what the library recovers on its own
  random_tiles  the same permuted model through order="tiles": the order that keeps neighbours inside a sharing tile
              at any mesh size (the yardstick for it is random_bfs in the same process and run)
Per variant: element-kernel and river-kernel ms (HIP events between the kernels, shud_rhs_time_kernels), wall ms per
device-pointer eval (host clock around `--reps` evals ending in a synchronise) and shud_rhs_layout_shared.  For the
ordered handles also the permute kernel (shud_rhs_permute on a state vector of the bfs handle: ms and the GB/s of
bytes read + written, beside the box's STREAM copy figure from bench.py's probe) and the host-pointer eval of each
against the plain handle on the same (random) model, whose DY must be the same bits.  Writes one JSON file (--out)
and prints it.

    python tools/order_bench.py --n-ele 1250000 --out profiles/order/syn1250k_tiles.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ele", type=int, default=1250000)
    ap.add_argument("--reps", type=int, default=50, help="evals per timed window")
    ap.add_argument("--rounds", type=int, default=5, help="interleaved rounds over the variants")
    ap.add_argument("--host-reps", type=int, default=3, help="host-pointer evals per round")
    ap.add_argument("--seed", type=int, default=12345)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import bench
    from shud_rhs import runtime, synth, workload

    if not torch.cuda.is_available():
        sys.exit("order_bench: no GPU (nothing is measured without one)")
    torch.cuda.set_device(0)
    stream = torch.cuda.current_stream()
    t0 = time.time()
    gm = synth.synth_model(args.n_ele)
    gm.step = workload.random_step_inputs(gm)
    y = workload.random_state(gm)
    NE, NR = gm.num_ele, gm.num_riv
    pe = np.random.default_rng(args.seed).permutation(NE).astype(np.int32)
    rm = runtime.order_apply(gm, pe)
    y_r = np.concatenate([runtime.order_gather(pe, y[:3 * NE], 3), y[3 * NE:]])
    t_plan = time.time()
    bfs = runtime.order_plan(rm, "bfs")
    t_plan = time.time() - t_plan
    t_plan_tiles = time.time()
    tiles = runtime.order_plan(rm, "tiles")
    t_plan_tiles = time.time() - t_plan_tiles
    print(f"[order_bench] NE={NE} NR={NR}: models in {time.time() - t0:.1f}s, breadth-first plan {t_plan:.2f}s, "
          f"tiles plan {t_plan_tiles:.2f}s", file=sys.stderr, flush=True)

    sp = bench.stream_probe(0)
    handles = {"generator": (runtime.RhsHandle(gm, stream=stream.cuda_stream), y),
               "random": (runtime.RhsHandle(rm, stream=stream.cuda_stream), y_r),
               "random_bfs": (runtime.RhsHandle(rm, stream=stream.cuda_stream, order="bfs"), y_r),
               "random_tiles": (runtime.RhsHandle(rm, stream=stream.cuda_stream, order="tiles"), y_r)}
    assert np.array_equal(handles["random_bfs"][0].order()[1], bfs)
    assert np.array_equal(handles["random_tiles"][0].order()[1], tiles)
    dev = {}
    for name, (h, yy) in handles.items():
        h.set_step_inputs()
        d_y = torch.from_numpy(yy).cuda()
        d_dy = torch.empty_like(d_y)
        if h.ordered:                                # device pointers of an ordered handle: the internal numbering
            d_in = torch.empty_like(d_y)
            h.permute(d_y.data_ptr(), d_in.data_ptr(), to="internal")
            d_y = d_in
        dev[name] = (d_y, d_dy)
        for _ in range(10):                          # warm-up: code objects, clocks
            h.eval_device(0.0, d_y.data_ptr(), d_dy.data_ptr())
    torch.cuda.synchronize()

    rows = {k: {"ele_ms": [], "riv_ms": [], "eval_wall_ms": []} for k in handles}
    for _ in range(args.rounds):
        for name, (h, _) in handles.items():
            d_y, d_dy = dev[name]
            _, ms = h.time_kernels(0.0, d_y.data_ptr(), d_dy.data_ptr(), args.reps)
            rows[name]["ele_ms"].append(ms["shud_ele_kernel"])
            rows[name]["riv_ms"].append(ms["shud_riv_kernel"])
            torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(args.reps):
                h.eval_device(0.0, d_y.data_ptr(), d_dy.data_ptr())
            torch.cuda.synchronize()
            rows[name]["eval_wall_ms"].append((time.perf_counter() - t) * 1e3 / args.reps)

    def med(v):
        return float(statistics.median(v))

    out = {"n_ele": NE, "n_riv": NR, "n_seg": gm.num_seg, "reps": args.reps, "rounds": args.rounds,
           "bfs_plan_s": t_plan, "tiles_plan_s": t_plan_tiles,
           "box": {k: sp.get(k) for k in ("stream_copy_GBs", "stream_read_GBs")}, "variants": {}}
    for name, (h, _) in handles.items():
        r = rows[name]
        out["variants"][name] = {"ele_ms": med(r["ele_ms"]), "riv_ms": med(r["riv_ms"]),
                                 "eval_wall_ms": med(r["eval_wall_ms"]),
                                 "ele_ms_spread": [min(r["ele_ms"]), max(r["ele_ms"])],
                                 "shared_edges": h.layout().get("shared_edges", 0),
                                 "share_of_elements": h.layout().get("shared_edges", 0) / NE}
    g, rd, bf, tl = (out["variants"][k] for k in ("generator", "random", "random_bfs", "random_tiles"))
    out["ratios"] = {k: {"random_over_generator": rd[k] / g[k], "bfs_over_generator": bf[k] / g[k],
                         "tiles_over_generator": tl[k] / g[k], "tiles_over_bfs": tl[k] / bf[k]}
                     for k in ("ele_ms", "riv_ms", "eval_wall_ms")}

    # the permute kernel on a state vector, both directions
    hb = handles["random_bfs"][0]
    a, b = torch.from_numpy(y_r).cuda(), torch.empty(y_r.size, dtype=torch.float64, device="cuda")
    nbytes = 2 * 8 * y_r.size + 4 * NE               # vector read + written, the index read
    perm_ms = {}
    # (the handle runs on its own stream: host clock around a window that ends in the handle's synchronise)
    nperm = 8 * args.reps
    for to in ("internal", "caller"):
        for _ in range(5):
            hb.permute(a.data_ptr(), b.data_ptr(), to=to)
        hb.synchronize()
        t = time.perf_counter()
        for _ in range(nperm):
            hb.permute(a.data_ptr(), b.data_ptr(), to=to)
        hb.synchronize()
        perm_ms[to] = (time.perf_counter() - t) * 1e3 / nperm
    out["permute"] = {"bytes": nbytes, "ms": perm_ms,
                      "GBs": {k: nbytes / (v * 1e-3) / 1e9 for k, v in perm_ms.items()},
                      "frac_of_stream_copy": ({k: nbytes / (v * 1e-3) / 1e9 / sp["stream_copy_GBs"]
                                               for k, v in perm_ms.items()} if sp.get("stream_copy_GBs") else None)}

    # host-pointer eval: the plain handle and the ordered ones on the same (random) model, interleaved
    host = {"random": [], "random_bfs": [], "random_tiles": []}
    dys = {}
    for _ in range(args.rounds):
        for name in host:
            h = handles[name][0]
            t = time.perf_counter()
            for _ in range(args.host_reps):
                dys[name] = h.eval(0.0, y_r)
            host[name].append((time.perf_counter() - t) * 1e3 / args.host_reps)
    out["host_eval"] = {"plain_ms": med(host["random"]), "ordered_ms": med(host["random_bfs"]),
                        "added_ms": med(host["random_bfs"]) - med(host["random"]),
                        "two_permute_launches_ms": perm_ms["internal"] + perm_ms["caller"],
                        "same_bits": bool(np.array_equal(dys["random"].view(np.uint64),
                                                         dys["random_bfs"].view(np.uint64))),
                        "tiles_ordered_ms": med(host["random_tiles"]),
                        "tiles_added_ms": med(host["random_tiles"]) - med(host["random"]),
                        "tiles_same_bits": bool(np.array_equal(dys["random"].view(np.uint64),
                                                               dys["random_tiles"].view(np.uint64)))}
    for h, _ in handles.values():
        h.close()
    txt = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(txt + "\n")
    print(txt)
    if not (out["host_eval"]["same_bits"] and out["host_eval"]["tiles_same_bits"]):
        sys.exit("order_bench: an ordered handle's DY differs from the plain handle's")


if __name__ == "__main__":
    main()
