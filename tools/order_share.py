#!/usr/bin/env python3
"""order_share.py — what an element order is worth to the in-tile edge sharing, counted on the CPU (no device): the
table of DESIGN §5i.

Per mesh and numbering (generator or file order, a seeded random permutation, that permutation through
shud_order_plan "bfs" and "tiles") the host's own plan of the applied model (shud_rhs_plan_layout, arrays=True):
  share   elements that receive a shared edge / NE (bit 4 of edge_plan: stored slot 2 is received)
  waves   of the NE // 64 full 64-lane waves (consecutive elements, as the element kernel maps them), the share in
          which every lane receives: a receiving lane skips its gathers, a wave saves the pass only when all 64 do
  plan_s  shud_order_plan wall time
The random permutation is default_rng(12345) as tools/order_bench.py (default_rng(43) for variant(20000, 43), as the
tests).  Prints one JSON line per mesh.

    python tools/order_share.py [--big]          # --big adds synth_model(1250000)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "shud-up_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(m, runtime):
    lay = runtime.plan_layout(m, arrays=True)
    rcv = ((lay["edge_plan"] >> 4) & 1).astype(bool)
    assert int(rcv.sum()) == lay.get("shared_edges", 0)
    nw = m.num_ele // 64
    waves = float(rcv[:nw * 64].reshape(nw, 64).all(1).mean()) if nw else 0.0
    return {"share": round(float(rcv.sum()) / m.num_ele, 4), "waves": round(waves, 4)}


def row(name, base, pe, runtime):
    out = {"mesh": name, "n_ele": base.num_ele, "generator_or_file": stats(base, runtime)}
    m = base
    if pe is not None:
        m = runtime.order_apply(base, pe.astype(np.int32))
        out["random"] = stats(m, runtime)
    for order in ("bfs", "tiles"):
        t = time.perf_counter()
        p = runtime.order_plan(m, order)
        dt = time.perf_counter() - t
        out[order] = dict(stats(runtime.order_apply(m, p), runtime), plan_s=round(dt, 4))
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", action="store_true", help="also synth_model(1250000)")
    args = ap.parse_args()
    import cases
    from shud_rhs import runtime, synth
    row("ccw", cases.ccw()[0], None, runtime)
    row("heihe", cases.heihe()[0], None, runtime)
    m = cases.variant(20000, seed=43)[0]
    row("variant(20000, 43)", m, np.random.default_rng(43).permutation(m.num_ele), runtime)
    for n in [300000] + ([1250000] if args.big else []):
        m = synth.synth_model(n)
        row(f"synth_model({n})", m, np.random.default_rng(12345).permutation(m.num_ele), runtime)


if __name__ == "__main__":
    main()
