#!/usr/bin/env python3
"""Dependent levels of a kernel's global loads, from the disassembly of the built library.

usage: vmem_levels.py [--lib shud-up_amd/libshud_rhs.so] [--listing FILE] [--dump] KERNEL-NAME-SUBSTRING

Every global load of the kernel is listed with its level: how many `s_waitcnt vmcnt` drains precede it since kernel
entry.  A wait opens a new level only if a load was issued since the last one that did, and a load that sits alone in
the shadow of a short forward `s_cbranch_execz` (one a wave skips unless a lane needs it: a boundary-condition value,
a stale head) is listed as conditional and opens none; neither do the system-scope (sc0 sc1) loads of the error-report
path, which a wave enters only when a lane reports.

The walk is the path of a wave whose lanes are active: unconditional branches and `s_cbranch_execnz` are taken,
every other conditional branch falls through, so blocks the compiler laid out of line are met where they run.  A
branch back to visited code closes a loop, which is walked once; a loop that holds loads is reported on its own.

Sections, by landmarks of the packed element kernel (shud_ele_packed.hip, the edge-sharing instantiations):
  prologue          entry .. the first s_barrier (the class table is in LDS)
  vertical part     .. the first non-temporal 8-B store (DY of the unsaturated zone)
  segment section   .. the first non-temporal load after it (edge stage 1's plane, or `area`)
  edge stage 1/2    each from the load group that holds a non-temporal 16-B load (the stage's ged plane)
  edge pass 3       likewise, the third such group
  tail              behind the first full drain of edge pass 3
A kernel without a landmark simply ends its sections early.  Only loads, stores, waits, barriers and branches are
looked at; --listing reads an `llvm-objdump -d` text instead of running it (the parser's test does).
"""
import argparse
import glob
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
SECTIONS = ["prologue", "vertical part", "segment section", "edge stage 1", "edge stage 2", "edge pass 3", "tail"]
_INS = re.compile(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
_TGT = re.compile(r"<[^>]*\+0x([0-9a-fA-F]+)>\s*$")


def objdump():
    for p in (os.path.join(ROCM, "llvm", "bin", "llvm-objdump"), os.path.join(ROCM, "bin", "llvm-objdump")):
        if os.path.exists(p):
            return p
    raise SystemExit("llvm-objdump not found under " + ROCM)


def disassemble(lib, key):
    """llvm-objdump -d text of the one kernel whose symbol holds `key`, from the gfx950 code objects bundled in lib"""
    od = objdump()
    with tempfile.TemporaryDirectory() as tmp:
        cp = os.path.join(tmp, "lib.so")
        with open(lib, "rb") as f, open(cp, "wb") as g:
            g.write(f.read())
        subprocess.run([od, "--offloading", cp], check=True, capture_output=True, cwd=tmp)
        for co in sorted(glob.glob(cp + ".*amdgcn*")):
            syms = subprocess.run([od, "-t", co], check=True, capture_output=True, text=True).stdout
            names = [l.split()[-1] for l in syms.splitlines() if " F .text" in l and key in l]
            if not names:
                continue
            if len(names) > 1:
                raise SystemExit("ambiguous kernel name, matches:\n  " + "\n  ".join(names))
            return subprocess.run([od, "-d", "--disassemble-symbols=" + names[0], co], check=True,
                                  capture_output=True, text=True).stdout
    raise SystemExit(f"no kernel matching {key!r} in {lib}")


def parse(text):
    """-> [{op, args, addr, target}] of one kernel's objdump text, in layout order (target: a branch's address)"""
    out, base = [], None
    for line in text.splitlines():
        m = _INS.match(line)
        if not m:
            continue
        op, args, addr = m.group(1), m.group(2), int(m.group(3), 16)
        if base is None:
            base = addr
        tgt = None
        if op.startswith("s_cbranch") or op == "s_branch":
            t = _TGT.search(line)
            if t:
                tgt = base + int(t.group(1), 16)
            else:                                     # no symbol: a signed dword count from the next instruction
                tgt = addr + 4 + 4 * int(args.split()[0], 0)
        out.append(dict(op=op, args=args, addr=addr, target=tgt))
    return out


def vm_load(i):
    return i["op"].startswith("global_load") or i["op"].startswith("flat_load")


def vm_store(i):
    return i["op"].startswith("global_store") or i["op"].startswith("flat_store")


def is_wait(i):
    return i["op"] == "s_waitcnt" and "vmcnt" in i["args"]


def is_nt(i):
    return re.search(r"\bnt\b", i["args"]) is not None


def path(ins):
    """-> (instructions in walking order, loops as (first, last) positions in it).  The walk is the path of a wave
    whose lanes are active: s_branch and a forward or not yet visited s_cbranch_execnz are taken, every other
    conditional branch falls through.  A conditional branch back to a visited instruction closes a loop and falls
    through; running into a visited instruction any other way closes a loop too, and the walk resumes at the latest
    branch whose other side is still unvisited (the loop's exit)."""
    at = {i["addr"]: k for k, i in enumerate(ins)}
    out, seen, alts, loops = [], {}, [], []
    k = 0
    while k is not None and k < len(ins):
        if k in seen:
            loops.append((seen[k], len(out) - 1))
            k = None
            while alts:
                t = alts.pop()
                if t not in seen:
                    k = t
                    break
            continue
        i = ins[k]
        seen[k] = len(out)
        out.append(i)
        t = at.get(i["target"])
        if i["op"] == "s_endpgm":
            break
        if i["op"] == "s_branch" and t is not None:
            k = t
        elif i["op"].startswith("s_cbranch") and t is not None:
            if t in seen:
                loops.append((seen[t], len(out) - 1))
                k += 1
            elif i["op"] == "s_cbranch_execnz":
                alts.append(k + 1)
                k = t
            else:
                alts.append(t)
                k += 1
        else:
            k += 1
    return out, loops


def analyse(ins):
    """-> (loads, loops): loads = [{addr, op, args, level, cond, section}], loops = [{section, levels, loads}]"""
    p, walked = path(ins)
    pos = {i["addr"]: k for k, i in enumerate(p)}
    # loads alone in the shadow of a short forward s_cbranch_execz, and the error-report path's system-scope loads
    cond = {i["addr"] for i in p if vm_load(i) and "sc0 sc1" in i["args"]}
    for k, i in enumerate(p):
        if i["op"] == "s_cbranch_execz" and i["target"] in pos and k < pos[i["target"]] <= k + 16:
            body = p[k + 1:pos[i["target"]]]
            if sum(map(vm_load, body)) == 1 and not any(is_wait(b) or vm_store(b) or b["op"] == "s_barrier"
                                                        or b["op"].startswith("s_cbranch") for b in body):
                cond.update(b["addr"] for b in body if vm_load(b))
    # load groups (runs of loads without a wait or barrier between them) that hold a non-temporal 16-B load
    groups, cur = [], []
    for k, i in enumerate(p):
        if vm_load(i):
            cur.append(k)
        elif (is_wait(i) or i["op"] == "s_barrier") and cur:
            groups.append(cur)
            cur = []
    if cur:
        groups.append(cur)
    sec_at = {}                                        # path index -> section that starts there
    k_bar = next((k for k, i in enumerate(p) if i["op"] == "s_barrier"), None)
    k_us = k_seg = None
    if k_bar is not None:
        sec_at[k_bar + 1] = 1
        k_us = next((k for k in range(k_bar, len(p)) if vm_store(p[k]) and is_nt(p[k]) and "dwordx2" in p[k]["op"]),
                    None)
    if k_us is not None:
        sec_at[k_us + 1] = 2
        k_seg = next((k for k in range(k_us, len(p)) if vm_load(p[k]) and is_nt(p[k])), None)
    if k_seg is not None:
        stages = [g for g in groups if g[-1] >= k_seg and any(is_nt(p[k]) and "dwordx4" in p[k]["op"] for k in g)][:3]
        for n, g in enumerate(stages):
            sec_at[min(g[0], k_seg) if n == 0 else g[0]] = 3 + n
        if len(stages) == 3:
            k_t = next((k for k in range(stages[2][-1], len(p)) if is_wait(p[k]) and "vmcnt(0)" in p[k]["args"]),
                       None)
            if k_t is not None:
                sec_at[k_t + 1] = 6
    loads, level, fresh, sec = [], 0, False, 0
    lvl_at = []
    for k, i in enumerate(p):
        sec = sec_at.get(k, sec)
        if is_wait(i) and fresh:
            level, fresh = level + 1, False
        lvl_at.append(level)
        if vm_load(i):
            c = i["addr"] in cond
            fresh = fresh or not c
            loads.append(dict(addr=i["addr"], op=i["op"], args=i["args"], level=level, cond=c,
                              section=SECTIONS[sec], k=k))
    loops = []
    for lo, hi in sorted(set(walked), key=lambda x: x[0] - x[1]):      # widest first; nested ones are dropped
        body = [l for l in loads if lo <= l["k"] <= hi]
        if body and not any(lp["lo"] <= lo and hi <= lp["hi"] for lp in loops):
            loops.append(dict(lo=lo, hi=hi, section=body[0]["section"],
                              levels=len({l["level"] for l in body if not l["cond"]}),
                              loads=len(body), cond=sum(l["cond"] for l in body)))
    return loads, loops


def barriers(ins):
    """-> for every s_barrier on the path: the loads issued since the last wait (in flight across it) and the first
    vmcnt wait behind it"""
    p, _ = path(ins)
    out, inflight = [], 0
    for k, i in enumerate(p):
        if vm_load(i):
            inflight += 1
        elif is_wait(i):
            inflight = 0
        elif i["op"] == "s_barrier":
            nxt = next((j for j in p[k + 1:] if is_wait(j) or j["op"] == "s_barrier"), None)
            out.append(dict(addr=i["addr"], inflight=inflight,
                            wait=nxt["args"] if nxt is not None and is_wait(nxt) else None))
    return out


def report(loads, loops, dump=False, bars=()):
    lines = []
    if dump:
        for l in loads:
            lines.append(f"{l['addr']:08x}  L{l['level']:<2d} {'c' if l['cond'] else ' '} {l['section']:16s} "
                         f"{l['op']} {l['args']}")
    lines.append(f"{'section':18s} {'loads':>5s} {'cond':>5s} {'levels':>6s} {'in loops':>8s} {'outside loops':>13s}")
    for s in SECTIONS:
        ls = [l for l in loads if l["section"] == s]
        lp = [x for x in loops if x["section"] == s]
        inl = {l["level"] for l in ls if not l["cond"] and any(x["lo"] <= l["k"] <= x["hi"] for x in lp)}
        outl = {l["level"] for l in ls if not l["cond"] and not any(x["lo"] <= l["k"] <= x["hi"] for x in lp)}
        lines.append(f"{s:18s} {len(ls):5d} {sum(l['cond'] for l in ls):5d} "
                     f"{len({l['level'] for l in ls if not l['cond']}):6d} {len(inl):8d} {len(outl):13d}")
    for x in loops:
        lines.append(f"loop in {x['section']}: {x['loads']} loads ({x['cond']} conditional), {x['levels']} levels per "
                     f"iteration")
    for b in bars:
        lines.append(f"s_barrier at {b['addr']:08x}: {b['inflight']} loads in flight across it, first wait behind it: "
                     f"{b['wait'] or 'none before the next barrier'}")
    lines.append(f"levels along the path: {max([l['level'] for l in loads], default=-1) + 1}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel")
    ap.add_argument("--lib", default=os.path.join(ROOT, "shud-up_amd", "libshud_rhs.so"))
    ap.add_argument("--listing", help="an llvm-objdump -d text of the kernel (instead of --lib)")
    ap.add_argument("--dump", action="store_true", help="list every load")
    a = ap.parse_args()
    text = open(a.listing).read() if a.listing else disassemble(a.lib, a.kernel)
    ins = parse(text)
    if not ins:
        raise SystemExit("no instructions parsed")
    print(report(*analyse(ins), dump=a.dump, bars=barriers(ins)))


if __name__ == "__main__":
    main()
