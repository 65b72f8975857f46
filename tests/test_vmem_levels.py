"""tools/vmem_levels.py: the parser and the level walk on a short canned llvm-objdump listing (no compiler run)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import vmem_levels as vl  # noqa: E402


def _listing(rows):
    """rows of (text, size in bytes) -> objdump text of kernel `k`, addresses from 0x1000; `@N` in a branch's text
    is replaced by the <k+0x..> form of row N"""
    addr, at = 0x1000, []
    for _, size in rows:
        at.append(addr)
        addr += size
    out = ["", "lib.so:\tfile format elf64-amdgpu", "", "Disassembly of section .text:", "",
           f"{0x1000:016x} <k>:"]
    for (text, _), a in zip(rows, at):
        if "@" in text:
            op, n = text.split("@")
            n = int(n)
            text = f"{op}{(at[n] - a - 4) // 4}"
            out.append(f"\t{text:58s} // {a:012X}: BF880000 <k+0x{at[n] - 0x1000:x}>")
        else:
            out.append(f"\t{text:58s} // {a:012X}: DC508000")
    return "\n".join(out) + "\n"


ROWS = [
    ("s_load_dwordx4 s[0:3], s[4:5], 0x0", 8),                      # 0
    ("global_load_dwordx4 v[0:3], v8, s[0:1]", 8),                  # 1  own record                    L0
    ("s_waitcnt vmcnt(0)", 4),                                      # 2
    ("s_barrier", 4),                                               # 3  -> vertical part
    ("s_cbranch_execnz @34", 4),                                    # 4  out-of-line block, taken
    ("v_add_f64 v[4:5], v[0:1], v[2:3]", 8),                        # 5  <- the block returns here
    ("global_load_dword v9, v8, s[2:3] sc0 sc1", 8),                # 6  error-report path: opens no level
    ("s_waitcnt vmcnt(0)", 4),                                      # 7
    ("global_store_dwordx2 v8, v[4:5], s[0:1] nt", 8),              # 8  -> segment section
    ("global_load_dword v10, v8, s[2:3]", 8),                       # 9  loop top                      L2
    ("global_load_dwordx4 v[12:15], v8, s[2:3]", 8),                # 10                               L2
    ("s_waitcnt vmcnt(1)", 4),                                      # 11
    ("global_load_dwordx2 v[16:17], v10, s[2:3]", 8),               # 12                               L3
    ("s_waitcnt vmcnt(0)", 4),                                      # 13
    ("s_cbranch_execz @16", 4),                                     # 14 a stage BC: one load in the shadow
    ("global_load_dwordx2 v[16:17], v[18:19], off", 8),             # 15 conditional                   L4
    ("s_waitcnt vmcnt(0)", 4),                                      # 16
    ("global_store_dwordx4 v8, v[12:15], s[2:3]", 8),               # 17
    ("s_cbranch_execnz @9", 4),                                     # 18 loop back edge
    ("global_load_dwordx4 v[20:23], v8, s[0:1] nt", 8),             # 19 -> edge stage 1               L4
    ("global_load_dwordx2 v[24:25], v11, s[0:1]", 8),               # 20                               L4
    ("s_barrier", 4),                                               # 21
    ("s_waitcnt vmcnt(0)", 4),                                      # 22
    ("global_load_dwordx4 v[20:23], v8, s[0:1] nt", 8),             # 23 -> edge stage 2               L5
    ("s_barrier", 4),                                               # 24
    ("s_waitcnt vmcnt(0)", 4),                                      # 25
    ("s_cbranch_vccz @33", 4),                                      # 26 falls through
    ("global_load_dwordx2 v[24:25], v11, s[0:1]", 8),               # 27 -> edge pass 3                L6
    ("global_load_dwordx4 v[20:23], v8, s[0:1] nt", 8),             # 28                               L6
    ("s_waitcnt vmcnt(1)", 4),                                      # 29
    ("s_waitcnt vmcnt(0)", 4),                                      # 30 -> tail
    ("global_load_dwordx2 v[26:27], v8, s[0:1] nt", 8),             # 31                               L7
    ("s_waitcnt vmcnt(0)", 4),                                      # 32
    ("s_endpgm", 4),                                                # 33
    ("global_load_dwordx2 v[28:29], v8, s[2:3]", 8),                # 34 out of line                   L1
    ("s_waitcnt vmcnt(0)", 4),                                      # 35
    ("s_branch @5", 4),                                             # 36
]


def test_parse_addresses_and_targets():
    ins = vl.parse(_listing(ROWS))
    assert len(ins) == len(ROWS)
    assert ins[0]["addr"] == 0x1000 and ins[1]["addr"] == 0x1008
    assert [i["op"] for i in ins[:4]] == ["s_load_dwordx4", "global_load_dwordx4", "s_waitcnt", "s_barrier"]
    assert ins[4]["target"] == ins[34]["addr"] and ins[36]["target"] == ins[5]["addr"]
    assert ins[18]["target"] == ins[9]["addr"] and ins[14]["target"] == ins[16]["addr"]
    assert ins[1]["target"] is None


def test_parse_branch_without_symbol():
    """a branch printed without the <symbol+off> form: the operand is a dword count from the next instruction"""
    text = ("\ts_cbranch_execz 2                    // 000000001000: BF880002\n"
            "\tglobal_load_dword v1, v0, s[0:1]     // 000000001004: DC508000 01000000\n"
            "\ts_endpgm                             // 00000000100C: BF810000\n")
    ins = vl.parse(text)
    assert ins[0]["target"] == 0x100C


def test_levels_sections_and_loops():
    ins = vl.parse(_listing(ROWS))
    loads, loops = vl.analyse(ins)
    by = {l["addr"]: l for l in loads}
    row = lambda n: by[ins[n]["addr"]]  # noqa: E731
    assert [row(n)["level"] for n in (1, 34, 9, 10, 12, 15, 19, 20, 23, 27, 28, 31)] == \
        [0, 1, 2, 2, 3, 4, 4, 4, 5, 6, 6, 7]
    assert row(6)["cond"] and row(15)["cond"] and not row(12)["cond"] and not row(34)["cond"]
    assert row(6)["level"] == 2                        # the report load's own wait opened no level
    sec = {n: row(n)["section"] for n in (1, 34, 6, 9, 15, 19, 20, 23, 27, 28, 31)}
    assert sec == {1: "prologue", 34: "vertical part", 6: "vertical part", 9: "segment section",
                   15: "segment section", 19: "edge stage 1", 20: "edge stage 1", 23: "edge stage 2",
                   27: "edge pass 3", 28: "edge pass 3", 31: "tail"}
    # the out-of-line block is walked where it runs: between the barrier and the instruction it returns to
    p, _ = vl.path(ins)
    order = [i["addr"] for i in p]
    assert order.index(ins[34]["addr"]) == order.index(ins[4]["addr"]) + 1
    assert order.index(ins[5]["addr"]) == order.index(ins[36]["addr"]) + 1
    assert len(loops) == 1 and loops[0]["section"] == "segment section"
    assert loops[0]["loads"] == 4 and loops[0]["cond"] == 1 and loops[0]["levels"] == 2


def test_report_table():
    loads, loops = vl.analyse(vl.parse(_listing(ROWS)))
    text = vl.report(loads, loops, dump=True)
    lines = text.splitlines()
    assert sum(l.startswith("0000") for l in lines) == len(loads)
    table = {l[:18].strip(): l[18:].split() for l in lines if l[:18].strip() in vl.SECTIONS}
    #                          loads cond levels in-loops outside
    assert table["segment section"] == ["4", "1", "2", "2", "0"]
    assert table["edge stage 1"] == ["2", "0", "1", "0", "1"]
    assert table["vertical part"] == ["2", "1", "1", "0", "1"]
    assert "loop in segment section: 4 loads (1 conditional), 2 levels per iteration" in text
    assert lines[-1] == "levels along the path: 8"


def test_loads_in_flight_across_barriers():
    ins = vl.parse(_listing(ROWS))
    bars = vl.barriers(ins)
    assert [b["addr"] for b in bars] == [ins[3]["addr"], ins[21]["addr"], ins[24]["addr"]]
    assert [b["inflight"] for b in bars] == [0, 2, 1]
    assert [b["wait"] for b in bars] == ["vmcnt(0)", "vmcnt(0)", "vmcnt(0)"]
    text = vl.report(*vl.analyse(ins), bars=bars)
    assert f"s_barrier at {ins[21]['addr']:08x}: 2 loads in flight across it, first wait behind it: vmcnt(0)" in text


def test_kernel_without_landmarks():
    """a kernel with no barrier: everything is prologue, nothing raises"""
    rows = [("global_load_dword v1, v0, s[0:1]", 8), ("s_waitcnt vmcnt(0)", 4),
            ("global_load_dword v2, v1, s[0:1]", 8), ("s_waitcnt vmcnt(0)", 4), ("s_endpgm", 4)]
    loads, loops = vl.analyse(vl.parse(_listing(rows)))
    assert [l["level"] for l in loads] == [0, 1] and {l["section"] for l in loads} == {"prologue"} and not loops
