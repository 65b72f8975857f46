"""CPU: the water-balance diagnostics' C-ABI (include/shud_wb.h) is exported and bound, the host's interval rule,
and the restatement's own writer and write gate (tests/wb_py.py) against hand-spelled expectations.  No GPU."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np

import cases
import wb_py
from conftest import ROOT
from shud_rhs import abi, host, shudio, synth

LIB = os.path.join(ROOT, "shud-up_amd", "libshud_rhs.so")


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "shud_wb.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(shud_wb_\w+)\s*\(", txt)))


def _c_sizeof(struct_name):
    src = (f'#include "shud_wb.h"\n#include <stdio.h>\n'
           f'int main(){{printf("%zu\\n", sizeof({struct_name}));return 0;}}\n')
    exe = f"/tmp/sz_{struct_name}_{os.getpid()}"
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(),
                   check=True)
    out = subprocess.check_output([exe]).decode().strip()
    os.unlink(exe)
    return int(out)


def test_wb_abi_exported_and_bound():
    names = _header_functions()
    assert len(names) >= 6 and {"shud_wb_create", "shud_wb_on_et_update", "shud_wb_sample", "shud_wb_maybe_write",
                                "shud_wb_read", "shud_wb_destroy"} <= set(names)
    assert set(names) == set(abi.WB_FUNCTIONS), set(names) ^ set(abi.WB_FUNCTIONS)
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shud-up_amd")])
    lib = C.CDLL(LIB)
    for n in names:
        assert hasattr(lib, n), n
    abi.bind(lib)
    assert lib.shud_rhs_abi_version() == 2                       # the diagnostic does not move the RHS ABI
    assert lib.shud_wb_sample.argtypes == abi.WB_FUNCTIONS["shud_wb_sample"][1]
    for name, cls in (("ShudWbOptions", abi.ShudWbOptions), ("ShudWbOut", abi.ShudWbOut)):
        assert C.sizeof(cls) == _c_sizeof(name), name
    assert abi.SHUD_ARR_COUNT == 37                              # no new SHUD_ARR_* entries


def test_project_wb_interval(tmp_path):
    """dt_qe_ET if positive, else dt_ye_SURF if positive, else 1440 (WaterBalanceDiag.cpp:10-19)"""
    for k, (qe, ys, want) in enumerate([(30, 60, 30), (0, 45, 45), (0, 0, 1440)]):
        d = tmp_path / f"p{k}"
        synth.write_project(str(d), "syn", 300, days=0.1, extra_para={"dt_qe_et": qe, "dt_ye_surf": ys})
        P = host.Project(str(d), "syn", cwd=str(d))
        assert P.wb_interval() == want == wb_py.choose_interval(qe, ys), (qe, ys, P.wb_interval())
        P.close()
    assert host.lib().shud_project_wb_interval(None) == -1


def test_restatement_writer_layout(tmp_path):
    """1024-byte zero-filled header whose second line names the diagnostic, StartTime, NumVar, icol, rows"""
    hb = wb_py.header_bytes("basinwbfull (m3)", 9, forc_start_time=20000101, radiation_input_mode=1,
                            terrain_radiation=1, solar_lonlat_mode="FIXED", lon=-122.71, lat=39.195)
    text = (b"# SHUD output\n# Water-balance diagnostic: basinwbfull (m3)\n# Radiation input mode: SWNET\n"
            b"# Terrain radiation (TSR): ON\n# Solar lon/lat mode: FIXED\n"
            b"# Solar lon/lat (deg): lon=-122.710000, lat=39.195000\n")
    want = text + b"\0" * (1024 - len(text)) + struct.pack("<11d", 20000101.0, 9.0, *range(1, 10))
    assert hb == want and len(hb) == 1024 + 8 * 11
    rows = [(0.0, np.arange(9) * 0.5), (60.0, -np.arange(9) * 1.25)]
    p = tmp_path / "x.basinwbfull.dat"
    with open(p, "wb") as f:
        f.write(hb)
        for t, v in rows:
            rb = wb_py.record_bytes(t, v)
            assert rb == struct.pack("<10d", t, *v)
            f.write(rb)
    d = shudio.read_dat(str(p))
    assert d["start_time"] == 20000101.0 and d["icol"].tolist() == list(range(1, 10))
    assert d["header"].splitlines()[1] == "# Water-balance diagnostic: basinwbfull (m3)"
    assert d["t"].tolist() == [0.0, 60.0] and np.array_equal(d["data"], np.stack([v for _, v in rows]))
    # the five files of a restatement: labels and column counts
    m, y = cases.single_element()
    st = wb_py.host_summary(m, y) + (np.zeros(1), np.zeros(1))
    w = wb_py.WaterBalancePy(m, 60, st, prefix=tmp_path / "one")
    w.close()
    for k, (label, ext) in enumerate(wb_py.LABELS):
        d = shudio.read_dat(str(tmp_path / "one") + ext)
        assert d["header"].splitlines()[1] == f"# Water-balance diagnostic: {label}"
        assert d["icol"].size == (1 if k < 4 else 9) and d["t"].size == 0


def test_maybe_write_gate():
    """t before the first interval, t off the grid, t repeated (maybeWrite :541-550); row time = tf - interval"""
    g = wb_py.write_gate
    assert g(59.999, 60, -1) is None                             # floor 59 < interval
    assert g(0.0, 60, -1) is None
    assert g(60.0, 60, -1) == 60 and g(60.7, 60, -1) == 60       # floor(t)
    assert g(61.0, 60, -1) is None and g(119.9999, 60, 60) is None   # off the grid
    assert g(60.5, 60, 60) is None                               # this floor was written already
    assert g(120.0, 60, 60) == 120
    m, y = cases.single_element()
    st = wb_py.host_summary(m, y) + (np.zeros(1), np.zeros(1))
    w = wb_py.WaterBalancePy(m, 60, st)
    wrote = [w.maybe_write(t, st) for t in (30.0, 59.5, 60.0, 60.0, 60.9, 75.0, 120.2, 180.0)]
    assert wrote == [False, False, True, False, False, False, True, True] and w.rows == 3
    assert wb_py.env_truthy("1") and wb_py.env_truthy("yes") and not any(
        wb_py.env_truthy(s) for s in (None, "", "0", "false", "OFF", "False"))


def test_device_sum_is_a_sum():
    """the restated reduction tree adds every term once (exact on integers), across the block and finalize edges"""
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025, 5000, 4 * 1024 * 1024 + 7):
        v = np.arange(n, dtype=np.float64) % 97.0
        assert wb_py.device_sum(v) == float(v.sum()) == wb_py.seq_sum(v[:6000]) + float(v[6000:].sum()), n
