"""CPU: the run monitors' C-ABI (include/shud_mon.h), their device-free formatters against the plain-Python
restatement tests/mon_py.py byte for byte, Update_IC_STEP / river-type parsing in the C++ host, and the round trip
of a written restart file through the host's INIT_MODE 3 reader.  No GPU calls."""
import ctypes as C
import os
import re
import shutil

import numpy as np
import pytest

import mon_py
from conftest import ROOT
from shud_rhs import abi, host, synth
from shud_rhs import runtime as rt

LIB = os.path.join(ROOT, "shud-up_amd", "libshud_rhs.so")
# values that stress %f: signed zero, the 6th-decimal rounding edge, a 16-digit integer part, a tie-looking tail
STRESS = [-0.0, 4.9999995e-7, 5.0000005e-7, 1e15, 123456.7890125, 0.0, -1.5, 0.1234565, 2.5e-7, 99999.9999995]


def _header_functions():
    txt = open(os.path.join(ROOT, "include", "shud_mon.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(shud_mon_\w+)\s*\(", txt)))


def test_mon_functions_exported_and_bound():
    names = _header_functions()
    assert len(names) >= 12
    assert set(names) == set(abi.MON_FUNCTIONS), set(names) ^ set(abi.MON_FUNCTIONS)
    lib = abi.bind(C.CDLL(LIB))
    for n in names:
        f = getattr(lib, n)
        res, args = abi.MON_FUNCTIONS[n]
        assert f.restype == res and list(f.argtypes) == args, n


def _c_sizeof(struct):
    import subprocess
    src = (f'#include "shud_mon.h"\n#include <stdio.h>\nint main(){{printf("%zu\\n", sizeof({struct}));return 0;}}\n')
    exe = f"/tmp/szmon_{struct}_{os.getpid()}"
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(),
                   check=True)
    out = int(subprocess.check_output([exe]).decode().strip())
    os.unlink(exe)
    return out


def test_mon_spec_layouts_match_header():
    for name, cls in (("ShudFloodSpec", abi.ShudFloodSpec), ("ShudIcSpec", abi.ShudIcSpec)):
        assert C.sizeof(cls) == _c_sizeof(name), name


@pytest.mark.parametrize("n_ele,n_riv,n_lake", [(1, 1, 0), (1, 1, 2), (len(STRESS), 3, 0), (len(STRESS), 3, 2)])
def test_write_ic_host_bytes(tmp_path, n_ele, n_riv, n_lake):
    v = np.array(STRESS)
    cols = [np.roll(v, k)[:n_ele] for k in range(5)]
    riv = np.roll(v, 5)[:n_riv]
    lake = np.array([1e15, -0.0])[:n_lake]
    fn = tmp_path / "x.cfg.ic.update"
    for t in (0.0, 720.0, 1440.25):                       # every write replaces the file
        rt.write_ic_host(fn, t, *cols, riv, lake if n_lake else None)
        assert open(fn, "rb").read() == mon_py.ic_file(t, *cols, riv, lake if n_lake else None)
    assert not os.path.exists(str(fn) + ".tmp")           # the temporary file was renamed over the target


def test_write_ic_host_literal(tmp_path):
    """the layout spelled out once (the odd spacing of the first line is the reference's)"""
    fn = tmp_path / "lit.ic"
    rt.write_ic_host(fn, 1440.25, [-0.0], [4.9999995e-7], [5.0000005e-7], [1e15], [123456.7890125], [0.1])
    assert open(fn, "rb").read() == (b"1\t 6 \t1440.250000\nIndex\tCanopy\tSnow\tSurface\tUnsat\tGW\n"
                                     b"1\t-0.000000\t0.000000\t0.000001\t1000000000000000.000000\t123456.789012\n"
                                     b"1\t2\nIndex\tStage\n1\t0.100000\n")


def test_write_ic_host_missing_directory(tmp_path):
    with pytest.raises(rt.ShudRhsError) as e:
        rt.write_ic_host(tmp_path / "nodir" / "x.ic", 0.0, [0.0], [0.0], [0.0], [0.0], [0.0], [0.0])
    assert e.value.code == abi.SHUD_MON_ERR_IO


def test_format_flood_rows_bytes():
    assert rt.lib().shud_mon_flood_header() == mon_py.FLOOD_HEADER
    n = len(STRESS)
    depth = np.full(n, -2.0)                              # every reach is above its bank
    depth[3] = 1e15                                       # 1e15 > 1e15 is false: no row
    stage = np.array(STRESS)
    q = np.roll(np.array(STRESS), 3)
    q[0], q[1], q[2] = np.inf, -np.inf, np.nan            # glibc prints these through mon_py's snprintf path
    rtype = 1 + np.arange(n) % 3
    ref, cnt = mon_py.flood_rows(61.25, stage, depth, rtype, q)
    idx = np.nonzero(stage > depth)[0]
    assert cnt == idx.size == n - 1
    got = rt.format_flood_rows(61.25, idx, rtype, stage[idx], depth, q[idx])
    assert got == ref
    assert got.startswith(b"61.2\t1\t1\t-0.000000\t-2.000000\tinf\n")
    # one reach, and a NaN / +inf stage through the selection rule of the restatement
    assert rt.format_flood_rows(0.0, [0], [2], [1.5], [1.0], [-0.0]) == b"0.0\t1\t2\t1.500000\t1.000000\t-0.000000\n"
    ref, cnt = mon_py.flood_rows(5.0, [np.nan, np.inf, 1.0], [1.0, 1.0, 1.0], [1, 2, 3], [1.0, 2.0, 3.0])
    assert cnt == 1 and ref == rt.format_flood_rows(5.0, [1], [1, 2, 3], [np.inf], [1.0, 1.0, 1.0], [2.0])
    assert rt.format_flood_rows(5.0, [], [1], [], [1.0], []) == b""


def test_ic_due_rule():
    assert mon_py.ic_due(0.0, 720) and mon_py.ic_due(720.9, 720) and mon_py.ic_due(1440.0, 720)
    assert not mon_py.ic_due(721.0, 720) and not mon_py.ic_due(719.999, 720)


@pytest.fixture(scope="module")
def project_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("monprj")
    synth.write_project(str(d), "syn", 300, days=1.0, max_step=60.0, et_step=60.0, dt_out=60,
                        extra_para={"Update_IC_STEP": 720})
    return d


def test_update_ic_step_and_riv_type(project_dir, tmp_path):
    P = host.Project(str(project_dir), "syn", cwd=str(project_dir))
    assert P.update_ic_step() == 720
    lines = open(project_dir / "syn.sp.riv").read().split("\n")
    nr = int(lines[0].split()[0])
    col = np.array([int(r.split("\t")[2]) for r in lines[2:2 + nr]])
    got = P.riv_type()
    assert got.dtype == np.int32 and np.array_equal(got, col) and got.min() >= 1
    P.close()
    # the key absent: the reference's default
    d2 = tmp_path / "p2"
    shutil.copytree(project_dir, d2)
    para = [ln for ln in open(d2 / "syn.cfg.para") if not ln.startswith("Update_IC_STEP")]
    open(d2 / "syn.cfg.para", "w").writelines(para)
    P2 = host.Project(str(d2), "syn", cwd=str(d2))
    assert P2.update_ic_step() == 1440
    P2.close()


def test_written_ic_loads_back(project_dir, tmp_path):
    """a file from shud_mon_write_ic_host placed as <prj>.cfg.ic (INIT_MODE 3) loads to the written arrays rounded
    to 6 decimals: the '%f' text of each value, read the way the project reader reads a number (mon_py.read_back:
    through long double, which is float(text) except for a rare one-ulp double rounding)"""
    d = tmp_path / "p"
    shutil.copytree(project_dir, d)
    P = host.Project(str(d), "syn", cwd=str(d))
    m = P.model()
    ne, nr = m.num_ele, m.num_riv
    P.close()
    rng = np.random.default_rng(5)
    cols = [rng.uniform(0, s, ne) for s in (0.002, 0.05, 0.01, 6.0, 18.0)]
    cols[0][0], cols[2][0], cols[3][0] = 4.9999995e-7, 5.0000005e-7, 123456.7890125 * 1e-4
    riv = rng.uniform(0.1, 1.0, nr)
    rt.write_ic_host(d / "syn.cfg.ic", 1440.0, *cols, riv)
    P = host.Project(str(d), "syn", cwd=str(d))
    y0, y_is, y_snow = P.array("y0"), P.array("y_is"), P.array("y_snow")
    r6 = lambda a: np.array([mon_py.read_back("%f" % v) for v in a])
    assert np.abs(r6(cols[4]) - np.array([float("%f" % v) for v in cols[4]])).max() <= 2.0 ** -48     # one ulp below 32
    assert np.array_equal(y_is, r6(cols[0])) and np.array_equal(y_snow, r6(cols[1]))
    assert np.array_equal(y0[:ne], r6(cols[2])) and np.array_equal(y0[ne:2 * ne], r6(cols[3]))
    assert np.array_equal(y0[2 * ne:3 * ne], r6(cols[4])) and np.array_equal(y0[3 * ne:3 * ne + nr], r6(riv))
    P.close()
