"""GPU: the NetCDF outputs packed on the device (OUTPUT_MODE NETCDF / BOTH; include/shud_out.h, include/shud_nc.h).

  * the conversion kernels (csrc/shud_out.hip k_snap_nc / k_snap_nc_sel) against the host put of the device-free
    writer: slab bytes equal (a NaN matches any NaN), over the block edges, the four selections, with and without
    a col_src map, two and four intervals per control;
  * BOTH and NETCDF mode through ShudSolver on ccw: every NetCDF value is float32 of the .dat value bit for bit, the
    .dat files are those of a LEGACY run, NETCDF mode leaves no .dat / .csv;
  * shud_gpu end to end against the Python driver on a synthetic project and on qhh (lakes)."""
import glob
import os
import re
import zipfile

import numpy as np
import pytest
from scipy.io import netcdf_file

import shud_gpu_run
from conftest import GOLDEN
from shud_rhs import driver, shudio, synth
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu
HIST = "2000-01-01T00:00:00Z: created by SHUD"
FILL_BITS = 0x7cf00000
# +-0 (a -0 mean: a negative double that underflows), a float subnormal, underflow to 0, a round-to-even tie, overflow
# to inf, +-inf, NaN
SPECIAL = np.array([0.0, -1e-320, 1e-40, 1e-46, 1.0 + 2.0 ** -24, 3.5e38, np.inf, -np.inf, np.nan, -1e-40,
                    1.0 + 3 * 2.0 ** -24, -3.5e38, 123.456])
SIZES = [1, 63, 64, 65, 255, 256, 257, 3000]


@pytest.fixture(scope="module")
def dev():
    """a small handle, for its device allocator and copies"""
    import cases
    m, _ = cases.ccw()
    h = rt.RhsHandle(m)
    yield h
    h.close()


def _words_equal(a, b):
    """two byte strings of big-endian float words: equal, or NaN on both sides"""
    a, b = np.frombuffer(a, dtype=">u4"), np.frombuffer(b, dtype=">u4")
    if a.size != b.size:
        return False
    fa, fb = a.astype(np.uint32).view(np.float32), b.astype(np.uint32).view(np.float32)
    return bool(np.all((a == b) | (np.isnan(fa) & np.isnan(fb))))


def _flags(sel, n):
    f = np.zeros(n, dtype=np.int32)
    if sel == "all":
        return None
    if sel == "third":
        f[::3] = 1
    elif sel == "one":
        f[n // 2] = 1
    else:
        f[n - 1] = 1
    return f


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("sel", ["all", "third", "one", "last"])
def test_conversion_kernel_matches_host_put(tmp_path, dev, sel, mapped):
    """control A: interval 30, a storage (tau 1), one update per interval, so the interval means ARE the source values
    (SPECIAL among them); control B: interval 60, a flux (tau 1440) over two updates.  Exports at t = 30 .. 120: four
    intervals of A, two of B, the sources rewritten before every export.  The device's file must equal, word for word,
    the file the host put writes from the double means; the .dat files beside it (BOTH mode) must be those of a
    legacy-only output set fed the same way."""
    rng = np.random.default_rng(17)
    for n in SIZES:
        d = tmp_path / f"{sel}_{int(mapped)}_{n}"
        flags = _flags(sel, n)
        cols = np.arange(n) if flags is None else np.nonzero(flags)[0]
        perm = rng.permutation(n).astype(np.int32) if mapped else None
        dsrc = dev.device_alloc(8 * n)
        out, leg = rt.Output(stream=dev.stream()), rt.Output(stream=dev.stream())
        out.attach_nc("riv", n, 20000101, out_dir=str(d / "nc"), history=HIST)
        os.makedirs(d / "both")
        os.makedirs(d / "legacy")
        for k, (itv, flux) in enumerate([(30, 0), (60, 1)]):
            name = ("rivystage", "rivqdown")[k]
            out.add(d / "both" / f"p.{name}", dsrc, n, itv, flux, start_time=20000101, flag_io=flags, col_src=perm,
                    nc="riv", legacy=True)
            leg.add(d / "legacy" / f"p.{name}", dsrc, n, itv, flux, start_time=20000101, flag_io=flags, col_src=perm)
        # the host yardstick: the same registrations, fed the double means in the order the reference would
        ref = rt.NcFile("riv", n, 20000101, out_dir=str(d / "ref"), history=HIST)
        ra = ref.add_var(str(d / "both" / "p.rivystage"), cols + 1)
        rb = ref.add_var(str(d / "both" / "p.rivqdown"), cols + 1)
        acc_b = np.zeros(n)
        for i, t in enumerate([30.0, 60.0, 90.0, 120.0]):
            v = rng.normal(0, 100.0, n) * 10.0 ** rng.integers(-30, 30, n)
            v[:min(n, SPECIAL.size)] = np.roll(SPECIAL, i)[:min(n, SPECIAL.size)]
            src = v if perm is None else None
            if perm is not None:                         # column c reads d_src[perm[c]]
                src = np.empty(n)
                src[perm] = v
            dev.h2d(dsrc, src)
            out.export(t)
            leg.export(t)
            with np.errstate(invalid="ignore", over="ignore"):
                ref.put(ra, t - 30.0, ((0.0 + v) * (1.0 / 1))[cols])
                acc_b = acc_b + v
                if i % 2 == 1:
                    ref.put(rb, t - 60.0, (acc_b * (1440.0 / 2))[cols])
                    acc_b = np.zeros(n)
        assert out.rows(0) == 4 and out.rows(1) == 2
        out.close()
        leg.close()
        ref.close()
        dev.device_free(dsrc)
        got, want = open(d / "nc" / "p.riv.nc", "rb").read(), open(d / "ref" / "p.riv.nc", "rb").read()
        nrec, recsize = 4, 8 + 2 * 4 * n
        head = len(want) - nrec * recsize
        assert len(got) == len(want) and got[:4] == b"CDF\x02" and got[:head] == want[:head], (n, sel, mapped)
        assert _words_equal(got[head:], want[head:]), (n, sel, mapped)
        # the fill positions persist and nothing else is fill; the special values arrived
        with netcdf_file(str(d / "nc" / "p.riv.nc"), "r", mmap=False) as f:
            a = np.array(f.variables["rivystage"][:]).astype(np.float32)
            assert a.shape == (4, n) and np.array_equal(f.variables["time"][:], [0.0, 30.0, 60.0, 90.0])
            unsel = np.setdiff1d(np.arange(n), cols)
            assert np.all(a[:, unsel].view(np.uint32) == FILL_BITS)
            assert not np.any(a[:, cols].view(np.uint32) == FILL_BITS)
            if sel == "all" and n >= SPECIAL.size:
                with np.errstate(over="ignore"):
                    w = SPECIAL.astype(np.float32)
                assert _words_equal(a[0, :w.size].astype(">f4").tobytes(), w.astype(">f4").tobytes())
                assert a[0, 1].view(np.uint32) == 0x80000000 and a[0, 2].view(np.uint32) == 71362
        for name in ("p.rivystage.dat", "p.rivqdown.dat"):
            assert open(d / "both" / name, "rb").read() == open(d / "legacy" / name, "rb").read(), (n, sel, name)


def test_attach_errors(tmp_path, dev):
    blocker = tmp_path / "afile"
    blocker.write_text("x")
    out = rt.Output(stream=dev.stream())
    with pytest.raises(rt.ShudRhsError, match="not a directory"):
        out.attach_nc("riv", 4, 20000101, out_dir=str(blocker))          # OUT_DIR that is a regular file
    out.attach_nc("riv", 4, 20000101, out_dir=str(tmp_path / "nc"), history=HIST)
    with pytest.raises(rt.ShudRhsError, match="already attached"):
        out.attach_nc("riv", 4, 20000101)
    dsrc = dev.device_alloc(8 * 8)
    dev.h2d(dsrc, np.arange(8.0))
    with pytest.raises(rt.ShudRhsError, match="no NetCDF file of kind"):
        out.add(tmp_path / "p.lakystage", dsrc, 4, 60, 0, start_time=20000101, nc="lake")
    with pytest.raises(rt.ShudRhsError, match="Inconsistent"):
        out.add(tmp_path / "p.rivqup", dsrc, 5, 60, 0, start_time=20000101, nc="riv")
    out.add(tmp_path / "p.rivqdown", dsrc, 4, 60, 0, start_time=20000101, nc="riv", legacy=False)
    out.export(60.0)
    with pytest.raises(rt.ShudRhsError, match="headers are final"):
        out.add(tmp_path / "p.rivqsub", dsrc, 4, 60, 0, start_time=20000101, nc="riv", legacy=False)
    assert out.rows(0) == 1
    out.close()
    dev.device_free(dsrc)
    assert not glob.glob(str(tmp_path / "*.dat"))                         # NETCDF mode: no legacy file
    with netcdf_file(str(tmp_path / "nc" / "p.riv.nc"), "r", mmap=False) as f:
        assert np.array_equal(f.variables["rivqdown"][:], [[0.0, 1.0, 2.0, 3.0]])


# ---------------------------------------------------------------- the drivers
def _unpack(root, prj, dts):
    """an example project unpacked under root with its output intervals rewritten: dts(key) -> minutes"""
    with zipfile.ZipFile(os.path.join(GOLDEN, "input", f"{prj}.zip")) as z:
        z.extractall(root)
    cfg = os.path.join(root, "input", prj, f"{prj}.cfg.para")
    txt = re.sub(r"^(DT_\w+)\s+\d+", lambda m: f"{m.group(1)}\t{dts(m.group(1))}", open(cfg).read(), flags=re.M)
    open(cfg, "w").write(txt)
    return os.path.join(root, "input", prj)


def _set_mode(indir, prj, base, mode, cfg_text="OUT_DIR ncout\n"):
    with open(os.path.join(indir, f"{prj}.cfg.para"), "w") as f:
        f.write(base if mode is None else base + f"OUTPUT_MODE\t{mode}\nNCOUTPUT_CFG\t{prj}.cfg.ncoutput\n")
    with open(os.path.join(indir, f"{prj}.cfg.ncoutput"), "w") as f:
        f.write(cfg_text)


def _py_driver(indir, prj, cwd, outdir, end_day=-1.0, history=HIST):
    """shud_gpu's set-up and loop in Python (shud_rhs.driver) -> what the checks below read"""
    run = driver.ProjectRun(indir, prj, outdir, cwd=cwd, end_day=end_day, history=history).start()
    run.run()
    m = run.m
    info = dict(decl=run.decl, mesh=run.P.mesh_nodes(), ne=m.num_ele, nr=m.num_riv, nl=getattr(m, "num_lake", 0))
    run.close()
    return info


def _nc_vars(path):
    with netcdf_file(str(path), "r", mmap=False) as f:
        return {k: np.array(v[:]) for k, v in f.variables.items() if v.shape != ()}


def test_both_and_netcdf_modes_on_ccw(tmp_path):
    """twelve 10-minute solver steps of ccw, storages every 20 minutes and fluxes every 60"""
    root = str(tmp_path / "ref")
    indir = _unpack(root, "ccw", lambda k: 20 if k.upper().startswith("DT_YE") else 60)
    base = open(os.path.join(indir, "ccw.cfg.para")).read()
    if not base.endswith("\n"):
        base += "\n"
    end = 2.0 / 24.0
    _set_mode(indir, "ccw", base, None)
    _py_driver(indir, "ccw", root, tmp_path / "legacy", end)
    _set_mode(indir, "ccw", base, "BOTH")
    info = _py_driver(indir, "ccw", root, tmp_path / "both", end)
    _set_mode(indir, "ccw", base, "NETCDF", "OUT_DIR ncout_only\n")
    _py_driver(indir, "ccw", root, tmp_path / "nconly", end)
    dats = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "legacy" / "*.dat")))
    assert len(dats) == len(info["decl"]) >= 15
    # BOTH: the .dat files are the LEGACY run's, byte for byte
    assert dats == sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "both" / "*.dat")))
    for f in dats:
        assert open(tmp_path / "legacy" / f, "rb").read() == open(tmp_path / "both" / f, "rb").read(), f
    ncdir = os.path.join(root, "ncout")                                   # OUT_DIR, relative to the run directory
    assert sorted(os.listdir(ncdir)) == ["ccw.ele.nc", "ccw.riv.nc"]
    ele, riv = _nc_vars(os.path.join(ncdir, "ccw.ele.nc")), _nc_vars(os.path.join(ncdir, "ccw.riv.nc"))
    # records: one per distinct left endpoint, in order of first appearance (20-minute controls come first)
    assert np.array_equal(ele["time"], [0.0, 20.0, 40.0, 60.0, 80.0, 100.0])
    assert np.array_equal(riv["time"], [0.0, 60.0])
    nchecked = 0
    for f in dats:
        d = shudio.read_dat(str(tmp_path / "both" / f))
        name = f[len("ccw."):-len(".dat")]
        nc = ele if d["data"].shape[1] == info["ne"] else riv
        assert d["data"].shape[1] in (info["ne"], info["nr"])
        t = nc["time"]
        for r, tq in enumerate(d["t"]):                                   # time equals the .dat stamps
            rec = int(np.nonzero(t == tq)[0][0])
            got = nc[name][rec].astype(np.float32).view(np.uint32)
            want = d["data"][r].astype(np.float32).view(np.uint32)
            assert np.array_equal(got, want), (f, r)
            nchecked += 1
        assert set(d["t"]) <= set(t)
    assert nchecked >= 2 * len(dats)
    m = info["mesh"]
    assert np.array_equal(ele["mesh_node_x"], m["node_x"]) and np.array_equal(ele["mesh_node_y"], m["node_y"])
    assert np.array_equal(ele["mesh_face_nodes"], m["face_nodes"])
    assert np.array_equal(ele["mesh_face_x"], m["face_x"]) and np.array_equal(ele["mesh_face_y"], m["face_y"])
    assert np.all(ele["element_output_mask"] == 1) and np.array_equal(ele["element_id"], np.arange(1, info["ne"] + 1))
    assert np.all(riv["river_output_mask"] == 1) and np.array_equal(riv["river_id"], np.arange(1, info["nr"] + 1))
    # NETCDF: the same .nc bytes, and no .dat / .csv anywhere
    only = os.path.join(root, "ncout_only")
    for f in ("ccw.ele.nc", "ccw.riv.nc"):
        assert open(os.path.join(only, f), "rb").read() == open(os.path.join(ncdir, f), "rb").read(), f
    assert not glob.glob(str(tmp_path / "nconly" / "*"))


def _shud_gpu(args, history=HIST):
    return shud_gpu_run.run(args, env={"SHUD_NC_HISTORY": history}, check=False)


def test_shud_gpu_both_mode_synthetic(tmp_path):
    """shud_gpu on a synthetic project (a .cfg.output column selection, boundary conditions): OUTPUT_MODE BOTH against
    the Python driver, file for file; --reorder tiles writes the same header and fixed variables; without the key
    the program writes the files it writes today"""
    run = tmp_path / "run"
    src = run / "input" / "syn"
    synth.write_project(str(src), "syn", 2000, days=0.125, max_step=10.0, et_step=60.0, dt_out=60, bc=True,
                        cfg_output=True, output_mode="BOTH", ncoutput_cfg="syn.cfg.ncoutput")
    (run / "crs.wkt").write_text('LOCAL_CS["synthetic"]')
    (src / "syn.cfg.ncoutput").write_text("OUT_DIR nc_cpp\nCRS_WKT crs.wkt\n")
    r = _shud_gpu(["-o", tmp_path / "out_cpp", "-C", src, src, "syn"])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "* \t OUTPUT_MODE: BOTH\n" in r.stdout
    (src / "syn.cfg.ncoutput").write_text("OUT_DIR nc_py\nCRS_WKT crs.wkt\n")
    info = _py_driver(src, "syn", src, tmp_path / "out_py")
    dats = sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / "out_cpp" / "*.dat")))
    assert len(dats) == 24 == len(info["decl"])
    for f in dats:
        assert open(tmp_path / "out_cpp" / f, "rb").read() == open(tmp_path / "out_py" / f, "rb").read(), f
    assert sorted(os.listdir(run / "nc_cpp")) == sorted(os.listdir(run / "nc_py")) == ["syn.ele.nc", "syn.riv.nc"]
    for f in ("syn.ele.nc", "syn.riv.nc"):
        assert open(run / "nc_cpp" / f, "rb").read() == open(run / "nc_py" / f, "rb").read(), f
    ele, riv = _nc_vars(run / "nc_cpp" / "syn.ele.nc"), _nc_vars(run / "nc_cpp" / "syn.riv.nc")
    assert 0 < ele["element_output_mask"].sum() < info["ne"] and 0 < riv["river_output_mask"].sum() < info["nr"]
    gw = shudio.read_dat(str(tmp_path / "out_cpp" / "syn.eleygw.dat"))
    on = np.nonzero(ele["element_output_mask"])[0]
    assert np.array_equal(ele["eleygw"][:, on].astype(np.float32), gw["data"].astype(np.float32))
    off = np.nonzero(ele["element_output_mask"] == 0)[0]
    assert np.all(ele["eleygw"][:, off].astype(np.float32).view(np.uint32) == FILL_BITS)
    with netcdf_file(str(run / "nc_cpp" / "syn.ele.nc"), "r", mmap=False) as f:
        assert f.variables["crs"].crs_wkt == b'LOCAL_CS["synthetic"]' and f.variables["eleygw"].grid_mapping == b"crs"
        assert f.history == HIST.encode()
    # --reorder: the files stay in the input's numbering (masks, ids, mesh, column positions)
    (src / "syn.cfg.ncoutput").write_text("OUT_DIR nc_tiles\nCRS_WKT crs.wkt\n")
    r = _shud_gpu(["-q", "--reorder", "tiles", "-o", tmp_path / "out_tiles", "-C", src, src, "syn"])
    assert r.returncode == 0, r.stdout + r.stderr
    a, b = open(run / "nc_cpp" / "syn.ele.nc", "rb").read(), open(run / "nc_tiles" / "syn.ele.nc", "rb").read()
    nrec = ele["time"].size
    recsize = 8 + 4 * info["ne"] * sum(1 for k, v in ele.items() if v.ndim == 2 and k != "mesh_face_nodes")
    head = len(a) - nrec * recsize
    assert len(a) == len(b) and a[:head] == b[:head]
    tiles = _nc_vars(run / "nc_tiles" / "syn.ele.nc")
    assert np.array_equal(tiles["time"], ele["time"])
    assert np.all(tiles["eleygw"][:, off].astype(np.float32).view(np.uint32) == FILL_BITS)
    # the first hour's values: the reordered run's reductions run in another order; tests/test_gpu_order.py bounds the
    # difference by 1e-6 of the error weight 1e-4 |v| + 1e-4, and each side then rounds to float (2^-24 |v| each)
    va, vb = ele["eleygw"][0, on].astype(np.float64), tiles["eleygw"][0, on].astype(np.float64)
    assert np.all(np.abs(va - vb) <= 1e-6 * (1e-4 * np.abs(va) + 1e-4) + 2.0 ** -23 * np.abs(va))
    # no key: the files of today, and nothing else
    para = open(src / "syn.cfg.para").read()
    open(src / "syn.cfg.para", "w").write("".join(ln for ln in para.splitlines(True)
                                                  if not ln.startswith(("OUTPUT_MODE", "NCOUTPUT_CFG"))))
    r = _shud_gpu(["-o", tmp_path / "out_plain", "-C", src, src, "syn"], history=None)
    assert r.returncode == 0 and "* \t OUTPUT_MODE: LEGACY\n" in r.stdout, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path / "out_plain")) == dats
    for f in dats:
        assert open(tmp_path / "out_plain" / f, "rb").read() == open(tmp_path / "out_cpp" / f, "rb").read(), f


def test_shud_gpu_lake_file_on_qhh(tmp_path):
    """qhh (688 lake elements) over three hours: .ele.nc, .riv.nc and .lake.nc of shud_gpu equal the Python driver's"""
    root = str(tmp_path / "ref")
    indir = _unpack(root, "qhh", lambda k: 60)
    base = open(os.path.join(indir, "qhh.cfg.para")).read()
    if not base.endswith("\n"):
        base += "\n"
    _set_mode(indir, "qhh", base, "NETCDF", "OUT_DIR nc_cpp\n")
    r = _shud_gpu(["-q", "-o", tmp_path / "out_cpp", "-C", root, "-e", "1.125", indir, "qhh"])
    assert r.returncode == 0, r.stdout + r.stderr
    _set_mode(indir, "qhh", base, "NETCDF", "OUT_DIR nc_py\n")
    info = _py_driver(indir, "qhh", root, tmp_path / "out_py", end_day=1.125)
    assert info["nl"] > 0
    names = ["qhh.ele.nc", "qhh.lake.nc", "qhh.riv.nc"]
    assert sorted(os.listdir(os.path.join(root, "nc_cpp"))) == sorted(os.listdir(os.path.join(root, "nc_py"))) == names
    for f in names:
        assert open(os.path.join(root, "nc_cpp", f), "rb").read() == open(os.path.join(root, "nc_py", f), "rb").read(), f
    lake = _nc_vars(os.path.join(root, "nc_cpp", "qhh.lake.nc"))
    assert np.array_equal(lake["time"], [1440.0, 1500.0, 1560.0]) and lake["lakystage"].shape == (3, info["nl"])
    assert np.all(np.isfinite(lake["lakystage"])) and np.all(lake["lake_output_mask"] == 1)
    assert set(lake) >= {"lakystage", "lakatop", "lakvevap", "lakvprcp", "lakqrivin", "lakqrivout", "lakqsurf", "lakqsub"}
    assert not glob.glob(str(tmp_path / "out_cpp" / "*")) and not glob.glob(str(tmp_path / "out_py" / "*"))
