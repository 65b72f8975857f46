"""CPU: the device-free NetCDF writer (include/shud_nc.h, csrc/shud_nc.cpp) and the OUTPUT_MODE / NCOUTPUT_CFG keys of
the C++ host.

The writer's files are compared byte for byte with tests/nc_py.py (struct packing written from the classic format
specification and the reference's attribute list) and read back through scipy.io.netcdf_file as an independent
reader.  The host conversion is compared bit for bit with numpy's float64 -> '>f4' cast."""
import os
import re
import struct
import tempfile

import numpy as np
import pytest
from scipy.io import netcdf_file

import nc_py
from shud_rhs import host, synth
from shud_rhs import runtime as rt

HIST = "2000-01-01T00:00:00Z: created by SHUD"
WKT = 'PROJCS["NAD83 / UTM zone 10N",GEOGCS["NAD83"]]\n'
FILL_BITS = 0x7cf00000
# the values of the issue: +-0, a float subnormal, underflow to 0, a round-to-even tie, overflow to inf, +-inf
SPECIAL = np.array([0.0, -0.0, 1e-40, 1e-46, 1.0 + 2.0 ** -24, 3.5e38, np.inf, -np.inf, -1e-40, 1.0 + 3 * 2.0 ** -24,
                    123.456, -9.96921e36])


def _mesh(n):
    """a strip of n triangles over n + 2 nodes (node indices 1-based)"""
    k = np.arange(n + 2)
    x, y = 100.0 * k + 0.25, 50.0 * (k % 2) + 1e6 + k / 3.0
    fn = np.stack([np.arange(n) + 1, np.arange(n) + 2, np.arange(n) + 3], axis=1)
    return dict(node_x=x, node_y=y, face_nodes=fn, face_x=(x[:-2] + x[1:-1] + x[2:]) / 3.0,
                face_y=(y[:-2] + y[1:-1] + y[2:]) / 3.0)


def _icol(sel, n):
    if sel == "all":
        return list(range(1, n + 1))
    if sel == "subset":
        return list(range(1, n + 1, 3))
    return [0, 1, n, n + 1, -5, 2 * n + 7] + ([2] if n > 2 else [])       # out-of-range entries are skipped


def _values(k, seed):
    v = np.random.default_rng(seed).normal(0, 10.0, k)
    m = min(k, SPECIAL.size)
    v[:m] = SPECIAL[:m]
    return v


def _write(tmp_path, kind, n, sel, crs, prefix="prj"):
    """two controls (a known and an unknown variable name), three puts over two records"""
    names = {"ele": ("eleygw", "elezz"), "riv": ("rivqdown", "rivzz"), "lake": ("lakystage", "lakzz")}[kind]
    icol = _icol(sel, n)
    mesh = _mesh(n) if kind == "ele" else None
    base = str(tmp_path / "out" / prefix)
    f = rt.NcFile(kind, n, 20000101, history=HIST, crs_wkt=WKT if crs else None, mesh=mesh)
    ctrls = [(f"{base}.{names[0]}", icol), (f"{base}.{names[1]}", list(range(1, n + 1)))]
    ids = [f.add_var(b, ic) for b, ic in ctrls]
    assert ids == [0, 1]
    puts = [(0, 0.0, _values(len(icol), 1)), (1, 0.0, _values(n, 2)), (0, 60.0, _values(len(icol), 3))]
    for c, t, v in puts:
        f.put(c, t, v)
    path = f.path
    assert f.num_records == 2
    f.close()
    return path, ctrls, puts, mesh


@pytest.mark.parametrize("n", [1, 3, 257])
@pytest.mark.parametrize("sel", ["all", "subset", "oor"])
@pytest.mark.parametrize("kind,crs", [("ele", False), ("ele", True), ("riv", False), ("lake", False)])
def test_file_bytes_match_python_restatement(tmp_path, kind, crs, sel, n):
    path, ctrls, puts, mesh = _write(tmp_path, kind, n, sel, crs)
    assert path == str(tmp_path / "out" / f"prj.{kind}.nc")             # out_dir: the basename's directory, created
    ref = nc_py.build(kind, n, ctrls, puts, HIST, mesh=mesh, crs_wkt=WKT if crs else "", forc_start=20000101)
    got = open(path, "rb").read()
    assert len(got) == len(ref)
    assert got == ref


@pytest.mark.parametrize("kind,crs", [("ele", False), ("ele", True), ("riv", False), ("lake", False)])
def test_independent_reader(tmp_path, kind, crs):
    n = 257
    path, ctrls, puts, mesh = _write(tmp_path, kind, n, "subset", crs)
    icol = np.array(ctrls[0][1])
    with netcdf_file(path, "r", mmap=False) as f:
        assert f.version_byte == 2
        dim, obj, _ = nc_py.KIND[kind]
        want_dims = {"time": None, dim: n}
        if kind == "ele":
            want_dims.update(mesh_node=n + 2, max_face_nodes=3)
        assert dict(f.dimensions) == want_dims                          # time is the unlimited dimension
        _, want_vars = nc_py.variables(kind, n, [nc_py.split_basename(b)[1] for b, _ in ctrls], n + 2,
                                       WKT if crs else "", 20000101)
        assert list(f.variables) == [v[0] for v in want_vars]
        dimnames = ["time", dim, "mesh_node", "max_face_nodes"]
        for name, dd, atts, ty, rec, _ in want_vars:
            v = f.variables[name]
            assert v.dimensions == tuple(dimnames[d] for d in dd), name
            assert v.data.dtype == {nc_py.NC_INT: ">i4", nc_py.NC_FLOAT: ">f4", nc_py.NC_DOUBLE: ">f8"}[ty], name
            assert v.isrec == rec
            assert sorted(v._attributes) == sorted(k for k, _ in atts), name
            for k, val in atts:
                got = v._attributes[k]
                if isinstance(val, str):
                    assert got == val.encode(), (name, k)
                elif k == "_FillValue":
                    assert struct.unpack(">I", struct.pack(">f", got))[0] == FILL_BITS
                    assert got.dtype == np.float32 or np.asarray(got).dtype.kind == "f"
                else:
                    assert int(got) == val and np.asarray(got).dtype.kind == "i", (name, k)
        assert f.variables["time"].units == b"minutes since 2000-01-01 00:00:00 UTC"
        assert f.variables["time"].calendar == b"standard"
        assert np.array_equal(f.variables["time"][:], [0.0, 60.0])
        assert f.Conventions == (b"CF-1.10 UGRID-1.0" if kind == "ele" else b"CF-1.10")
        assert f.title == b"SHUD output: prj" and f.source == b"SHUD" and f.history == HIST.encode()
        ids = f.variables[f"{obj}_id"]
        assert np.array_equal(ids[:], np.arange(1, n + 1)) and ids.start_index == 1
        mask = np.zeros(n, dtype=int)
        mask[icol - 1] = 1
        assert np.array_equal(f.variables[f"{obj}_output_mask"][:], mask)
        known, unknown = [nc_py.split_basename(b)[1] for b, _ in ctrls]
        assert f.variables[known].long_name == nc_py.META[known][1].encode()
        assert f.variables[known].units == nc_py.META[known][0].encode()
        assert f.variables[unknown].long_name == b"SHUD output variable: " + unknown.encode()
        assert not hasattr(f.variables[unknown], "units")
        if kind == "ele":
            assert np.array_equal(f.variables["mesh_node_x"][:], mesh["node_x"])
            assert np.array_equal(f.variables["mesh_node_y"][:], mesh["node_y"])
            assert np.array_equal(f.variables["mesh_face_nodes"][:], mesh["face_nodes"])
            assert f.variables["mesh_face_nodes"].start_index == 1
            assert np.array_equal(f.variables["mesh_face_x"][:], mesh["face_x"])
            assert f.variables["mesh"].cf_role == b"mesh_topology" and f.variables["mesh"].topology_dimension == 2
            assert ("crs" in f.variables) == crs
            assert hasattr(f.variables[known], "grid_mapping") == crs
            if crs:
                assert f.variables["crs"].crs_wkt == WKT.encode() == f.variables["crs"].spatial_ref
        # data: float32 of the put values at the selected columns, fill elsewhere
        d = np.array(f.variables[known][:])
        fillv = np.array([FILL_BITS], dtype=np.uint32).view(np.float32)[0]
        for r, (c, t, vals) in zip((0, 1), (puts[0], puts[2])):
            want = np.full(n, fillv, dtype=np.float32)
            with np.errstate(over="ignore"):
                want[icol - 1] = vals.astype(np.float32)
            assert np.array_equal(d[r].astype(np.float32).view(np.uint32), want.view(np.uint32))
        other = np.array(f.variables[unknown][:]).astype(np.float32)
        assert np.all(other[1].view(np.uint32) == FILL_BITS)            # the 60-minute record: never written


def _read(path):
    with netcdf_file(path, "r", mmap=False) as f:
        return ({k: np.array(v[:]).astype(v.data.dtype.newbyteorder("=")) for k, v in f.variables.items() if v.isrec},
                f._recs)


def test_record_bookkeeping(tmp_path):
    """intervals 60 and 180 over six exports: records in first-appearance order; the coarse control's first write lands
    in the t = 0 record the fine one created; unwritten slabs are fill; numrecs is right after every put"""
    n = 5
    f = rt.NcFile("riv", n, 20000101, history=HIST)
    a = f.add_var(str(tmp_path / "p.rivqdown"), [1, 2, 3, 4, 5])
    b = f.add_var(str(tmp_path / "p.rivystage"), [2, 4])
    path = f.path
    assert not os.path.exists(path)                                     # nothing on disk before the first record
    fill = np.array([FILL_BITS], dtype=np.uint32).view(np.float32)[0]
    want_t, nput = [], 0
    for i in range(1, 7):                                               # export at t = 60 i: left endpoints
        t = 60.0 * i
        f.put(a, t - 60.0, np.full(5, float(i)))
        want_t.append(t - 60.0)
        nput += 1
        v, numrecs = _read(path)
        assert numrecs == f.num_records == len(want_t) and np.array_equal(v["time"], want_t)
        if i % 3 == 0:
            f.put(b, t - 180.0, np.array([10.0 * i, 20.0 * i]))
            v, numrecs = _read(path)
            assert numrecs == len(want_t)                               # an existing record: t - 180 was created earlier
            rec = want_t.index(t - 180.0)
            assert np.array_equal(v["rivystage"][rec], np.array([fill, 10.0 * i, fill, 20.0 * i, fill], dtype=np.float32))
        # every slab not yet written is fill; written ones keep their data
        v, _ = _read(path)
        written_b = {want_t.index(60.0 * k - 180.0) for k in range(3, i + 1, 3)}
        for r in range(len(want_t)):
            assert np.array_equal(v["rivqdown"][r], np.full(5, r + 1.0, dtype=np.float32))
            if r not in written_b:
                assert np.all(v["rivystage"][r].view(np.uint32) == FILL_BITS)
    assert want_t == [0.0, 60.0, 120.0, 180.0, 240.0, 300.0]
    # a time that rounds to an existing record shares it (llround), a new one appends out of order
    f.put(b, 59.6, np.array([1.0, 2.0]))
    f.put(b, -60.0, np.array([3.0, 4.0]))
    v, numrecs = _read(path)
    assert numrecs == 7 and v["time"][-1] == -60.0 and v["rivystage"][1][1] == 1.0 and v["rivystage"][6][3] == 4.0
    with pytest.raises(rt.ShudRhsError, match="after the first record"):
        f.add_var(str(tmp_path / "p.rivqup"), [1])
    f.close()


def test_shared_variable_and_empty_file(tmp_path):
    f = rt.NcFile("lake", 3, 20000101, out_dir=str(tmp_path / "a" / "b"), history=HIST)
    c0 = f.add_var(str(tmp_path / "x" / "q.lakystage"), [1, 3])
    c1 = f.add_var(str(tmp_path / "x" / "q.lakystage"), [2])           # same derived name: one variable (ensureVar)
    assert (c0, c1) == (0, 1)
    assert rt.lib().shud_nc_ctrl_var(f.h, 0) == rt.lib().shud_nc_ctrl_var(f.h, 1) == 0
    path = f.path
    assert path == str(tmp_path / "a" / "b" / "q.lake.nc")              # OUT_DIR wins over the basename's directory
    f.close()                                                           # no put: a valid file with 0 records
    with netcdf_file(path, "r", mmap=False) as g:
        assert g._recs == 0 and g.variables["lakystage"].shape == (0, 3) and list(g.variables["lake_output_mask"][:]) == [1, 0, 1]
    assert open(path, "rb").read() == nc_py.build("lake", 3, [(str(tmp_path / "x" / "q.lakystage"), [1, 3])], [], HIST)
    # no registered control: no file (the reference opens a file in its first sink's onInit)
    g = rt.NcFile("riv", 3, 20000101, out_dir=str(tmp_path / "none"), history=HIST)
    g.close()
    assert not os.path.exists(tmp_path / "none")


def test_refusals(tmp_path):
    with pytest.raises(rt.ShudRhsError, match="4 GiB"):
        rt.NcFile("riv", 1 << 30, 20000101)                             # a 4 GiB record slab
    with pytest.raises(rt.ShudRhsError, match="4 GiB"):
        s, _ = rt.nc_spec("riv", 3, 20000101)
        s.kind, s.n_all, s.num_node = 0, 0, 1 << 29                     # an element file with 4 GiB of node coordinates
        h = rt.C.c_void_p()
        rt._nc_check(rt.lib().shud_nc_create(rt.C.byref(s), rt.C.byref(h)), "shud_nc_create")
    with pytest.raises(rt.ShudRhsError, match="Invalid output dimension"):
        rt.NcFile("lake", 0, 20000101)
    f = rt.NcFile("riv", 4, 20000101, history=HIST)
    with pytest.raises(rt.ShudRhsError, match="Inconsistent"):
        f.add_var(str(tmp_path / "p.rivqdown"), [1], n_all=5)
    with pytest.raises(rt.ShudRhsError, match="Cannot derive"):
        f.add_var(str(tmp_path / "nodot"), [1])
    f.close()
    blocker = tmp_path / "file"
    blocker.write_text("x")
    f = rt.NcFile("riv", 4, 20000101, out_dir=str(blocker), history=HIST)
    c = f.add_var(str(tmp_path / "p.rivqdown"), [1])
    with pytest.raises(rt.ShudRhsError, match="cannot create"):
        f.put(c, 0.0, [1.0])
    with pytest.raises(rt.ShudRhsError):
        f.close()


def test_default_history(tmp_path):
    f = rt.NcFile("riv", 2, 20000101)
    f.add_var(str(tmp_path / "p.rivqdown"), [1, 2])
    path = f.path
    f.close()
    with netcdf_file(path, "r", mmap=False) as g:
        assert re.fullmatch(rb"\d{4}-\d\d-\d\dT\d\d:\d\d:\d\dZ: created by SHUD", g.history)


def test_host_conversion_matches_numpy():
    rng = np.random.default_rng(5)
    v = np.concatenate([SPECIAL, rng.normal(0, 1, 4000) * 10.0 ** rng.integers(-50, 40, 4000),
                        (1.0 + rng.integers(0, 1 << 26, 2000) * 2.0 ** -26) * 2.0 ** rng.integers(-150, 128, 2000)])
    n = v.size
    got = rt.nc_convert(v, np.arange(1, n + 1), n)
    with np.errstate(over="ignore"):
        want = v.astype(">f4")
    assert np.array_equal(got.view(">u4"), want.view(">u4"))
    for x, bits in [(0.0, 0), (-0.0, 0x80000000), (1e-46, 0), (1.0 + 2.0 ** -24, 0x3f800000), (3.5e38, 0x7f800000),
                    (-np.inf, 0xff800000), (1e-40, 71362)]:
        assert int(rt.nc_convert([x], [1], 1).view(">u4")[0]) == bits, x
    assert np.isnan(rt.nc_convert([np.nan], [1], 1)[0])                 # a NaN stays a NaN
    # selection: fill everywhere else, out-of-range entries skipped, extra values ignored
    got = rt.nc_convert([1.0, 2.0, 3.0, 4.0], [5, 0, 2], 5)
    assert list(got.view(">u4")) == [FILL_BITS, 0x40400000, FILL_BITS, FILL_BITS, 0x3f800000]


# ---- OUTPUT_MODE / NCOUTPUT_CFG through the C++ host ----
@pytest.fixture(scope="module")
def proj(tmp_path_factory):
    run = tmp_path_factory.mktemp("run")
    indir = run / "input" / "syn"
    synth.write_project(str(indir), "syn", 300, days=1.0)
    return run, indir, open(indir / "syn.cfg.para").read()


def _load(indir, base, extra):
    with open(indir / "syn.cfg.para", "w") as f:
        f.write(base + extra)
    P = host.Project(str(indir), "syn", cwd=str(indir))
    try:
        return P.ncoutput()
    finally:
        P.close()


def test_cfg_keys(proj):
    run, indir, base = proj
    cfg = indir / "syn.cfg.ncoutput"
    cfg.write_text("# comment\n\nOUT_DIR output/nc\n")
    # no key: LEGACY, no warning; a key without a value: LEGACY with the reference's warning
    c = _load(indir, base, "")
    assert c["output_mode"] == 0 and c["warnings"] == "" and c["ncoutput_cfg"] == ""
    c = _load(indir, base, "OUTPUT_MODE\n")
    assert c["output_mode"] == 0 and "OUTPUT_MODE missing value" in c["warnings"] and "default LEGACY (0)" in c["warnings"]
    for word, mode in [("LEGACY", 0), ("legacy", 0), ("0", 0), ("NETCDF", 1), ("NetCdf", 1), ("1", 1), ("1.0", 1),
                       ("BOTH", 2), ("both", 2), ("2", 2)]:
        c = _load(indir, base, f"OUTPUT_MODE\t{word}\nNCOUTPUT_CFG\tsyn.cfg.ncoutput\n")
        assert c["output_mode"] == mode, word
        if mode:
            # a relative NCOUTPUT_CFG resolves against the .cfg.para's directory; OUT_DIR against the run directory
            assert c["ncoutput_cfg"] == f"{indir}/syn.cfg.ncoutput"
            assert c["out_dir"] == f"{run}/output/nc" and c["crs_wkt"] == "" and c["schema"] == ""
            assert "do not embed CRS information" in c["warnings"]
    for bad in ("3", "NC", "1x", "-1"):
        with pytest.raises(RuntimeError, match="invalid OUTPUT_MODE value"):
            _load(indir, base, f"OUTPUT_MODE {bad}\nNCOUTPUT_CFG syn.cfg.ncoutput\n")
    for mode in ("NETCDF", "BOTH"):
        with pytest.raises(RuntimeError, match="requires NCOUTPUT_CFG"):
            _load(indir, base, f"OUTPUT_MODE {mode}\n")
    with pytest.raises(RuntimeError, match="NCOUTPUT_CFG missing value"):
        _load(indir, base, "NCOUTPUT_CFG\n")
    with pytest.raises(RuntimeError, match="NCOUTPUT_CFG is not readable"):
        _load(indir, base, "OUTPUT_MODE NETCDF\nNCOUTPUT_CFG nothere.cfg\n")
    # absolute paths; CRS_WKT is a file whose text is embedded; SCHEMA is ignored with the reference's warning
    other = run / "elsewhere"
    other.mkdir()
    (other / "crs.wkt").write_text(WKT)
    (run / "rel.wkt").write_text("LOCAL_CS[]")
    cfg2 = other / "nc.cfg"
    cfg2.write_text(f"out_dir {other}/o\nCRS_WKT {other}/crs.wkt\nSCHEMA schema.yaml\n")
    c = _load(indir, base, f"OUTPUT_MODE BOTH\nNCOUTPUT_CFG {cfg2}\n")
    assert c["ncoutput_cfg"] == str(cfg2) and c["out_dir"] == f"{other}/o" and c["crs_wkt"] == WKT
    # relative values of this cfg resolve against ITS run directory: the parent of the parent of its directory
    assert c["schema"] == f"{os.path.dirname(os.path.dirname(str(other)))}/schema.yaml"
    assert "SCHEMA is currently ignored (not implemented)" in c["warnings"]
    assert "do not embed CRS" not in c["warnings"]
    cfg.write_text("CRS_WKT rel.wkt\n")
    c = _load(indir, base, "OUTPUT_MODE 1\nNCOUTPUT_CFG syn.cfg.ncoutput\n")
    assert c["crs_wkt"] == "LOCAL_CS[]" and c["out_dir"] == ""
    cfg.write_text("CRS_WKT missing.wkt\n")
    with pytest.raises(RuntimeError, match="Failed to open CRS_WKT"):
        _load(indir, base, "OUTPUT_MODE 1\nNCOUTPUT_CFG syn.cfg.ncoutput\n")
    cfg.write_text("OUT_DIR\n")
    with pytest.raises(RuntimeError, match="missing value"):
        _load(indir, base, "OUTPUT_MODE 1\nNCOUTPUT_CFG syn.cfg.ncoutput\n")
    # LEGACY never opens the cfg
    c = _load(indir, base, "OUTPUT_MODE LEGACY\nNCOUTPUT_CFG nothere.cfg\n")
    assert c["output_mode"] == 0
    # synth.write_project's keyword arguments write the two keys
    d2 = run / "input" / "syn2"
    synth.write_project(str(d2), "syn2", 300, days=1.0, output_mode="BOTH", ncoutput_cfg="syn2.cfg.ncoutput")
    assert "OUTPUT_MODE\tBOTH\n" in open(d2 / "syn2.cfg.para").read()
    (d2 / "syn2.cfg.ncoutput").write_text("OUT_DIR nc\n")
    P = host.Project(str(d2), "syn2", cwd=str(d2))
    assert P.ncoutput()["output_mode"] == 2 and P.ncoutput()["out_dir"] == f"{run}/nc"
    P.close()


def test_mesh_accessors(proj):
    run, indir, base = proj
    with open(indir / "syn.cfg.para", "w") as f:
        f.write(base)
    P = host.Project(str(indir), "syn", cwd=str(indir))
    m = P.mesh_nodes()
    lines = open(indir / "syn.sp.mesh").read().split("\n")
    ne = int(lines[0].split()[0])
    ele = np.array([ln.split() for ln in lines[2:2 + ne]], dtype=float)
    nn = int(lines[2 + ne].split()[0])
    nodes = np.array([ln.split() for ln in lines[4 + ne:4 + ne + nn]], dtype=float)
    assert np.array_equal(m["face_nodes"], ele[:, 1:4].astype(np.int32)) and m["face_nodes"].min() == 1
    assert np.array_equal(m["node_x"], nodes[:, 1]) and np.array_equal(m["node_y"], nodes[:, 2])
    assert np.array_equal(m["face_x"], P.array("x")) and np.array_equal(m["face_y"], P.array("y"))
    P.close()


def test_reserved_records_are_created_in_index_order(tmp_path):
    """shud_nc_reserve fixes the record order without I/O (the exporting thread, in control order); whichever writer
    arrives first creates every reserved record up to its own, so the file never depends on thread timing"""
    import ctypes as C
    f = rt.NcFile("riv", 3, 20000101, history=HIST)
    a = f.add_var(str(tmp_path / "p.rivqdown"), [1, 2, 3])
    rec = C.c_int64()
    for t, want in ((120.0, 0), (60.0, 1), (120.2, 0), (0.0, 2)):
        assert rt.lib().shud_nc_reserve(f.h, t, C.byref(rec)) == 0 and rec.value == want
    assert f.num_records == 0 and not os.path.exists(f.path)
    with pytest.raises(rt.ShudRhsError, match="after the first record"):
        f.add_var(str(tmp_path / "p.rivqup"), [1])                      # the header is final once a record is reserved
    f.put(a, 60.0, [1.0, 2.0, 3.0])                                     # creates records 0 and 1
    v, numrecs = _read(f.path)
    assert numrecs == 2 and np.array_equal(v["time"], [120.0, 60.0])
    assert np.all(v["rivqdown"][0].view(np.uint32) == FILL_BITS) and list(v["rivqdown"][1]) == [1.0, 2.0, 3.0]
    f.put(a, 0.0, [4.0, 5.0, 6.0])
    v, numrecs = _read(f.path)
    assert numrecs == 3 and np.array_equal(v["time"], [120.0, 60.0, 0.0]) and list(v["rivqdown"][2]) == [4.0, 5.0, 6.0]
    f.close()


def test_header_functions_bound_and_exported():
    """every function include/shud_nc.h declares is exported by libshud_rhs.so and mirrored in abi.NC_FUNCTIONS; the
    ctypes ShudNcSpec has the C layout"""
    import ctypes as C
    import subprocess
    from conftest import ROOT
    from shud_rhs import abi
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "shud_nc.h")).read(), flags=re.S)
    names = set(re.findall(r"\b(shud_nc_\w+)\s*\(", txt))
    assert len(names) >= 12 and names == set(abi.NC_FUNCTIONS), names ^ set(abi.NC_FUNCTIONS)
    for n in names:
        assert hasattr(rt.lib(), n), n
    src = '#include "shud_nc.h"\n#include <stdio.h>\nint main(){printf("%zu\\n", sizeof(ShudNcSpec));return 0;}\n'
    exe = os.path.join(tempfile.mkdtemp(), "sz")
    subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(), check=True)
    assert int(subprocess.check_output([exe]).decode()) == C.sizeof(abi.ShudNcSpec)
