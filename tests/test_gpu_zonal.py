"""GPU: zonal print controls (include/shud_out.h: shud_out_add_zonal) against the numpy restatement tests/zonal_py.py,
which tests/test_zonal.py pins on the CPU.  Every comparison is bit for bit (uint64 views, NaN == NaN), time stamps
included.

(1) known answers through Output.add_zonal over a test-owned device array: zone sizes at the wave, block and finalize
    edges, contiguous / interleaved / c % 3 memberships, the signed and the integer family, SUM and WMEAN, iflux 0 / 1,
    NumUpdate 1 and 3 over two intervals, an empty zone, NaN / inf / -0.0, col_src, a .csv twin;
(2) every refusal by its message, with no file created;
(3) plain and zonal controls interleaved in one set: the plain files are those of a set without the zonal controls;
(4) ProjectRun(zones=...) on ccw, in the file's order and on order="tiles";
(5) checkpoint: a split run with zonal controls equals the straight run byte for byte, also after a killed tail;
(6) shud_gpu --zones.
"""
import glob
import os
import re
import zipfile

import numpy as np
import pytest

import ode_kernels_py as K
import shud_gpu_run
import zonal_py as Z
from conftest import GOLDEN
from shud_rhs import abi, driver, shudio
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu
START = 20000101


@pytest.fixture(scope="module")
def dev():
    """a small handle, for its device allocator and copies"""
    import cases
    m, _ = cases.ccw()
    h = rt.RhsHandle(m)
    yield h
    h.close()


def _bits_equal(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def _layout(sizes, kind, gap=3):
    """zone[]: zone k+1 has sizes[k] members, in contiguous runs with `gap` zone-0 columns after each, or dealt
    round-robin (every zone strided)"""
    if kind == "contiguous":
        parts = []
        for k, n in enumerate(sizes):
            parts += [np.full(n, k + 1), np.zeros(gap)]
        return np.concatenate(parts).astype(np.int32)
    left = np.array(sizes)
    out = []
    while left.any():
        live = np.nonzero(left)[0]
        out.append(np.append(live + 1, 0))
        left[live] -= 1
    return np.concatenate(out).astype(np.int32)


def _csv_text(rows, nz):
    """the .csv twin of shud_out_add: the preamble, then "%.1f\\t" and "%e\\t" per value"""
    head = ("# Timestamp semantics: left endpoint (t-Interval)\n" + f"0\t {nz}\t {START}\n"
            "# Radiation input mode: SWDOWN\n# Terrain radiation (TSR): OFF\n# Solar lon/lat mode: FORCING_FIRST\n"
            "# Solar lon/lat (deg): lon=0.000000, lat=0.000000\nTime_min" + "".join(f" \tX{i + 1}" for i in range(nz)) + "\n")
    return head + "".join(f"{t:.1f}\t" + "".join(f"{v:e}\t" for v in row) + "\n" for t, row in rows)


def _drive(dev, d, zone, nz, sources, controls, times, col_src=None):
    """registers `controls` (dicts: op, weight, interval, iflux, ascii) over one device array of zone.size values,
    exports at `times` with sources[i] written before export i, and compares every file with the restatement.
    -> the expected rows of each control"""
    n = zone.size
    os.makedirs(d, exist_ok=True)
    dsrc = dev.device_alloc(8 * n)
    out = rt.Output(stream=dev.stream())
    ref = []
    for k, c in enumerate(controls):
        out.add_zonal(d / f"z{k}", dsrc, n, c["interval"], c["iflux"], zone, weight=c.get("weight"), op=c["op"],
                      col_src=col_src, start_time=START, n_zone=nz, ascii=c.get("ascii", False))
        ref.append(Z.ZonalControl(zone, nz, c.get("weight"), c["op"], col_src))
    want = [[] for _ in controls]
    with np.errstate(all="ignore"):
        for src, t in zip(sources, times):
            dev.h2d(dsrc, src)
            out.export(t)
            for k, c in enumerate(controls):
                ref[k].export(src)
                if int(np.floor(t + 0.001)) % c["interval"] == 0:
                    want[k].append((float(int(np.floor(t + 0.001)) - c["interval"]), ref[k].row(1440.0 if c["iflux"] else 1.0)))
    for k in range(len(controls)):
        assert out.rows(k) == len(want[k])
    out.close()
    dev.device_free(dsrc)
    for k, c in enumerate(controls):
        got = shudio.read_dat(str(d / f"z{k}.dat"))
        assert got["start_time"] == START and np.array_equal(got["icol"], np.arange(1, nz + 1)), k
        assert np.array_equal(got["t"], [t for t, _ in want[k]]), (k, got["t"])
        for j, (_, row) in enumerate(want[k]):
            assert _bits_equal(got["data"][j], row), (k, c["op"], j, got["data"][j], row)
        if c.get("ascii"):
            assert open(d / f"z{k}.csv").read() == _csv_text(want[k], nz), k
    return want


def _four(weight, ascii=False):
    """SUM and WMEAN, each as a storage at NumUpdate 1 and as a flux at NumUpdate 3"""
    return [dict(op="sum", weight=None, interval=10, iflux=0, ascii=ascii), dict(op="sum", weight=weight, interval=30, iflux=1),
            dict(op="mean", weight=weight, interval=10, iflux=1), dict(op="mean", weight=weight, interval=30, iflux=0)]


TIMES = [10.0, 20.0, 30.0, 40.0, 50.0, 60.0]                     # six exports: two intervals of 30, six of 10
EDGES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]


# ---------------------------------------------------------------- (1) known answers
@pytest.mark.parametrize("kind,mapped", [("contiguous", False), ("interleaved", False), ("interleaved", True)])
def test_zone_sizes_at_the_edges_signed(dev, tmp_path, kind, mapped):
    zone = _layout(EDGES, kind)
    n, nz = zone.size, len(EDGES)
    x, y = K.signed_pair(n)
    base = x * y
    weight = 0.5 + (np.arange(n) % 11) / 4.0
    sources = [np.roll(base, 17 * i) * (1.0 + i / 8.0) for i in range(len(TIMES))]
    perm = np.random.default_rng(3).permutation(n).astype(np.int32) if mapped else None
    _drive(dev, tmp_path / "a", zone, nz, sources, _four(weight, ascii=True), TIMES, col_src=perm)
    if not mapped:                                               # an empty zone under SUM: +0.0
        zone2 = np.where(zone == 3, 0, zone)
        want = _drive(dev, tmp_path / "b", zone2, nz, sources[:3], [dict(op="sum", weight=weight, interval=30, iflux=1)],
                      TIMES[:3])
        assert want[0][0][1].view(np.uint64)[2] == 0


def test_mod3_membership_and_integer_family(dev, tmp_path):
    n = 3 * 2049 + 1
    zone = (np.arange(n) % 3).astype(np.int32)                   # 0 included: two zones of 2049 strided members
    ent = np.zeros(n)
    for m in Z.members(zone, 2):
        ent[m] = K.integer_entries(m.size)
    sources = [ent * (i + 1) for i in range(len(TIMES))]
    want = _drive(dev, tmp_path, zone, 2, sources, _four(ent), TIMES)
    closed = float(sum(c * (v + 1) ** 2 for v, c in enumerate(K.integer_counts(2049))))
    assert [r[1][0] for r in want[1]] == [closed * 6 * 480.0, closed * 15 * 480.0]       # sum(w x), f = 1440 / 3
    plain = float(sum(c * (v + 1) for v, c in enumerate(K.integer_counts(2049))))
    assert [r[1][1] for r in want[0]] == [plain * (i + 1) for i in range(6)]


def test_large_zones_offset_partials_and_second_trip(dev, tmp_path):
    """a zone of 1024*1024 + 1 members after a small one (its partials start at a non-zero offset, the finalize uses
    acc[1]) and one of 4096*1024 + 1 (the finalize's second trip)"""
    sizes = [5, 1024 * 1024 + 1, 4096 * 1024 + 1]
    zone = _layout(sizes, "contiguous", gap=1)
    n = zone.size
    x, y = K.signed_pair(n)
    base = x * y
    weight = 0.5 + (np.arange(n) % 11) / 4.0
    controls = [dict(op="sum", weight=None, interval=10, iflux=0), dict(op="mean", weight=weight, interval=20, iflux=1)]
    want = _drive(dev, tmp_path, zone, 3, [base, np.roll(base, 1)], controls, [10.0, 20.0])
    serial = Z.serial_zone_sums(base, zone, 3)
    assert want[0][0][1].view(np.uint64)[2] != serial.view(np.uint64)[2]          # not a left-to-right sum


def test_special_values(dev, tmp_path):
    sizes = [1024, 70, 1, 2049]
    zone = _layout(sizes, "contiguous", gap=4)
    n = zone.size
    mem = Z.members(zone, 4)
    free = np.nonzero(zone == 0)[0]
    base = np.linspace(-3.0, 5.0, n)
    base[mem[0]] = -0.0                                          # a full chunk of -0.0 terms
    base[mem[2]] = -0.0                                          # and a zone of one
    s0, s1, s2 = base.copy(), base.copy(), base.copy()
    s0[free[0]], s0[free[1]], s0[free[-1]] = np.nan, np.inf, -np.inf     # zone-0 columns reach no zone
    s1[free[0]] = np.nan
    s1[mem[3][1500]] = np.nan                                    # a NaN inside zone 4 only
    s2[mem[1][3]] = np.inf
    weight = np.ones(n)
    controls = [dict(op="sum", weight=None, interval=10, iflux=0), dict(op="mean", weight=weight, interval=10, iflux=1),
                dict(op="sum", weight=weight, interval=30, iflux=0)]
    want = _drive(dev, tmp_path, zone, 4, [s0, s1, s2], controls, TIMES[:3])
    r0, r1, r2 = (want[0][j][1] for j in range(3))
    assert np.isfinite(r0).all() and r0.view(np.uint64)[0] == 0 and r0.view(np.uint64)[2] == 0       # +0.0 from -0.0
    assert np.isnan(r1[3]) and np.isfinite(r1[:3]).all()
    assert r2[1] == np.inf and np.isfinite(r2[[0, 2, 3]]).all()
    assert np.isnan(want[2][0][1][3]) and want[2][0][1][1] == np.inf                     # the 30-minute sums keep both


# ---------------------------------------------------------------- (2) refusals
def test_refusals(dev, tmp_path):
    n = 6
    dsrc = dev.device_alloc(8 * n)
    zone = np.array([1, 2, 0, 2, 1, 1], dtype=np.int32)
    w = np.ones(n)
    out = rt.Output(stream=dev.stream())
    cases = [
        (dict(zone=zone, n_zone=0), r"n_zone = 0"),
        (dict(zone=np.array([1, 2, 0, 3, 1, 1]), n_zone=2), r"zone\[3\] = 3 outside 0\.\.2"),
        (dict(zone=zone, flag_io=np.ones(n, dtype=np.int32)), r"flag_io"),
        (dict(zone=zone, op="mean"), r"SHUD_ZONE_WMEAN needs a weight"),
        (dict(zone=zone, op="mean", weight=w, n_zone=3), r"empty zone 3"),
        (dict(zone=zone, op="mean", weight=np.array([1.0, 2.0, 1.0, -2.0, 1.0, 1.0])), r"weight sum of zone 2 is 0"),
        (dict(zone=zone, op="mean", weight=np.array([1.0, 2.0, 1.0, 2.0, np.inf, 1.0])), r"weight sum of zone 1 is inf"),
        (dict(zone=zone, nc="ele"), r"nc = 'ele'.*no NetCDF sink"),
        (dict(zone=zone, col_src=np.array([0, 1, 2, 3, 4, 6])), r"col_src\[5\] = 6 outside the source"),
    ]
    for k, (kw, pat) in enumerate(cases):
        with pytest.raises(rt.ShudRhsError, match=pat) as ei:
            out.add_zonal(tmp_path / f"bad{k}", dsrc, n, 10, 0, **kw)
        assert ei.value.code == abi.SHUD_ERR_ARG, pat
    assert not os.listdir(tmp_path)                              # nothing created
    out.add_zonal(tmp_path / "ok", dsrc, n, 10, 0, zone)         # and the set is still usable
    dev.h2d(dsrc, np.arange(6.0))
    out.export(10.0)
    assert out.rows(0) == 1
    out.close()
    dev.device_free(dsrc)
    assert np.array_equal(shudio.read_dat(str(tmp_path / "ok.dat"))["data"], [[0.0 + 4.0 + 5.0, 1.0 + 3.0]])


# ---------------------------------------------------------------- (3) a mixed set
def test_mixed_set_leaves_plain_controls_alone(dev, tmp_path):
    n = 5000
    rng = np.random.default_rng(9)
    zone = rng.integers(0, 8, n).astype(np.int32)
    weight = rng.uniform(0.5, 2.0, n)
    flags = (np.arange(n) % 3 != 0).astype(np.int32)
    perm = rng.permutation(n).astype(np.int32)
    dsrc = dev.device_alloc(8 * n)
    mixed, plain = rt.Output(stream=dev.stream()), rt.Output(stream=dev.stream())
    for d in ("mixed", "plain"):
        os.makedirs(tmp_path / d)

    def add_plain(o, d):
        o.add(tmp_path / d / "p0", dsrc, n, 10, 0, start_time=START)
        yield
        o.add(tmp_path / d / "p1", dsrc, n, 30, 1, start_time=START, flag_io=flags, col_src=perm, ascii=True)
        yield
        o.add(tmp_path / d / "p2", dsrc, 100, 20, 1, start_time=START)
        yield
    for _ in add_plain(plain, "plain"):
        pass
    zk = []
    for k, _ in enumerate(add_plain(mixed, "mixed")):            # plain, zonal, plain, zonal, plain, zonal
        zk.append(mixed.add_zonal(tmp_path / "mixed" / f"z{k}", dsrc, n, (10, 30, 20)[k], k % 2, zone,
                                  weight=weight, op=("sum", "mean", "sum")[k], start_time=START))
    assert zk == [1, 3, 5]
    ref = [Z.ZonalControl(zone, 7, weight, op) for op in ("sum", "mean", "sum")]
    want = [[], [], []]
    for i, t in enumerate(TIMES):
        src = rng.normal(0.0, 10.0, n)
        dev.h2d(dsrc, src)
        mixed.export(t)
        plain.export(t)
        for k in range(3):
            ref[k].export(src)
            if int(t) % (10, 30, 20)[k] == 0:
                want[k].append(ref[k].row(1440.0 if k % 2 else 1.0))
    mixed.close()
    plain.close()
    dev.device_free(dsrc)
    for f in ("p0.dat", "p1.dat", "p1.csv", "p2.dat"):
        a, b = open(tmp_path / "mixed" / f, "rb").read(), open(tmp_path / "plain" / f, "rb").read()
        assert a == b and len(a) > 1100, f
    for k in range(3):
        got = shudio.read_dat(str(tmp_path / "mixed" / f"z{k}.dat"))["data"]
        assert _bits_equal(got, np.array(want[k])), k


# ---------------------------------------------------------------- (4) ProjectRun(zones=...) on ccw
def _ccw(root, dt=None):
    with zipfile.ZipFile(os.path.join(GOLDEN, "input", "ccw.zip")) as z:
        z.extractall(root)
    src = os.path.join(root, "input", "ccw")
    if dt is not None:                                           # every print control at `dt` minutes
        para = os.path.join(src, "ccw.cfg.para")
        text = re.sub(r"^(DT_\w+)\s+\d+", rf"\1\t{dt}", open(para).read(), flags=re.M)
        open(para, "w").write(text)
    return src


STEPS = 12


@pytest.mark.parametrize("order", [None, "tiles"])
def test_project_run_zones(tmp_path, order):
    root = tmp_path / "prj"
    src = _ccw(root)
    leaf = lambda d: d["basename"].rsplit(".", 1)[1]             # noqa: E731
    import cases
    ne, step = cases.ccw()[0].num_ele, 10

    def override(k, d):
        """the storages at every solver step (f = 1), the other element controls every third"""
        if d["n_all"] != ne or d["array"] in driver.ARR_NOT_ELE:
            return {}
        return dict(interval=step if leaf(d).startswith("eley") else 3 * step)
    zone = ((np.arange(ne) * 7 + 2) % 5).astype(np.int32)        # 0 included
    run = driver.ProjectRun(src, "ccw", tmp_path / "out", cwd=root, order=order, override=override, zones=zone,
                            control=dict(reltol=1e-6, abstol=1e-6, init_step=1e-3))
    assert run.c["solver_step"] == step and run.m.num_ele == ne
    assert (order is not None) == run.h.ordered
    twins = {os.path.basename(n): n for n in run.zonal}
    ele = [d for d in run.decl if d["n_all"] == ne and d["array"] not in driver.ARR_NOT_ELE]
    assert len(twins) == len(ele) >= 15 and all(d["flag_io"] is None for d in ele)
    area = np.asarray(run.m.ele["area"])
    inv = run.h.order()[2] if run.h.ordered else None
    flux = [d for d in ele if not leaf(d).startswith("eley")]
    steps = {leaf(d): [] for d in flux}                          # the per-step source values, as the device holds them

    def on_output(i, t, y):
        for d in flux:
            p, n = run.h.device_array(d["array"])
            a = run.h.d2h(np.empty(n), p)
            steps[leaf(d)].append(a[d["column"] * ne:(d["column"] + 1) * ne] if d["column"] >= 0 else a)
    y0 = run.P.array("y0").copy()
    y0[:ne] += 0.05                                              # ponded water: a transient to resolve
    run.start(y0).run(STEPS, on_output=on_output)
    run.close()
    nsum = 0
    for d in ele:
        name = leaf(d)
        total = name.startswith("eleq")
        nsum += total
        twin = shudio.read_dat(d["basename"].rsplit(".", 1)[0] + ".zone." + name + ".dat")
        full = shudio.read_dat(d["basename"] + ".dat")
        assert np.array_equal(twin["icol"], [1, 2, 3, 4]) and twin["start_time"] == full["start_time"]
        assert twin["header"] == full["header"] and np.array_equal(twin["t"].view(np.uint64), full["t"].view(np.uint64))
        if name.startswith("eley"):
            # f = 1: the per-element rows ARE the exported source values (in the file's numbering)
            assert twin["t"].size == STEPS
            ctl = Z.ZonalControl(zone, 4, area, "mean")
            for j in range(STEPS):
                ctl.export(full["data"][j])
                assert _bits_equal(twin["data"][j], ctl.row(1.0)), (name, j)
        else:
            assert twin["t"].size == STEPS // 3 and d["iflux"] == (0 if name.startswith("rn_") else 1)
            ctl = Z.ZonalControl(zone, 4, None if total else area, "sum" if total else "mean", col_src=inv)
            for j in range(STEPS):
                ctl.export(steps[name][j])
                if j % 3 == 2:
                    assert _bits_equal(twin["data"][j // 3], ctl.row(1440.0 if d["iflux"] else 1.0)), (name, j)
    assert nsum >= 2                                             # ccw declares eleqsurf and eleqsub


# ---------------------------------------------------------------- (5) checkpoint
INTERVALS = (20, 30)


class ZRun(driver.ProjectRun):
    """tests/test_gpu_ckpt.py's run (ccw with ponded water, tolerances 1e-6, .dat and .csv controls at two intervals)
    with the zonal twins"""

    def __init__(self, root, src, outdir, zone, resume=False):
        super().__init__(src, "ccw", outdir, cwd=root, resume=resume, zones=zone,
                         control=dict(reltol=1e-6, abstol=1e-6, init_step=1e-3),
                         override=lambda k, d: dict(interval=INTERVALS[k % 2], binary=True, ascii=k % 3 == 0))

    def start(self):
        y0 = self.P.array("y0").copy()
        y0[:self.m.num_ele] += 0.05
        return super().start(y0)

    def files(self):
        self.close()
        return {os.path.basename(f): open(f, "rb").read() for f in sorted(glob.glob(os.path.join(self.outdir, "*")))
                if not f.endswith(".ckpt")}


def test_checkpoint_split_equals_straight(tmp_path):
    root = tmp_path / "prj"
    src = _ccw(root)
    import cases
    ne = cases.ccw()[0].num_ele
    zone = (np.arange(ne) % 5).astype(np.int32)
    straight = ZRun(root, src, tmp_path / "straight", zone).start()
    straight.run(STEPS)
    want = straight.files()
    zonal = [f for f in want if ".zone." in f]
    assert len(zonal) >= 20 and any(f.endswith(".csv") for f in zonal)
    assert all(len(want[f]) > 1100 for f in zonal if f.endswith(".dat"))
    for tail in (0, 3):                                          # tail: steps run on after the snapshot, then lost
        out = tmp_path / f"split{tail}"
        path = tmp_path / f"run{tail}.ckpt"
        a = ZRun(root, src, out, zone).start()
        a.run(4)
        a.sv.snapshot(path, output=a.out, monitors=a.mon)
        a.sv.flush_snapshot()
        if tail:
            a.run(tail)
        a.close()
        b = ZRun(root, src, out, zone, resume=True).restore(path)
        assert b.sv.step == 4
        b.run(STEPS - 4)
        got = b.files()
        assert sorted(got) == sorted(want)
        for f in want:
            assert got[f] == want[f], (tail, f, len(got[f]), len(want[f]))
    # an output set without the zonal controls does not take this checkpoint
    c = driver.ProjectRun(src, "ccw", tmp_path / "split0", cwd=root, resume=True,
                          control=dict(reltol=1e-6, abstol=1e-6, init_step=1e-3),
                          override=lambda k, d: dict(interval=INTERVALS[k % 2], binary=True, ascii=k % 3 == 0))
    with pytest.raises(rt.ShudRhsError, match="device sections"):
        c.restore(tmp_path / "run0.ckpt")
    c.close()


def test_checkpoint_tells_a_zonal_control_from_a_plain_one(tmp_path):
    """a zonal control with NZ = 4 and a plain control with n_all = 4 under the same name agree in everything out.host
    compares per control (numvar, interval, start time, files) and in their device sections: only the zone_op trailer
    tells them apart, in both directions.  The section of a set without zonal controls has no trailer: it is, byte
    for byte in length, the section written before zonal controls existed (int32 count, then 52 bytes per control)."""
    import ctypes as C
    root = tmp_path / "prj"
    src = _ccw(root)
    zone = np.array([1, 2, 0, 4, 3, 3, 1], dtype=np.int32)

    def make(kind, resume):
        r = driver.ProjectRun(src, "ccw", tmp_path / "out", cwd=root, resume=resume, override=lambda k, d: None,
                              control=dict(reltol=1e-6, abstol=1e-6, init_step=1e-3))
        assert r.decl == []
        r.d_own = r.h.device_alloc(8 * 8)
        r.h.h2d(r.d_own, np.arange(8.0))
        if kind == "zonal":
            r.out.add_zonal(tmp_path / "out" / "x", r.d_own, zone.size, 20, 0, zone, start_time=START)
        else:
            r.out.add(tmp_path / "out" / "x", r.d_own, 4, 20, 0, start_time=START)
        return r

    def words(path):
        raw, nw = np.zeros(64, dtype=np.uint64), C.c_uint64()
        assert rt.lib().shud_ckpt_read_section(str(path).encode(), b"out.host", raw.ctypes.data_as(abi.c_uint64_p), 64,
                                               C.byref(nw)) == 0
        return nw.value
    for kind, other, pat, nwords in (("zonal", "plain", r"field zone_op differs: the checkpoint's output set has zonal", 9),
                                     ("plain", "zonal", r"field zone_op is missing", 7)):
        path = tmp_path / f"{kind}.ckpt"
        a = make(kind, False).start()
        a.run(3)
        a.sv.snapshot(path, output=a.out, monitors=a.mon)
        a.sv.flush_snapshot()
        a.close()
        assert words(path) == nwords                             # 4 + 52 bytes; the trailer adds a tag and one int32
        b = make(other, True)
        with pytest.raises(rt.ShudRhsError, match=pat):
            b.restore(path)
        b.close()
        c = make(kind, True).restore(path)                       # and the same kind takes it
        assert c.sv.step == 3
        c.run(1)
        assert c.out.rows(0) == 2
        c.close()


# ---------------------------------------------------------------- (6) shud_gpu --zones
def test_shud_gpu_zones(tmp_path):
    root = tmp_path / "prj"
    src = _ccw(root, dt=30)
    import cases
    ne = cases.ccw()[0].num_ele
    zone = (np.arange(ne) % 5).astype(np.int32)
    zfile = tmp_path / "ccw.zone"
    with open(zfile, "w") as f:
        f.write(f"{ne}\t2\nINDEX\tZONE\n" + "".join(f"{i + 1}\t{z}\n" for i, z in enumerate(zone)))
    common = ["-q", "-C", root, "-n", STEPS]
    launches = lambda r: shud_gpu_run.json_line(r)["out_launches"]                                    # noqa: E731
    lz = launches(shud_gpu_run.run(common + ["-o", tmp_path / "z", "--zones", zfile, src, "ccw"]))
    shud_gpu_run.run(common + ["-o", tmp_path / "z_tiles", "--zones", zfile, "--reorder", "tiles", src, "ccw"])
    lp = launches(shud_gpu_run.run(common + ["-o", tmp_path / "plain", src, "ccw"]))
    # What the output set launched before zonal controls existed, from its shud_out_export: ONE k_accumulate per export
    # over every control, and one k_snap per finished row of a control without a NetCDF sink.  Here: 12 exports, and
    # every control finishes 4 intervals of 30 minutes, so the rows are counted from the files themselves.  Without
    # --zones that is all, by name and by count.
    rows = lambda d, keep: sum(shudio.read_dat(f)["t"].size for f in glob.glob(str(tmp_path / d / "*.dat"))     # noqa: E731
                               if keep(os.path.basename(f)))
    n_plain = len(glob.glob(str(tmp_path / "plain" / "*.dat")))
    assert n_plain >= 20 and rows("plain", lambda f: True) == 4 * n_plain
    assert lp == {"k_accumulate": STEPS, "k_snap": 4 * n_plain, "k_snap_nc": 0, "k_snap_nc_sel": 0, "k_zone_partial": 0,
                  "k_zone_final": 0, "k_snap_wmean": 0}, lp
    # with --zones: two launches per export for all twins; the eleq* sums end through k_snap, the means through
    # k_snap_wmean, one launch per finished row each
    n_sum = rows("z", lambda f: ".zone.eleq" in f)
    n_mean = rows("z", lambda f: ".zone." in f and ".zone.eleq" not in f)
    assert n_sum >= 8 and n_mean >= 52
    assert lz == {"k_accumulate": STEPS, "k_snap": 4 * n_plain + n_sum, "k_snap_nc": 0, "k_snap_nc_sel": 0,
                  "k_zone_partial": STEPS, "k_zone_final": STEPS, "k_snap_wmean": n_mean}, lz
    run = driver.ProjectRun(src, "ccw", tmp_path / "py", cwd=root, zones=str(zfile)).start()
    run.run(STEPS)
    run.close()
    run = driver.ProjectRun(src, "ccw", tmp_path / "py_plain", cwd=root).start()
    run.run(STEPS)
    assert run.out.launches() == lp
    run.close()
    run = driver.ProjectRun(src, "ccw", tmp_path / "py_tiles", cwd=root, order="tiles", zones=str(zfile)).start()
    run.run(STEPS)
    run.close()
    names = lambda d: sorted(os.path.basename(f) for f in glob.glob(str(tmp_path / d / "*.dat")))     # noqa: E731
    twins = [f for f in names("z") if ".zone." in f]
    assert len(twins) >= 15 and names("z") == names("py") == names("z_tiles")
    for f in names("z"):
        a, b = open(tmp_path / "z" / f, "rb").read(), open(tmp_path / "py" / f, "rb").read()
        assert a == b, f
    for f in names("z_tiles"):                                   # the C++ driver's own weight and column maps
        a, b = open(tmp_path / "z_tiles" / f, "rb").read(), open(tmp_path / "py_tiles" / f, "rb").read()
        assert a == b, f
    assert len(twins) == (n_sum + n_mean) // 4
    for f in twins:
        d = shudio.read_dat(str(tmp_path / "z" / f))
        assert np.array_equal(d["icol"], [1, 2, 3, 4]) and np.array_equal(d["t"], [0.0, 30.0, 60.0, 90.0]), f
        assert np.isfinite(d["data"]).all()
    # a run without --zones writes exactly the files it wrote before, with the bytes of the run with them
    assert names("plain") == names("py_plain") == [f for f in names("z") if ".zone." not in f]
    for f in names("plain"):
        a = open(tmp_path / "plain" / f, "rb").read()
        assert a == open(tmp_path / "py_plain" / f, "rb").read() == open(tmp_path / "z" / f, "rb").read(), f
    # OUTPUT_MODE NETCDF has no legacy files: refused
    with open(os.path.join(src, "ccw.cfg.para"), "a") as f:
        f.write("OUTPUT_MODE\tNETCDF\nNCOUTPUT_CFG\tccw.cfg.ncoutput\n")
    with open(os.path.join(src, "ccw.cfg.ncoutput"), "w") as f:
        f.write("OUT_DIR ncout\n")
    r = shud_gpu_run.run(common + ["-o", tmp_path / "nc", "--zones", zfile, src, "ccw"], check=False)
    assert r.returncode != 0 and "--zones cannot be combined with OUTPUT_MODE NETCDF" in r.stderr
