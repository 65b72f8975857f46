"""CPU: zonal print controls (include/shud_out.h: shud_out_add_zonal) without a device.

(1) The restatement tests/zonal_py.py, before it judges the device (tests/test_gpu_zonal.py): every zone's sum is
    faithful, |S_z - fsum(p)| <= D u sum|p| / (1 - D u) with the D tests/test_ode_kernels.py derives for a vector of the
    zone's length (the zone's own term vector goes through the same tree); it differs in bits from a left-to-right sum
    on the signed family from 65 members up; the integer family hits its closed form.
(2) The create-time plan (csrc/shud_zone.cpp, through shud_zone_plan): members ascending within each zone, col_src
    applied, zone 0 absent, the chunk table covering every member once, the weights in member order, and W_z (formed
    on the host in the device's order) equal to the restatement's bit for bit; every refusal by its message.
(3) shud_project_zones on written tables, with its error cases.
"""
import ctypes as C
import math
import os
import zipfile

import numpy as np
import pytest

import ode_kernels_py as K
import zonal_py as Z
from conftest import GOLDEN, PKG_DIR
from shud_rhs import abi, host

U = 2.0 ** -53
ZONE_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2049]


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _signed(n):
    x, y = K.signed_pair(n)
    return x * y


def _layout(sizes, interleave=False, gap=3):
    """zone[] with zone k+1 of sizes[k] members: contiguous runs (with `gap` zone-0 columns between them), or dealt
    round-robin so every zone's members are strided"""
    if not interleave:
        parts = []
        for k, n in enumerate(sizes):
            parts += [np.full(n, k + 1), np.zeros(gap)]
        return np.concatenate(parts).astype(np.int32)
    left = list(sizes)
    out = []
    while any(left):
        for k in range(len(left)):
            if left[k]:
                out.append(k + 1)
                left[k] -= 1
        out.append(0)
    return np.array(out, dtype=np.int32)


# ---------------------------------------------------------------- (1) the restatement
@pytest.mark.parametrize("interleave", [False, True])
def test_restatement_faithful_and_not_serial(interleave):
    zone = _layout(ZONE_SIZES, interleave)
    nz = len(ZONE_SIZES)
    src = _signed(zone.size)
    w = 1.0 + (np.arange(zone.size) % 7) / 8.0
    for weight in (None, w):
        S = Z.zone_sums(src, zone, nz, weight)
        p = src if weight is None else weight * src
        for k, m in enumerate(Z.members(zone, nz)):
            assert m.size == ZONE_SIZES[k] and (np.diff(m) > 0).all()
            D = 6 + 4 + -(-K.grid_blocks(m.size) // 4096) + 2 + 6 + 4
            bound = D * U * math.fsum(np.abs(p[m])) / (1.0 - D * U)
            assert abs(S[k] - math.fsum(p[m])) <= bound, (k, m.size)
    # the signed family itself as each zone's term vector (the seed tests/test_ode_kernels.py fixes for these sizes)
    for n in [s for s in ZONE_SIZES if s >= 65]:
        t = _signed(n)
        zone1 = np.ones(n, dtype=np.int32)
        assert _bits(Z.zone_sums(t, zone1, 1))[0] != _bits(Z.serial_zone_sums(t, zone1, 1))[0], n
        assert _bits(Z.zone_sums(t, zone1, 1))[0] == _bits(K.device_order_sum(t)), n


def test_restatement_integer_family_and_empty_zone():
    sizes = [1025, 0, 16 * 1024 + 1, 7]
    zone = _layout(sizes, interleave=True)
    nz = len(sizes)
    src = np.zeros(zone.size)
    for k, m in enumerate(Z.members(zone, nz)):
        src[m] = K.integer_entries(m.size)
    S = Z.zone_sums(src, zone, nz, weight=src)                   # p = e * e
    for k, n in enumerate(sizes):
        want = float(sum(c * (v + 1) ** 2 for v, c in enumerate(K.integer_counts(n))))
        assert S[k] == want, (k, S[k], want)
    assert _bits(S[1]) == _bits(0.0)                             # +0.0, not -0.0
    ctl = Z.ZonalControl(zone, nz, op="sum")
    for _ in range(3):
        ctl.export(src)
    assert np.array_equal(ctl.row(1440.0), Z.zone_sums(src, zone, nz) * 3 * (1440.0 / 3))
    assert ctl.num_update == 0 and not ctl.buf.any()


# ---------------------------------------------------------------- (2) the plan unit
def _lib():
    return abi.bind(C.CDLL(os.path.join(PKG_DIR, "libshud_rhs.so")))


def _plan(zone, nz, weight=None, op=abi.SHUD_ZONE_SUM, col_src=None):
    """-> (rc, dict) through shud_zone_plan"""
    lib = _lib()
    zone = np.ascontiguousarray(zone, dtype=np.int32)
    n = zone.size
    w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
    cs = None if col_src is None else np.ascontiguousarray(col_src, dtype=np.int32)
    spec = abi.ShudZoneSpec(nz, zone.ctypes.data_as(abi.c_int32_p), None if w is None else w.ctypes.data_as(abi.c_double_p),
                            op)
    cap = n // 1024 + max(nz, 0) + 1
    member, wm = np.full(n, -1, dtype=np.int32), np.full(n, np.nan)
    zoff = np.zeros(max(nz, 0) + 1, dtype=np.int32)
    cz, cf = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.int32)
    wsum = np.full(max(nz, 1), np.nan)
    nm, nc = C.c_int32(-1), C.c_int32(-1)
    i32 = lambda a: a.ctypes.data_as(abi.c_int32_p)              # noqa: E731
    f64 = lambda a: a.ctypes.data_as(abi.c_double_p)             # noqa: E731
    rc = lib.shud_zone_plan(n, None if cs is None else i32(cs), C.byref(spec), C.byref(nm), i32(member), f64(wm),
                            i32(zoff), C.byref(nc), i32(cz), i32(cf), f64(wsum))
    if rc:
        return rc, lib.shud_rhs_last_error_string().decode()
    return 0, dict(member=member[:nm.value], weight=wm[:nm.value], zone_off=zoff, chunk_zone=cz[:nc.value],
                   chunk_first=cf[:nc.value], wsum=wsum)


def test_plan_on_a_random_zone_table():
    rng = np.random.default_rng(5)
    n, nz = 20000, 9
    zone = rng.choice(np.arange(nz + 1), size=n, p=[0.1, 0.5, 0.2, 0.1, 0.05, 0.03, 0.01, 0.0, 0.009, 0.001])
    zone[zone == 7] = 0                                          # zone 7 is empty
    col_src = rng.permutation(n).astype(np.int32)
    weight = rng.uniform(0.5, 2.0, n)
    rc, p = _plan(zone, nz, weight, abi.SHUD_ZONE_SUM, col_src)
    assert rc == 0, p
    mem = Z.members(zone, nz)
    assert p["member"].size == sum(m.size for m in mem) == int((zone > 0).sum())          # zone 0 is absent
    seen = np.zeros(p["member"].size, dtype=np.int64)
    for k, m in enumerate(mem):
        lo, hi = p["zone_off"][k], p["zone_off"][k + 1]
        assert hi - lo == m.size
        assert np.array_equal(p["member"][lo:hi], col_src[m])    # ascending caller column, col_src applied
        assert np.array_equal(_bits(p["weight"][lo:hi]), _bits(weight[m]))
        ch = np.nonzero(p["chunk_zone"] == k + 1)[0]
        assert ch.size == -(-m.size // 1024)
        assert (np.diff(ch) == 1).all()                          # a zone's partials are contiguous
        for j, c in enumerate(ch):
            first = p["chunk_first"][c]
            assert first == lo + 1024 * j
            seen[first:min(first + 1024, hi)] += 1
    assert (seen == 1).all()                                     # the chunks cover every member once
    assert (np.diff(p["chunk_first"]) > 0).all()
    # identity col_src: the members are the columns themselves
    rc, q = _plan(zone, nz)
    assert rc == 0 and np.array_equal(q["member"], np.concatenate(mem))


@pytest.mark.parametrize("n", ZONE_SIZES + [16 * 1024 + 1, 1024 * 1024 + 1, 4096 * 1024 + 1])
def test_host_order_sum_is_the_device_order(n):
    lib = _lib()
    for t in (_signed(n), np.full(n, -0.0), K.integer_entries(n)):
        t = np.ascontiguousarray(t)
        got = lib.shud_zone_order_sum(t.ctypes.data_as(abi.c_double_p), n)
        assert _bits(got) == _bits(K.device_order_sum(t)), n


def test_plan_weight_sums():
    sizes = [1, 65, 1025, 2049]
    zone = _layout(sizes, interleave=True)
    w = np.abs(_signed(zone.size)) + 0.25
    rc, p = _plan(zone, len(sizes), w, abi.SHUD_ZONE_WMEAN)
    assert rc == 0, p
    want = np.array([K.device_order_sum(w[m]) for m in Z.members(zone, len(sizes))])
    assert np.array_equal(_bits(p["wsum"]), _bits(want))


def test_plan_refusals():
    zone = np.array([1, 2, 0, 2, 1], dtype=np.int32)
    w = np.ones(5)
    cases = [
        (dict(zone=zone, nz=0), r"n_zone = 0"),
        (dict(zone=np.array([1, 3, 0, 2, 1]), nz=2), r"zone\[1\] = 3 outside 0\.\.2"),
        (dict(zone=np.array([1, -1, 0, 2, 1]), nz=2), r"zone\[1\] = -1 outside 0\.\.2"),
        (dict(zone=zone, nz=2, op=abi.SHUD_ZONE_WMEAN), r"SHUD_ZONE_WMEAN needs a weight"),
        (dict(zone=zone, nz=3, weight=w, op=abi.SHUD_ZONE_WMEAN), r"empty zone 3"),
        (dict(zone=zone, nz=2, weight=np.array([1.0, 1.0, 5.0, -1.0, 1.0]), op=abi.SHUD_ZONE_WMEAN),
         r"weight sum of zone 2 is 0"),
        (dict(zone=zone, nz=2, weight=np.array([1.0, 1.0, 5.0, 1.0, np.inf]), op=abi.SHUD_ZONE_WMEAN),
         r"weight sum of zone 1 is inf"),
        (dict(zone=zone, nz=2, col_src=np.array([0, 1, 2, 5, 4])), r"col_src\[3\] = 5 outside the source"),
    ]
    import re
    for kw, pat in cases:
        rc, msg = _plan(kw["zone"], kw["nz"], kw.get("weight"), kw.get("op", abi.SHUD_ZONE_SUM), kw.get("col_src"))
        assert rc == abi.SHUD_ERR_ARG and re.search(pat, msg), (pat, rc, msg)


# ---------------------------------------------------------------- (3) shud_project_zones
@pytest.fixture(scope="module")
def ccw(tmp_path_factory):
    root = tmp_path_factory.mktemp("zones")
    with zipfile.ZipFile(os.path.join(GOLDEN, "input", "ccw.zip")) as z:
        z.extractall(root)
    P = host.Project(os.path.join(root, "input", "ccw"), "ccw", cwd=str(root))
    yield P, root
    P.close()


def _write(path, ids, index=None):
    ids = list(ids)
    with open(path, "w") as f:
        f.write(f"{len(ids)}\t2\nINDEX\tZONE\n")
        for i, z in enumerate(ids):
            f.write(f"{i + 1 if index is None else index[i]}\t{z}\n")
    return str(path)


def test_project_zones(ccw):
    P, root = ccw
    ne = P.model().num_ele
    want = (np.arange(ne) * 7 % 5).astype(np.int32)
    zone, nz = P.zones(_write(root / "ok.zone", want))
    assert nz == 4 and zone.dtype == np.int32 and np.array_equal(zone, want)
    zone, nz = P.zones(_write(root / "one.zone", np.ones(ne, dtype=int)))
    assert nz == 1 and (zone == 1).all()
    with pytest.raises(RuntimeError, match=rf"has {ne - 1} rows, NumEle = {ne}"):
        P.zones(_write(root / "short.zone", want[:-1]))
    frac = [str(v) for v in want]
    frac[10] = "2.5"
    with pytest.raises(RuntimeError, match=r"row 11: zone 2\.5 is not an integer"):
        P.zones(_write(root / "frac.zone", frac))
    neg = want.copy()
    neg[3] = -2
    with pytest.raises(RuntimeError, match=r"row 4: zone -2 is negative"):
        P.zones(_write(root / "neg.zone", neg))
    with pytest.raises(RuntimeError, match=r"does not exist"):
        P.zones(root / "missing.zone")
