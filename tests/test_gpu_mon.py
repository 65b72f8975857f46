"""GPU: the run monitors on the device (include/shud_mon.h, csrc/shud_mon.hip) on plain device tensors, against the
plain-Python restatement tests/mon_py.py byte for byte.

Flood compaction: the kernels use 256-thread blocks (B = 256; 4 waves of 64), so the reach counts straddle the wave
(63/64/65), the block (255/256/257) and several blocks (1023/1025, 4099 = 17 blocks); 65537 reaches are 257 blocks,
one more than the single scan block takes per pass, so its carry between passes is used.  IC pack: element counts
at the same wave / block edges."""
import numpy as np
import pytest
import torch

import mon_py
from shud_rhs import abi
from shud_rhs import runtime as rt

pytestmark = pytest.mark.gpu
B = 256


def _stream():
    return torch.cuda.current_stream().cuda_stream or None


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()


def _patterns(nr, rng):
    """(name, stage) with bank depth 1.0 everywhere"""
    below = lambda: rng.uniform(0.0, 0.999, nr)
    above = lambda: rng.uniform(1.001, 3.0, nr)
    pats = [("all", above())]
    s = below()
    s[::2] = above()[::2]
    pats.append(("every_second", s))
    s = below()
    s[0] = 1.5
    pats.append(("first", s))
    s = below()
    s[-1] = 2.5
    pats.append(("last", s))
    s = below()
    s[[i for i in (B - 1, B, B + 1) if i < nr]] = 1.25
    pats.append(("block_edge", s))
    pats.append(("exactly_bank", np.full(nr, 1.0)))            # strict >: no row
    s = above()
    s[::3] = np.nan                                            # NaN > 1.0 is false: no row
    pats.append(("nan", s))
    s = below()
    s[::5] = np.inf                                            # +inf > 1.0: a row
    pats.append(("inf", s))
    return pats


@pytest.mark.parametrize("nr", [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, B * B + 1])
def test_flood_compaction(tmp_path, nr):
    rng = np.random.default_rng(1000 + nr)
    depth = np.full(nr, 1.0)
    rtype = 1 + np.arange(nr) % 3
    stage, q = _dev(np.zeros(nr)), _dev(np.zeros(nr))
    mon = rt.RunMonitors(stream=_stream())
    fn = tmp_path / "syn.flood.csv"
    mon.add_flood(fn, stage, q, nr, depth, rtype)
    # none above the bank: the header only
    s0, q0 = rng.uniform(0.0, 0.999, nr), rng.normal(0.0, 1e4, nr)
    stage.copy_(torch.from_numpy(s0))
    q.copy_(torch.from_numpy(q0))
    mon.flood(60.0)
    mon.flush()
    assert open(fn, "rb").read() == mon_py.FLOOD_HEADER
    assert mon.flood_last() == 0 and mon.flood_rows() == 0
    # successive calls with different t and patterns into the same file, no flush in between
    calls = [(60.0, s0, q0)]
    for k, (name, s) in enumerate(_patterns(nr, rng)):
        qk = rng.normal(0.0, 1e4, nr)
        qk[0] = -0.0
        stage.copy_(torch.from_numpy(s))
        q.copy_(torch.from_numpy(qk))
        t = 120.0 + 60.0 * k + 0.25 * (k % 2)
        mon.flood(t)
        calls.append((t, s, qk))
    mon.flush()
    ref, total, last = mon_py.flood_file(calls, depth, rtype)
    got = open(fn, "rb").read()
    assert got == ref, f"nr={nr}: {len(got)} vs {len(ref)} bytes"
    assert mon.flood_rows() == total and total > 0
    assert mon.flood_last() == last == 1
    assert mon.time_flood(3) > 0.0                             # the timing helper runs and writes nothing
    mon.flush()
    assert open(fn, "rb").read() == ref
    mon.close()


@pytest.mark.parametrize("n_lake", [0, 3])
@pytest.mark.parametrize("nr", [1, 65])
@pytest.mark.parametrize("ne", [1, 63, 64, 65, 257, 1025])
def test_ic_pack(tmp_path, ne, nr, n_lake):
    rng = np.random.default_rng(7 * ne + nr + n_lake)

    def draw():
        cols = [rng.normal(0.0, s, ne) for s in (1e-3, 0.05, 0.01, 6.0, 1e6)]
        return cols, rng.uniform(0.0, 2.0, nr), rng.uniform(0.0, 9.0, n_lake)

    cols, riv, lake = draw()
    d_cols, d_riv = [_dev(c) for c in cols], _dev(riv)
    d_lake = _dev(lake) if n_lake else None
    mon = rt.RunMonitors(stream=_stream())
    fn = tmp_path / "syn.cfg.ic.update"
    mon.add_ic(fn, 720, *d_cols, d_riv, d_lake, ne, nr, n_lake)

    def put(cols, riv, lake):
        for d, c in zip(d_cols, cols):
            d.copy_(torch.from_numpy(c))
        d_riv.copy_(torch.from_numpy(riv))
        if n_lake:
            d_lake.copy_(torch.from_numpy(lake))

    assert mon.ic_update(0.0) is True
    mon.flush()
    first = mon_py.ic_file(0.0, *cols, riv, lake)
    assert open(fn, "rb").read() == first
    # not due: nothing queued, the previous file stays
    put(*draw())
    assert mon.ic_update(721.0) is False
    mon.flush()
    assert open(fn, "rb").read() == first and mon.ic_snapshots() == 1
    # due snapshots in a row with the tensors changed in between (both banks, then the first again)
    for t in (720.0, 1440.5, 2160.0):
        cols, riv, lake = draw()
        put(cols, riv, lake)
        assert mon.ic_update(t) is True
    mon.flush()
    assert open(fn, "rb").read() == mon_py.ic_file(2160.0, *cols, riv, lake)
    assert mon.ic_snapshots() == 4
    mon.close()


def test_bad_arguments_and_writer_paths(tmp_path):
    nr = 5
    stage, q = _dev(np.full(nr, 2.0)), _dev(np.zeros(nr))
    mon = rt.RunMonitors(stream=_stream())
    with pytest.raises(rt.ShudRhsError) as e:                  # UpdateICStep 0: the reference divides by it
        mon.add_ic(tmp_path / "a.ic", 0, stage, stage, stage, stage, stage, q, None, nr, nr, 0)
    assert e.value.code == abi.SHUD_ERR_ARG
    with pytest.raises(rt.ShudRhsError) as e:                  # a directory that does not exist
        mon.add_ic(tmp_path / "nodir" / "a.ic", 720, stage, stage, stage, stage, stage, q, None, nr, nr, 0)
    assert e.value.code == abi.SHUD_MON_ERR_IO
    with pytest.raises(rt.ShudRhsError) as e:
        mon.add_flood(tmp_path / "nodir" / "f.csv", stage, q, nr, np.ones(nr), np.ones(nr, dtype=np.int32))
    assert e.value.code == abi.SHUD_MON_ERR_IO
    with pytest.raises(rt.ShudRhsError):                       # nothing was added
        mon.flood(0.0)
    with pytest.raises(rt.ShudRhsError):
        mon.ic_update(0.0)
    # the set still works after the refusals
    mon.add_flood(tmp_path / "f.csv", stage, q, nr, np.ones(nr), np.ones(nr, dtype=np.int32))
    mon.flood(1.0)
    assert mon.flood_rows() == nr
    mon.close()
