"""GPU: shud_gpu --flood --ic-snapshots end to end on a synthetic project (about 2,000 elements, one day of 60-minute
solver steps, every state output and rivqdown at 60 minutes, Update_IC_STEP 720, element and reach boundary
conditions).

With the output interval equal to the solver step an interval mean is its single sample (buffer = 0 + x, times
tau / 1), so the .dat rows hold the very values the monitors read: stages bit for bit, fluxes as x * 1440.
  .cfg.ic.bak      header time 0, LoadIC's y0 / y_is / y_snow
  .cfg.ic.update   header time 1440, every column equals '%f' of the last .dat row of its array
  .flood.csv       the restatement applied row by row to the rivystage / rivqdown .dat rows: selection, order, ids,
                   stage and bank text exact; discharge text equals '%f' of (x * 1440) / 1440 or of one of its two
                   neighbouring doubles (dividing the scaled value back is within one ulp of x, tighter than a
                   1e-12 relative bound; where it is x itself the whole file is byte-identical)
A run without the flags writes none of the three files and the same .dat bytes; the written restart file loads as
the .cfg.ic of a copy of the project."""
import glob
import os
import shutil

import numpy as np
import pytest

import mon_py
import shud_gpu_run
from shud_rhs import host, shudio, synth

pytestmark = pytest.mark.gpu
MON_FILES = ("syn.flood.csv", "syn.cfg.ic.update", "syn.cfg.ic.bak")


def _run(src, out, *flags):
    return shud_gpu_run.json_line(shud_gpu_run.run([*flags, "-o", out, "-C", src, src, "syn"]))


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("monhost")
    src = tmp / "in"
    synth.write_project(str(src), "syn", 2000, days=1.0, max_step=60.0, et_step=60.0, dt_out=60, bc=True,
                        extra_para={"Update_IC_STEP": 720, "dt_ye_ic": 60})
    # Raised initial stages drain below the banks well within the first 60-minute step (measured: no row), so the
    # flood comes from the project's two head-boundary reaches: their .tsd.rbc1 head is set 0.3 m above the lower of
    # their two banks, so that reach has a row at every step (a higher head floods more reaches but makes the day
    # several times as expensive to integrate).  The element head boundaries that bc=True adds make .cfg.ic.bak
    # differ from the pre-loop summary arrays.
    P = host.Project(str(src), "syn", cwd=str(src))
    m = P.model()
    P.close()
    head = m.riv["riv_depth"][m.riv_bc > 0].min() + 0.3
    ln = open(src / "syn.tsd.rbc1").read().split("\n")
    rows = [r.split("\t")[0] + "\t%.17g" % head for r in ln[2:] if r]
    open(src / "syn.tsd.rbc1", "w").write("\n".join(ln[:2] + rows) + "\n")
    res_on = _run(src, tmp / "out_on", "--flood", "--ic-snapshots")
    res_off = _run(src, tmp / "out_off")
    return {"src": src, "on": tmp / "out_on", "off": tmp / "out_off", "res_on": res_on, "res_off": res_off,
            "tmp": tmp}


def _last(out, sfx):
    d = shudio.read_dat(str(out / f"syn.{sfx}.dat"))
    assert d["t"].size == 24
    return d


def test_ic_bak_is_the_loaded_initial_condition(runs):
    P = host.Project(str(runs["src"]), "syn", cwd=str(runs["src"]))
    ne, nr = P.model().num_ele, P.model().num_riv
    y0, y_is, y_snow = P.array("y0"), P.array("y_is"), P.array("y_snow")
    P.close()
    ref = mon_py.ic_file(0, y_is, y_snow, y0[:ne], y0[ne:2 * ne], y0[2 * ne:3 * ne], y0[3 * ne:3 * ne + nr])
    assert open(runs["on"] / "syn.cfg.ic.bak", "rb").read() == ref
    assert ref.startswith(b"%d\t 6 \t0.000000\n" % ne)


def test_final_ic_update_equals_last_dat_rows(runs):
    t, ele, riv, lake = mon_py.parse_ic(runs["on"] / "syn.cfg.ic.update")
    assert t == 1440.0 and lake is None
    for k, sfx in enumerate(("eleyic", "eleysnow", "eleysurf", "eleyunsat", "eleygw")):
        last = _last(runs["on"], sfx)["data"][-1]
        assert [r[k] for r in ele] == ["%f" % v for v in last], sfx
    assert riv == ["%f" % v for v in _last(runs["on"], "rivystage")["data"][-1]]
    assert runs["res_on"]["ic_snapshots"] == 3                 # t = 0 (LoadIC's values), 720 and the final 1440
    assert not os.path.exists(runs["on"] / "syn.cfg.ic.update.tmp")


def test_flood_csv_equals_restatement_on_dat_rows(runs):
    P = host.Project(str(runs["src"]), "syn", cwd=str(runs["src"]))
    depth, rtype = P.model().riv["riv_depth"], P.riv_type()
    P.close()
    stg, qd = _last(runs["on"], "rivystage"), _last(runs["on"], "rivqdown")
    got = open(runs["on"] / "syn.flood.csv", "rb").read()
    calls = [(stg["t"][k] + 60.0, stg["data"][k], qd["data"][k] / 1440.0) for k in range(24)]
    ref, total, _ = mon_py.flood_file(calls, depth, rtype)
    assert total >= 1, "no reach above its bank: the test exercises no row"
    assert runs["res_on"]["flood_rows"] == total
    if got == ref:
        return
    g, r = got.split(b"\n"), ref.split(b"\n")
    assert len(g) == len(r) and g[0] == r[0]
    k = 1
    for t, s, q in calls:
        for i in np.nonzero(s > depth)[0]:
            gf, rf = g[k].split(b"\t"), r[k].split(b"\t")
            assert gf[:5] == rf[:5], (k, g[k], r[k])
            near = {("%f" % v).encode() for v in (q[i], np.nextafter(q[i], -np.inf), np.nextafter(q[i], np.inf))}
            assert gf[5] in near, (k, g[k], r[k])
            k += 1


def test_run_without_flags_writes_no_monitor_file_and_the_same_dat(runs):
    for f in MON_FILES:
        assert os.path.exists(runs["on"] / f), f
        assert not os.path.exists(runs["off"] / f), f
    for key in ("flood_rows", "ic_snapshots", "monitors_writer_s"):
        assert key in runs["res_on"] and key not in runs["res_off"]
    assert "monitors" in runs["res_on"]["loop_phases_s"] and "monitors" not in runs["res_off"]["loop_phases_s"]
    files = sorted(os.path.basename(f) for f in glob.glob(str(runs["on"] / "*.dat")))
    assert len(files) == 25 and files == sorted(os.path.basename(f) for f in glob.glob(str(runs["off"] / "*.dat")))
    for f in files:
        assert open(runs["on"] / f, "rb").read() == open(runs["off"] / f, "rb").read(), f


def test_written_update_loads_as_cfg_ic(runs):
    d = runs["tmp"] / "restart"
    shutil.copytree(runs["src"], d)
    shutil.copyfile(runs["on"] / "syn.cfg.ic.update", d / "syn.cfg.ic")
    P = host.Project(str(d), "syn", cwd=str(d))
    ne = P.model().num_ele
    _, ele, riv, _ = mon_py.parse_ic(d / "syn.cfg.ic")
    y0 = P.array("y0")
    rb = mon_py.read_back                                       # the reader's strtold-then-double rule
    for k, got in ((2, y0[:ne]), (3, y0[ne:2 * ne]), (4, y0[2 * ne:3 * ne]), (0, P.array("y_is")), (1, P.array("y_snow"))):
        assert np.array_equal(got, np.array([rb(r[k]) for r in ele])), k
    assert np.array_equal(y0[3 * ne:3 * ne + len(riv)], np.array([rb(v) for v in riv]))
    P.close()
