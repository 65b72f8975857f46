"""The set-up in front of SHUD()'s time loop (src/Model/shud.cpp:32-85), written once in Python: the counterpart of
host/shud_gpu.cpp's stages, under the same names, so the two drivers read side by side.  Each stage is a plain
function over a host.Project and an RhsHandle; `ProjectRun` strings them together and hands ShudSolver.run() what they
built.  The loop itself is solver.ShudSolver.run().  Not restated here (shud_gpu only): the restart-snapshot schedule
inside the loop and .cfg.ic.bak.
"""
import os

import numpy as np

from . import abi, host
from . import runtime as rt
from .solver import ShudSolver, SolverControl

LONLAT = {0: "FORCING_FIRST", 1: "FORCING_MEAN", 2: "FIXED"}        # Control_Data::solar_lonlat_mode
# the SHUD_ARR_* arrays indexed by reach or by lake (every other one is per element)
ARR_NOT_ELE = frozenset({abi.SHUD_ARR_Y_RIV_STG, abi.SHUD_ARR_Y_LAKE_STG, abi.SHUD_ARR_QRIV_DOWN, abi.SHUD_ARR_QRIV_UP,
                         abi.SHUD_ARR_QRIV_SURF, abi.SHUD_ARR_QRIV_SUB, abi.SHUD_ARR_LAKE_TOPAREA,
                         abi.SHUD_ARR_Q_LAKE_EVAP, abi.SHUD_ARR_Q_LAKE_PRCP, abi.SHUD_ARR_Q_LAKE_RIVIN,
                         abi.SHUD_ARR_Q_LAKE_RIVOUT, abi.SHUD_ARR_Q_LAKE_SURF, abi.SHUD_ARR_Q_LAKE_SUB})


def header_kw(c):
    """the header fields every .dat file carries, from Project.control()"""
    return dict(radiation_input_mode=c["radiation_input_mode"], terrain_radiation=c["terrain_radiation"],
                solar_lonlat_mode=LONLAT[c["solar_lonlat_mode"]], lon=c["solar_lon_deg"], lat=c["solar_lat_deg"])


def solver_control(c, **overrides):
    """SetCVODE's settings (cvode_config.cpp:149-197) from Project.control()"""
    kw = dict(reltol=c["reltol"], abstol=c["abstol"], init_step=c["init_step"], max_step=c["max_step"],
              et_step=c["et_step"], start=c["start_time"])
    return SolverControl(**{**kw, **overrides})


def _sizes(m):
    return m.num_ele, m.num_riv, getattr(m, "num_lake", 0) or 0


def device_model(P, mode=abi.SHUD_MODE_SERIAL, order=None, tweak=None, model=None, **handle_kw):
    """the device side -> (m, h): the RHS handle over P.model() (or `model`; tweak(m) may edit it first) with the ET
    prelude attached, LoadIC's interception and snow storages, and the carried u_satn of the first updateforcing:
    f_update's globals are freshly allocated (zero) before the first f() call"""
    m = P.model() if model is None else model
    if tweak:
        tweak(m)
    h = rt.RhsHandle(m, mode=mode, order=order, **handle_kw)
    try:
        h.et_attach(P.et_model())
        h.et_set_state(P.array("y_is"), P.array("y_snow"))
        h.set_step_inputs(step={"u_satn": np.zeros(m.num_ele)})
    except Exception:
        h.close()
        raise
    return m, h


def sink_kind(n_all, ne, nr, nl, output_mode):
    """setSink (MD_initialize.cpp:348-356) -> "ele" | "riv" | "lake" | None: by NumAll, elements first, then reaches
    if there are any, then lakes if there are any; OUTPUT_MODE LEGACY (0) has no NetCDF sink"""
    if not output_mode:
        return None
    if n_all == ne:
        return "ele"
    if nr > 0 and n_all == nr:
        return "riv"
    if nl > 0 and n_all == nl:
        return "lake"
    return None


def add_outputs(P, h, out, outdir, c=None, ncc=None, history=None, override=None):
    """initialize_output (MD_initialize.cpp:246-371) with device sources -> the registered declarations.  Attaches the
    NetCDF files when OUTPUT_MODE is not LEGACY (history: their whole `history` attribute), then registers every print
    control of P.outputs(outdir).  override(k, d) -> keyword changes for control k (interval and Output.add's), or
    None to leave that control out."""
    c = P.control() if c is None else c
    ncc = P.ncoutput() if ncc is None else ncc
    mode = ncc["output_mode"]
    ne, nr, nl = _sizes(h.model)
    if mode:                                                 # NetcdfOutputContext (MD_initialize.cpp:346-347)
        for kind, n in (("ele", ne), ("riv", nr), ("lake", nl)):
            if kind == "ele" or n > 0:
                out.attach_nc(kind, n, c["forc_start_time"], out_dir=ncc["out_dir"] or None, history=history,
                              crs_wkt=ncc["crs_wkt"] or None, mesh=P.mesh_nodes() if kind == "ele" else None)
    # an ordered handle's element arrays are in the internal numbering: column c reads element inv[c]
    inv = h.order()[2] if h.ordered else None
    decl = []
    for k, d in enumerate(P.outputs(outdir)):
        p, _ = h.device_array(d["array"])
        if not p:
            raise ValueError(f"no device source for {d['basename']}")
        if d["column"] >= 0:
            p += 8 * d["column"] * ne
        mapped = inv is not None and d["array"] not in ARR_NOT_ELE
        if mapped and d["n_all"] != ne:
            raise ValueError(f"element output {d['basename']} has {d['n_all']} columns, mesh {ne} elements")
        kw = dict(interval=d["interval"], binary=bool(c["binary"]) and mode != 1, ascii=bool(c["ascii"]) and mode != 1,
                  col_src=inv if mapped else None, nc=sink_kind(d["n_all"], ne, nr, nl, mode), legacy=mode != 1)
        if override:
            change = override(k, d)
            if change is None:
                continue
            kw.update(change)
        out.add(d["basename"], p, d["n_all"], kw.pop("interval"), d["iflux"], start_time=c["forc_start_time"],
                flag_io=d["flag_io"], **header_kw(c), **kw)
        decl.append(d)
    if mode:                                                 # headers and fixed variables before the time loop
        out.nc_begin()
    return decl


def add_zonal_outputs(P, h, out, outdir, zones, c=None, ncc=None, override=None):
    """the zonal twins (shud_gpu --zones): every element control of P.outputs(outdir) (NumEle columns of a per-element
    array) also gets <outdir>/<prj>.zone.<leaf> with the same interval, iflux and binary / ascii settings, one column
    per zone.  A leaf that begins with "eleq" (m3/day) is the zone's sum; every other one (eley*, elev*, rn_*) the mean
    weighted by element area.  zones: a table's path (Project.zones) or NumEle ids in the file's numbering (0: in no
    zone); on an ordered handle they go through the same inverse permutation as the element controls.  The twins cover
    every element whatever io_ele masks, and are legacy files only: refused under OUTPUT_MODE NETCDF.
    override(k, d): add_outputs' (None leaves the twin out too; only interval, binary and ascii are taken).
    -> the registered twins' basenames"""
    c = P.control() if c is None else c
    ncc = P.ncoutput() if ncc is None else ncc
    if ncc["output_mode"] == 1:
        raise ValueError("zonal outputs are legacy files (.dat / .csv): not with OUTPUT_MODE NETCDF")
    ne = _sizes(h.model)[0]
    zone = P.zones(zones)[0] if isinstance(zones, (str, os.PathLike)) else np.asarray(zones)
    if zone.shape != (ne,):
        raise ValueError(f"zones: {zone.shape} ids, mesh {ne} elements")
    nz = int(zone.max(initial=0))
    area = np.asarray(h.model.ele["area"], dtype=np.float64)
    inv = h.order()[2] if h.ordered else None
    names = []
    for k, d in enumerate(P.outputs(outdir)):
        if d["array"] in ARR_NOT_ELE or d["n_all"] != ne:
            continue
        kw = dict(interval=d["interval"], binary=bool(c["binary"]), ascii=bool(c["ascii"]))
        if override:
            change = override(k, d)
            if change is None:
                continue
            kw.update({key: v for key, v in change.items() if key in kw})
        p, _ = h.device_array(d["array"])
        if not p:
            raise ValueError(f"no device source for {d['basename']}")
        if d["column"] >= 0:
            p += 8 * d["column"] * ne
        head, leaf = d["basename"].rsplit(".", 1)
        total = leaf.startswith("eleq")
        out.add_zonal(f"{head}.zone.{leaf}", p, ne, kw.pop("interval"), d["iflux"], zone, n_zone=nz,
                      weight=None if total else area, op="sum" if total else "mean", col_src=inv,
                      start_time=c["forc_start_time"], **header_kw(c), **kw)
        names.append(f"{head}.zone.{leaf}")
    return names


def water_balance(P, h, outdir, prj, trapz=False, quad=False, c=None):
    """WaterBalanceDiag::enable (shud.cpp:70-75), after the pre-loop summary; quad: SHUD_WB_DIAG_QUAD's monitor"""
    c = P.control() if c is None else c
    wb = rt.WaterBalance(h, P.wb_interval(), start_time=c["start_time"], trapz=trapz,
                         prefix=os.path.join(str(outdir), prj), forc_start_time=c["forc_start_time"], **header_kw(c))
    if quad:
        try:
            wb.quad_enable()
        except Exception:
            wb.close()
            raise
    return wb


def monitors(P, h, outdir, prj, flood=False, ic=False, resume=False):
    """InitFloodAlert and PrintInit's registration (shud.cpp:76-77) -> RunMonitors.  ic: <prj>.cfg.ic.update every
    Update_IC_STEP minutes from the handle's arrays (in the file's numbering on an ordered handle).  flood: True, or
    a dict replacing some of path (<outdir>/<prj>.flood.csv), riv_depth (the banks) and riv_type (arrays or scalars)."""
    m = h.model
    ne, nr, nl = _sizes(m)
    arr = lambda a: h.device_array(a)[0]                                       # noqa: E731
    mon = rt.RunMonitors(stream=h.stream())
    try:
        if resume:
            mon.resume()
        if ic:
            mon.add_ic(os.path.join(str(outdir), f"{prj}.cfg.ic.update"), P.update_ic_step(),
                       arr(abi.SHUD_ARR_Y_ELE_IS), arr(abi.SHUD_ARR_Y_ELE_SNOW), arr(abi.SHUD_ARR_Y_ELE_SURF),
                       arr(abi.SHUD_ARR_Y_ELE_UNSAT), arr(abi.SHUD_ARR_Y_ELE_GW), arr(abi.SHUD_ARR_Y_RIV_STG),
                       arr(abi.SHUD_ARR_Y_LAKE_STG) if nl else None, ne, nr, nl)
            if h.ordered:
                mon.set_ic_order(h.order()[1])
        if flood:
            f = {"path": os.path.join(str(outdir), f"{prj}.flood.csv"), "riv_depth": m.riv["riv_depth"],
                 "riv_type": None, **({} if flood is True else flood)}
            rtype = P.riv_type() if f["riv_type"] is None else f["riv_type"]
            mon.add_flood(f["path"], arr(abi.SHUD_ARR_Y_RIV_STG), arr(abi.SHUD_ARR_QRIV_DOWN), nr,
                          np.broadcast_to(f["riv_depth"], nr), np.broadcast_to(rtype, nr))
    except Exception:
        mon.close()
        raise
    return mon


def forcing_callback(P, h):
    """ShudSolver.run's forcing(t, tout): the forcing rows, then the BC rows (tsd_eyBC .. tsd_rqBC of f_update) when the
    project has any; the ET step follows in run()"""
    def forcing(t, tout):
        f = P.forcing(t, tout)
        bc = P.bc_rows()
        if bc:
            h.set_step_inputs(step={}, bc_tables=bc)
        return f
    return forcing


class ProjectRun:
    """shud_gpu's run in Python: the stages above in shud_gpu's order, then start() or restore(path), run(), close().
    control: SolverControl overrides; override, history: add_outputs'; wb / trapz / quad: SHUD_WB_DIAG,
    SHUD_WB_DIAG_TRAPZ, SHUD_WB_DIAG_QUAD; flood, ic: monitors' (flood(t) then runs after every solver step's export);
    resume: the outputs and monitors keep the files of an earlier run, for restore(); zones: add_zonal_outputs' (a
    table's path or NumEle ids): the zonal twins of the element controls, registered after them."""

    def __init__(self, indir, prj, outdir, cwd=None, end_day=-1.0, mode=abi.SHUD_MODE_SERIAL, order=None, tweak=None,
                 control=None, history=None, override=None, wb=False, trapz=False, quad=False, flood=False, ic=False,
                 resume=False, zones=None):
        self.prj, self.outdir, self.quad, self.flood = prj, str(outdir), quad, bool(flood)
        self.P = self.h = self.out = self.wb = self.mon = self.sv = None
        try:
            self.P = P = host.Project(str(indir), prj, cwd=None if cwd is None else str(cwd), end_day=end_day)
            self.c = c = P.control()
            self.ctl = solver_control(c, **(control or {}))
            self.m, self.h = device_model(P, mode=mode, order=order, tweak=tweak)
            os.makedirs(self.outdir, exist_ok=True)
            self.h.prepare_outputs()
            self._summary(P.array("y0"))
            self.out = rt.Output(stream=self.h.stream())
            if resume:
                self.out.resume()
            self.decl = add_outputs(P, self.h, self.out, self.outdir, c=c, history=history, override=override)
            self.zonal = [] if zones is None else add_zonal_outputs(P, self.h, self.out, self.outdir, zones, c=c,
                                                                    override=override)
            if wb:
                self.wb = water_balance(P, self.h, self.outdir, prj, trapz=trapz, quad=quad, c=c)
            if flood or ic:
                self.mon = monitors(P, self.h, self.outdir, prj, flood=flood, ic=ic, resume=resume)
            self.forcing = forcing_callback(P, self.h)
        except Exception:
            self.close()
            raise

    def _summary(self, y0):
        """Model_Data::summary on the initial state (shud_gpu does it before registering the outputs): the arrays the
        water balance and the monitors read before the first step"""
        h = self.h
        bufs = [h.device_alloc(8 * h.num_y) for _ in range(2 if h.ordered else 1)]
        try:
            h.h2d(bufs[0], y0)
            if h.ordered:
                h.permute(bufs[0], bufs[1], to="internal")
            h.summary(bufs[-1])
            h.synchronize()
        finally:
            for p in bufs:
                h.device_free(p)

    def start(self, y0=None):
        self.sv = ShudSolver(self.h, self.P.array("y0") if y0 is None else y0, self.ctl)
        return self

    def restore(self, path):
        self.sv = ShudSolver.resume(self.h, self.ctl, path, output=self.out, monitors=self.mon)
        return self

    def run(self, num_steps=None, on_output=None):
        """num_steps solver steps (default: the project's NumSteps) -> (t, y) of ShudSolver.run"""
        cb = on_output
        if self.flood:                                       # MD->flood->FloodWarning(t), after ExportResults
            def cb(i, t, y):
                self.mon.flood(t)
                if on_output is not None:
                    on_output(i, t, y)
        return self.sv.run(self.c["num_steps"] if num_steps is None else num_steps, forcing=self.forcing,
                           on_output=cb, output=self.out, wb=self.wb, quad=self.quad)

    def close(self):
        for name in ("out", "mon", "wb", "sv", "h", "P"):
            x = getattr(self, name)
            setattr(self, name, None)
            if x is not None:
                x.close()
