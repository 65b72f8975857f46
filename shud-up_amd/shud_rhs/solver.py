"""SHUD()'s time loop on the device (src/Model/shud.cpp:89-131).

`ShudSolver` drives, per solver step, the device ET prelude (updateforcing/tReadForcing + ET(t, tout),
MD_ET.cpp:14-341, include/shud_et.h) and then the device integrator (CVode(mem, tout, y, &t, CV_NORMAL),
include/shud_ode.h) over an RhsHandle.  State, step inputs and the Nordsieck history stay in HBM; only the
per-interval forcing rows (host bookkeeping in the reference too) and the requested outputs cross PCIe.

Control settings are the reference's Model_Control fields (Model_Control.hpp:176-182, .cpp:137,502):
SolverStep = MaxStep, NumSteps = (END - START)/SolverStep, ET sub-stepping when ETStep < SolverStep.
"""
from dataclasses import dataclass

import numpy as np

from . import abi
from .runtime import Checkpoint, OdeSolver, ShudRhsError

ZERO = 1.0e-10                      # Macros.hpp:32


@dataclass
class SolverControl:
    reltol: float = 1.0e-3          # Model_Control.hpp:177 defaults; ccw/heihe/qhh cfg.para use 1e-4
    abstol: float = 1.0e-4
    init_step: float = 1.0e-2
    max_step: float = 30.0
    et_step: float = 60.0
    start: float = 0.0
    min_step: float = 1.0e-6        # SetCVODE (cvode_config.cpp:182)
    max_num_steps: int = 1000000    # SetCVODE (cvode_config.cpp:185)

    @property
    def solver_step(self):          # Model_Control.cpp:502
        return self.max_step

    @property
    def et_substep(self):           # shud.cpp:86-87
        return self.et_step > ZERO and self.et_step + ZERO < self.solver_step


class ShudSolver:
    """handle: RhsHandle with step inputs set (and shud_et_attach'ed when forcing is given).
    forcing(t, tout) -> et.EtForcing for the ET prelude of [t, tout), or None to keep the step inputs."""

    def __init__(self, handle, y0, ctl: SolverControl):
        self.h = handle
        self.ctl = ctl
        self.t = ctl.start
        self.step = 0                   # solver steps taken since ctl.start (a resumed solver continues the count)
        self._ckpt = None
        self._wb = None                 # the WaterBalance a run() was given (a checkpoint is then refused)
        self.ode = OdeSolver(handle, ctl.start, y0, ctl.reltol, ctl.abstol, ctl.init_step, ctl.max_step,
                             ctl.min_step, ctl.max_num_steps)
        self.y = None
        # the handle runs in an internal element order (RhsHandle(order=)): device vectors are carried to the model's
        self._ordered = getattr(handle, "ordered", False)
        self.quad_steps = 0             # monitor steps of run(quad=True)

    @classmethod
    def resume(cls, handle, ctl: SolverControl, path, output=None, monitors=None):
        """A solver that continues from the checkpoint at `path` (include/shud_ckpt.h): handle (with its ET prelude
        attached), output (controls added after Output.resume()) and monitors (after RunMonitors.resume()) are built as
        for a new run and take the file's state; self.t and self.step are the snapshot's.  The forcing callback of the
        continued run() must recompute the terrain-radiation samples of its first interval (SHUD_TSR_RECOMPUTE)."""
        self = cls(handle, np.zeros(handle.num_y), ctl)
        try:
            self.t, self.step = Checkpoint.restore(path, self.ode, rhs=handle, output=output, monitors=monitors)
        except Exception:
            self.close()
            raise
        return self

    def snapshot(self, path, output=None, monitors=None):
        """checkpoint of the run at the current solver-step boundary, after that step's export and monitors; returns
        once the device pass is enqueued (flush_snapshot() waits for the file)"""
        if self._ckpt is None:
            self._ckpt = Checkpoint(stream=self.h.stream())
        # a run that used water-balance diagnostics is refused by the library (SHUD_ERR_UNSUPPORTED)
        self._ckpt.snapshot(path, self.t, self.step, self.ode, rhs=self.h, output=output, monitors=monitors,
                            wb=self._wb)

    def flush_snapshot(self):
        if self._ckpt is not None:
            self._ckpt.flush()

    def run(self, num_steps, forcing=None, on_output=None, output=None, wb=None, quad=False):
        """On an ordered handle (RhsHandle(order=)) y0 and the y of on_output are in the model's numbering; `output`
        controls read the handle's device arrays, which are in the internal one (Output.add(col_src=inv)); wb is
        refused (its basin sums would change order).
        num_steps solver steps (the reference's NumSteps loop); on_output(i, t, y) after each (host copy of y).
        output: runtime.Output whose controls point at the handle's device arrays — after each solver step
        summary(udata) + ExportResults(t) run on the device (shud.cpp:137,153): no host copy of y at all.
        wb: runtime.WaterBalance (needs output) — the reference's SHUD_WB_DIAG hooks (shud.cpp:110-112,137-152):
        onETUpdate after every ET step; after summary the extra, stateful f() on the accepted state, CVodeGetDky(k = 1),
        sample and maybeWrite, then ExportResults.  The extra f() advances the carried state: the trajectory differs
        from a run without wb, as in the reference.
        quad: SHUD_WB_DIAG_QUAD (needs wb, with wb.quad_enable() called) — the reference's CV_ONE_STEP loop
        (shud.cpp:113-135): the stop time is always set, the integrator returns after every internal step, and each
        is followed by a stateful f() on the returned state, its flux arrays and wb.quad_step(t); self.quad_steps
        counts them.  These f() calls advance the carried state too: the trajectory differs from a run with wb
        alone, as in the reference."""
        ctl = self.ctl
        tnext = self.t
        d_y = None
        if wb is not None and output is None:
            raise ValueError("wb needs output (the device-resident loop)")
        if quad and wb is None:
            raise ValueError("quad needs wb")
        ordered = self._ordered
        if ordered and wb is not None:
            raise ValueError("water-balance diagnostics are not available on an ordered handle")
        if wb is not None:
            self._wb = wb
        if output is not None:
            d_y = self._out_y = getattr(self, "_out_y", None) or self.h.device_alloc(8 * self.h.num_y)
        d_du = None
        if wb is not None:
            d_du = self._wb_du = getattr(self, "_wb_du", None) or self.h.device_alloc(8 * self.h.num_y)
        for i in range(num_steps):
            tnext += ctl.solver_step
            while self.t + ZERO < tnext:
                tout = min(self.t + ctl.et_step, tnext) if ctl.et_substep else tnext
                if forcing is not None:
                    f = forcing(self.t, tout)
                    if f is not None:
                        self.h.et_step(f)
                if wb is not None:
                    wb.on_et_update()
                if ctl.et_substep or quad:
                    self.ode.set_stop_time(tout)
                if quad:
                    # shud.cpp:121-129: one internal step at a time; f() on the returned state (stateful, like the
                    # sample's extra f()), its flux arrays, onCvodeMonitorStep(t)
                    while self.t + ZERO < tout:
                        flag, t = self.ode.solve_device(tout, d_y, one_step=True)
                        self._check_flag(flag, t)
                        self.t, self.y = t, None
                        self.h.eval_device(t, d_y, d_du)
                        self.h.refresh_diagnostics()
                        wb.quad_step(t)
                        self.quad_steps += 1
                    continue
                if d_y is not None:
                    flag, t = self.ode.solve_device(tout, d_y)
                    y = None
                else:
                    flag, t, y = self.ode.solve(tout)
                self._check_flag(flag, t)
                self.t, self.y = t, y
            if output is not None:
                # Model_Data::summary(udata) on y(tout); the flux arrays are those of CVODE's last f() call,
                # replayed on its input buffer (the integrator never rewrites that buffer before its next RHS
                # call: the Newton residual's y and the DQ work vector are only written right before an RHS)
                self.h.summary(d_y)
                if wb is not None:
                    self.h.eval_device(self.t, d_y, d_du)
                self.h.refresh_diagnostics()
                if wb is not None:
                    self.ode.get_dky_device(self.t, 1, d_du)
                    wb.sample(self.t, d_du)
                    wb.maybe_write(self.t)
                output.export(self.t)
            self.step += 1
            if on_output is not None:
                if self.y is None:
                    src = d_y
                    if ordered:                # d_y is in the internal numbering
                        src = self._cal_y = getattr(self, "_cal_y", None) or self.h.device_alloc(8 * self.h.num_y)
                        self.h.permute(d_y, src, to="caller")
                    self.y = self.h.d2h(np.empty(self.h.num_y), src)
                on_output(i, self.t, self.y)
        return self.t, self.y

    def _check_flag(self, flag, t):
        if flag < 0:
            if flag == abi.ODE_RHSFUNC_FAIL:
                e = self.h.get_error()
                if e["exit_code"]:
                    raise ShudRhsError(abi.SHUD_ERR_PHYSICS, e["message"], e)
            raise RuntimeError(f"CVode failed with flag {flag} at t={t}")

    def stats(self):
        return self.ode.stats()

    def close(self):
        if self._ckpt is not None:
            self._ckpt.close()
            self._ckpt = None
        self.ode.close()
        for name in ("_out_y", "_wb_du", "_cal_y"):
            if getattr(self, name, None):
                self.h.device_free(getattr(self, name))
                setattr(self, name, None)
