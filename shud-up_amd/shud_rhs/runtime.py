"""ctypes front end of libshud_rhs.so — the product path.  Fails loudly if the HIP library is absent.

`RhsHandle` mirrors the reference call sequence: construct once from a ShudModel (Model_Data after
initialize(), MD_initialize.cpp:168-245), `set_step_inputs` once per ET step (updateforcing()/ET(),
MD_ET.cpp:14-342), then `eval(t, y)` per CVODE RHS call (f(), src/Model/f.cpp:2-32).
"""
import ctypes as C
import os

import numpy as np

from . import abi

_LIB = None
LIB_PATH = os.environ.get("SHUD_RHS_LIB") or os.path.join(
    os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libshud_rhs.so")   # env: A/B builds only


class ShudRhsError(RuntimeError):
    def __init__(self, code, msg, err=None):
        super().__init__(f"shud_rhs error {code}: {msg}")
        self.code = code
        self.err = err


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"HIP library {LIB_PATH} not built: run `make -C shud-up_amd` "
                              "or __graft_entry__.build() (there is no CPU fallback)")
        _LIB = abi.bind(C.CDLL(LIB_PATH))
    return _LIB


def _check(rc, what):
    if rc != abi.SHUD_OK:
        raise ShudRhsError(rc, f"{what}: {lib().shud_rhs_last_error_string().decode(errors='replace')}")


class RhsHandle:
    def __init__(self, model, mode=abi.SHUD_MODE_SERIAL, device=0, stream=None, check_errors=True,
                 partition=None, order=None):
        """order (include/shud_order.h): None = a plain handle; "identity", "bfs", "tiles" or a permutation array (new
        element k is old order[k]) = shud_rhs_create_ordered.  Host arrays stay in the model's numbering, device
        pointers are in the internal one (permute())."""
        self.model = model
        self.ordered = False
        self._mesh = model.mesh_struct()
        self._par = model.params_struct()
        opt = abi.ShudRhsOptions(mode, device, stream, 1 if check_errors else 0)
        h = C.c_void_p()
        if order is not None:
            if partition is not None:
                raise ValueError("order= is not available on partitioned handles")
            kind, up = order_kind(order, model.num_ele)
            _check(lib().shud_rhs_create_ordered(C.byref(self._mesh), C.byref(self._par), C.byref(opt), kind,
                                                 None if up is None else up.ctypes.data_as(abi.c_int32_p),
                                                 C.byref(h)), "shud_rhs_create_ordered")
            self.n_own, self.n_own_riv = model.num_ele, model.num_riv
            self.n_lake = getattr(model, "num_lake", 0)
            self.h = h
            perm = self.order()[1]
            self.ordered = bool((perm != np.arange(perm.size)).any())    # device pointers are in another numbering
        elif partition is None:
            _check(lib().shud_rhs_create(C.byref(self._mesh), C.byref(self._par), C.byref(opt), C.byref(h)),
                   "shud_rhs_create")
            self.n_own, self.n_own_riv = model.num_ele, model.num_riv
            self.n_lake = getattr(model, "num_lake", 0)
        else:
            self._part = partition.struct()
            _check(lib().shud_rhs_create_partitioned(C.byref(self._mesh), C.byref(self._par), C.byref(opt),
                                                     C.byref(self._part), C.byref(h)),
                   "shud_rhs_create_partitioned")
            self.n_own, self.n_own_riv = partition.n_own_ele, partition.n_own_riv
            self.n_lake = getattr(model, "num_lake", 0)   # the local mesh carries the owned lakes
        self.h = h
        self.mode = mode

    @property
    def num_y(self):
        return 3 * self.n_own + self.n_own_riv + self.n_lake

    def close(self):
        if self.h:
            lib().shud_rhs_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_step_inputs(self, step=None, bc_tables=None):
        s = self.model.step_struct(step, bc_tables)
        _check(lib().shud_rhs_set_step_inputs(self.h, C.byref(s)), "shud_rhs_set_step_inputs")

    def eval(self, t, y, ydot=None, raise_on_physics=True):
        """Host-array RHS: returns ydot (numpy).  Raises ShudRhsError on a physics error (the reference
        would have exited; the error details are in .err)."""
        y = np.ascontiguousarray(y, dtype=np.float64)
        if y.size != self.num_y:
            raise ValueError(f"y has {y.size} entries, expected {self.num_y}")
        if ydot is None:
            ydot = np.empty_like(y)
        rc = lib().shud_rhs_eval(self.h, float(t), y.ctypes.data, ydot.ctypes.data, abi.SHUD_WHERE_HOST)
        if rc == abi.SHUD_ERR_PHYSICS and raise_on_physics:
            e = self.get_error()
            raise ShudRhsError(rc, e["message"], e)
        if rc not in (abi.SHUD_OK, abi.SHUD_ERR_PHYSICS):
            _check(rc, "shud_rhs_eval")
        return ydot

    def eval_device(self, t, d_y, d_ydot):
        """Stream-ordered eval on device pointers (ints)."""
        _check(lib().shud_rhs_eval(self.h, float(t), C.c_void_p(d_y), C.c_void_p(d_ydot), abi.SHUD_WHERE_DEVICE),
               "shud_rhs_eval(device)")

    def get_error(self):
        e = abi.ShudErr()
        _check(lib().shud_rhs_get_error(self.h, C.byref(e)), "shud_rhs_get_error")
        return {"flags": e.flags, "exit_code": e.exit_code, "first_index": list(e.first_index),
                "n_aet_warn": e.n_aet_warn, "message": e.message.decode(errors="replace")}

    def clear_error(self):
        _check(lib().shud_rhs_clear_error(self.h), "shud_rhs_clear_error")

    def num_calls(self):
        return lib().shud_rhs_num_calls(self.h)

    def layout(self):
        pk, nc, ns = C.c_int(), C.c_int(), C.c_int()
        _check(lib().shud_rhs_layout(self.h, C.byref(pk), C.byref(nc)), "shud_rhs_layout")
        _check(lib().shud_rhs_layout_streamed(self.h, C.byref(ns)), "shud_rhs_layout_streamed")
        sh = C.c_int()
        if hasattr(lib(), "shud_rhs_layout_shared"):     # (A/B builds of older sources lack it)
            _check(lib().shud_rhs_layout_shared(self.h, C.byref(sh)), "shud_rhs_layout_shared")
        out = {"packed": bool(pk.value), "n_classes": nc.value}
        if ns.value:
            out["streamed_fields"] = ns.value
        if sh.value:
            out["shared_edges"] = sh.value
        return out

    def order(self):
        """(kind, perm, inv): abi.SHUD_ORDER_*, perm[internal] = model index, inv[model index] = internal"""
        kind = C.c_int()
        perm, inv = (np.zeros(self.model.num_ele, dtype=np.int32) for _ in range(2))
        _check(lib().shud_rhs_order(self.h, C.byref(kind), perm.ctypes.data_as(abi.c_int32_p),
                                    inv.ctypes.data_as(abi.c_int32_p)), "shud_rhs_order")
        return kind.value, perm, inv

    def permute(self, d_src, d_dst, to="internal", what="state"):
        """stream-ordered device copy between the numberings (shud_rhs_permute): to = "internal" | "caller";
        what = "state" ([sf|us|gw|riv]), "ele" ([NE]) or "ele3" ([3*NE] edge-major)"""
        d = {"internal": abi.SHUD_PERM_TO_INTERNAL, "caller": abi.SHUD_PERM_TO_CALLER}[to]
        w = {"state": abi.SHUD_PERM_STATE, "ele": abi.SHUD_PERM_ELE, "ele3": abi.SHUD_PERM_ELE3}[what]
        _check(lib().shud_rhs_permute(self.h, d, w, C.c_void_p(d_src), C.c_void_p(d_dst)), "shud_rhs_permute")

    def diagnostics(self):
        m = self.model
        NE, NR, NS = m.num_ele, m.num_riv, m.num_seg
        out = {}
        o = abi.ShudFluxOut()
        for name in abi.FLUXOUT_ORDER:
            n = (3 * NE if name in abi.DIAG_ELE3 else NS if name in abi.DIAG_SEG else NR if name in abi.DIAG_RIV
                 else getattr(m, "num_lake", 0) if name in abi.DIAG_LAKE else NE)
            out[name] = np.zeros(n)
            setattr(o, name, out[name].ctypes.data_as(abi.c_double_p))
        _check(lib().shud_rhs_sync_diagnostics(self.h, C.byref(o)), "shud_rhs_sync_diagnostics")
        return out

    # ---- device memory helpers (bench / tests without torch) ----
    def device_alloc(self, nbytes):
        p = C.c_void_p()
        _check(lib().shud_rhs_device_alloc(self.h, nbytes, C.byref(p)), "device_alloc")
        return p.value

    def device_free(self, p):
        _check(lib().shud_rhs_device_free(self.h, C.c_void_p(p)), "device_free")

    def h2d(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(lib().shud_rhs_memcpy(self.h, C.c_void_p(dptr), arr.ctypes.data, arr.nbytes, 1), "memcpy H2D")

    def d2h(self, arr, dptr):
        _check(lib().shud_rhs_memcpy(self.h, arr.ctypes.data, C.c_void_p(dptr), arr.nbytes, 2), "memcpy D2H")
        return arr

    def synchronize(self):
        _check(lib().shud_rhs_synchronize(self.h), "synchronize")

    def stream(self):
        return lib().shud_rhs_stream(self.h)

    def time_kernels(self, t, d_y, d_ydot, reps):
        ms_eval = C.c_double()
        ms = (C.c_double * 8)()
        nk = C.c_int(8)
        names = C.create_string_buffer(256)
        _check(lib().shud_rhs_time_kernels(self.h, float(t), C.c_void_p(d_y), C.c_void_p(d_ydot), int(reps),
                                           C.byref(ms_eval), ms, C.byref(nk), names, 256), "time_kernels")
        nm = names.value.decode().split(",")
        return ms_eval.value, {nm[k]: ms[k] for k in range(nk.value)}

    def timing(self, max_evals, stride=1):
        """record per-kernel HIP events in every `stride`-th of the next evals, up to `max_evals` of them
        (shud_rhs_timing)"""
        _check(lib().shud_rhs_timing(self.h, int(max_evals), int(stride)), "timing")

    def timing_read(self):
        """(ms_ele, ms_riv, ms_eval, n): per-eval averages of the evals recorded since timing()"""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        _check(lib().shud_rhs_timing_read(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)), "timing_read")
        return a.value, b.value, c.value, n.value

    # ---- output path (include/shud_out.h) ----
    def summary(self, d_y):
        """Model_Data::summary(udata) on the device: SHUD_ARR_Y_* from the state at d_y"""
        _check(lib().shud_rhs_summary(self.h, C.c_void_p(d_y)), "summary")

    def refresh_diagnostics(self):
        """the last RHS evaluation replayed with diagnostic stores into the device arrays (no host copy)"""
        _check(lib().shud_rhs_refresh_diagnostics(self.h), "refresh_diagnostics")

    def prepare_outputs(self):
        """allocate every device output array (zeros) without evaluating anything (shud_rhs_prepare_outputs)"""
        _check(lib().shud_rhs_prepare_outputs(self.h), "prepare_outputs")

    def device_array(self, which):
        n = C.c_int64()
        p = lib().shud_rhs_device_array(self.h, int(which), C.byref(n))
        return p, n.value

    # ---- external-transport partition hooks ----
    def halo_buffers(self):
        p = [C.c_void_p() for _ in range(4)]
        _check(lib().shud_rhs_halo_buffers(self.h, *[C.byref(x) for x in p]), "halo_buffers")
        return [x.value for x in p]

    # ---- ET-step prelude (include/shud_et.h) ----
    def et_attach(self, etm):
        self._et_mesh = etm.mesh_struct()
        self._et_par = etm.params_struct()
        _check(lib().shud_et_attach(self.h, C.byref(self._et_mesh), C.byref(self._et_par)), "shud_et_attach")

    def et_set_state(self, y_is=None, y_snow=None):
        a = None if y_is is None else np.ascontiguousarray(y_is, dtype=np.float64)
        b = None if y_snow is None else np.ascontiguousarray(y_snow, dtype=np.float64)
        _check(lib().shud_et_set_state(self.h, None if a is None else a.ctypes.data,
                                       None if b is None else b.ctypes.data), "shud_et_set_state")

    def et_step(self, forcing, raise_on_physics=True):
        fs = forcing.struct()
        rc = lib().shud_et_step(self.h, C.byref(fs))
        if rc == abi.SHUD_ERR_PHYSICS and raise_on_physics:
            e = self.get_error()
            raise ShudRhsError(rc, e["message"], e)
        if rc not in (abi.SHUD_OK, abi.SHUD_ERR_PHYSICS):
            _check(rc, "shud_et_step")
        return rc

    def et_get(self):
        from .et import out_struct
        o, arrs = out_struct(self.model.num_ele)
        _check(lib().shud_et_get(self.h, C.byref(o)), "shud_et_get")
        return arrs

    def eval_pack(self, d_y):
        _check(lib().shud_rhs_eval_pack(self.h, C.c_void_p(d_y)), "eval_pack")

    def eval_compute(self, t, d_y, d_ydot):
        _check(lib().shud_rhs_eval_compute(self.h, float(t), C.c_void_p(d_y), C.c_void_p(d_ydot)), "eval_compute")

    def debug_halo(self, spin_us=0.0, d_ele_src=None, d_riv_src=None, publish=True, timeout_ms=0.0):
        """test hook (shud_rhs_debug_halo): late / kernel-written / missing halo on the comm stream"""
        _check(lib().shud_rhs_debug_halo(self.h, float(spin_us), C.c_void_p(d_ele_src), C.c_void_p(d_riv_src),
                                         1 if publish else 0, float(timeout_ms)), "debug_halo")


def order_kind(order, num_ele):
    """(SHUD_ORDER_*, user permutation or None) of an order= argument: "identity", "bfs", "tiles" or a permutation
    array"""
    if isinstance(order, str):
        try:
            return {"identity": abi.SHUD_ORDER_IDENTITY, "bfs": abi.SHUD_ORDER_BFS,
                    "tiles": abi.SHUD_ORDER_TILES}[order], None
        except KeyError:
            raise ValueError(f"unknown order {order!r}") from None
    up = np.ascontiguousarray(order, dtype=np.int32)
    if up.shape != (num_ele,):
        raise ValueError(f"order has shape {up.shape}, expected ({num_ele},)")
    return abi.SHUD_ORDER_USER, up


def order_plan(model, order):
    """perm [NE] (new element k is old perm[k]) that shud_rhs_create_ordered would use (shud_order_plan; no device)"""
    kind, up = order_kind(order, model.num_ele)
    mesh = model.mesh_struct()
    perm = np.zeros(model.num_ele, dtype=np.int32)
    _check(lib().shud_order_plan(C.byref(mesh), kind, None if up is None else up.ctypes.data_as(abi.c_int32_p),
                                 perm.ctypes.data_as(abi.c_int32_p)), "shud_order_plan")
    return perm


def order_gather(perm, a, planes=1):
    """a per-element host array carried into the numbering of perm (shud_order_gather_host)"""
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    a = np.ascontiguousarray(a)
    out = np.empty_like(a)
    assert a.size == planes * perm.size
    _check(lib().shud_order_gather_host(perm.ctypes.data_as(abi.c_int32_p), perm.size, a.itemsize, int(planes),
                                        a.ctypes.data, out.ctypes.data), "shud_order_gather_host")
    return out


def order_apply(model, perm):
    """the model under perm (shud_order_apply: mesh and parameters; the step arrays through shud_order_gather_host),
    as a new ShudModel that owns its arrays.  Lake models raise (SHUD_ERR_UNSUPPORTED)."""
    import copy

    from .model import ELE1, ELE3
    perm = np.ascontiguousarray(perm, dtype=np.int32)
    mesh, par = model.mesh_struct(), model.params_struct()
    mo, po, st = abi.ShudMeshSoA(), abi.ShudParamsSoA(), C.c_void_p()
    _check(lib().shud_order_apply(C.byref(mesh), C.byref(par), perm.ctypes.data_as(abi.c_int32_p), C.byref(st),
                                  C.byref(mo), C.byref(po)), "shud_order_apply")
    try:
        NE = model.num_ele

        def take(ptr, n):
            return np.ctypeslib.as_array(ptr, shape=(n,)).copy() if ptr and n else (np.zeros(0) if ptr else None)

        r = copy.deepcopy(model)                    # reaches, segments, tables, meta: unchanged
        r.nabr = take(mo.nabr, 3 * NE)
        for k in ELE1 + ELE3:
            if k in model.ele:
                r.ele[k] = take(getattr(mo, k), (3 if k in ELE3 else 1) * NE)
        for k in ("ibc", "iss", "ilake"):
            if getattr(model, k) is not None:
                setattr(r, k, take(getattr(mo, k), NE))
        r.seg_ele = take(mo.seg_ele, model.num_seg) if model.num_seg else model.seg_ele.copy()
        r.par = {k: take(getattr(po, k), NE) for k in abi.PARAM_NAMES}
        r.step = {k: order_gather(perm, v) for k, v in model.step.items()}
    finally:
        lib().shud_order_free(st)
    return r.finalize()


def plan_layout(model, mode=abi.SHUD_MODE_SERIAL, partition=None, arrays=False):
    """What RhsHandle(model, mode, partition=partition) would lay out, derived on the host alone
    (shud_rhs_plan_layout): the keys of RhsHandle.layout() plus n_int and riv_sb; arrays=True adds edge_plan [NE]
    (seg_first bits 26-30) and stored_nabr [3, NE] (the neighbours in stored-slot order)."""
    mesh, par = model.mesh_struct(), model.params_struct()
    opt = abi.ShudRhsOptions(mode, 0, None, 1)
    part = None if partition is None else partition.struct()
    info = abi.ShudLayoutInfo()
    NE = model.num_ele
    plan, nabr = (np.zeros(NE, dtype=np.int32), np.zeros((3, NE), dtype=np.int32)) if arrays else (None, None)
    _check(lib().shud_rhs_plan_layout(C.byref(mesh), C.byref(par), C.byref(opt),
                                      None if part is None else C.byref(part), C.byref(info),
                                      None if plan is None else plan.ctypes.data_as(abi.c_int32_p),
                                      None if nabr is None else nabr.ctypes.data_as(abi.c_int32_p)),
           "shud_rhs_plan_layout")
    out = {"packed": bool(info.packed), "n_classes": info.n_classes, "n_int": info.n_int, "riv_sb": info.riv_sb}
    if info.n_streamed:
        out["streamed_fields"] = info.n_streamed
    if info.n_shared:
        out["shared_edges"] = info.n_shared
    if arrays:
        out["edge_plan"], out["stored_nabr"] = plan, nabr
    return out


def nccl_unique_id():
    buf = C.create_string_buffer(128)
    _check(lib().shud_rhs_nccl_unique_id(buf), "nccl_unique_id")
    return buf.raw


class OdeSolver:
    """Device-resident CVODE-semantics integrator (include/shud_ode.h) over an RhsHandle, or over a raw device
    RHS function pointer (tests).  Mirrors SetCVODE (cvode_config.cpp:149-197) + CVode() as SHUD() calls it."""

    def __init__(self, rhs, t0, y0, reltol, abstol, init_step, max_step=0.0, min_step=1e-6,
                 max_num_steps=1000000, maxl=0, max_order=0, fn=None):
        self._opt = abi.ShudOdeOptions(reltol, abstol, init_step, max_step, min_step, max_num_steps, maxl, max_order)
        y0 = np.ascontiguousarray(y0, dtype=np.float64)
        self.n = y0.size
        h = C.c_void_p()
        if fn is None:
            self._rhs = rhs
            if self.n != rhs.num_y:
                raise ValueError(f"y0 has {self.n} entries, expected {rhs.num_y}")
            _check(lib().shud_ode_create(rhs.h, float(t0), y0.ctypes.data, abi.SHUD_WHERE_HOST, C.byref(self._opt),
                                         C.byref(h)), "shud_ode_create")
        else:                                   # fn = (function pointer, user pointer, stream)
            self._fn = fn
            _check(lib().shud_ode_create_fn(self.n, fn[0], fn[1], fn[2], float(t0), y0.ctypes.data,
                                            abi.SHUD_WHERE_HOST, C.byref(self._opt), C.byref(h)), "shud_ode_create_fn")
        self.h = h

    def set_stop_time(self, tstop):
        lib().shud_ode_set_stop_time(self.h, float(tstop))

    def solve(self, tout, one_step=False, y_out=True):
        """CVode(mem, tout, y, &t, CV_NORMAL | CV_ONE_STEP) -> (flag, t, y or None)"""
        y = np.empty(self.n) if y_out else None
        t = C.c_double()
        flag = lib().shud_ode_solve(self.h, float(tout), None if y is None else y.ctypes.data, abi.SHUD_WHERE_HOST,
                                    C.byref(t), abi.ODE_ONE_STEP if one_step else abi.ODE_NORMAL)
        return flag, t.value, y

    def solve_device(self, tout, d_y, one_step=False):
        """CVode() with y(t) written to device memory at d_y (NY doubles): -> (flag, t)"""
        t = C.c_double()
        flag = lib().shud_ode_solve(self.h, float(tout), C.c_void_p(d_y), abi.SHUD_WHERE_DEVICE, C.byref(t),
                                    abi.ODE_ONE_STEP if one_step else abi.ODE_NORMAL)
        return flag, t.value

    def get_dky(self, t, k):
        d = np.empty(self.n)
        flag = lib().shud_ode_get_dky(self.h, float(t), int(k), d.ctypes.data, abi.SHUD_WHERE_HOST)
        return flag, d

    def get_dky_device(self, t, k, d_out):
        """CVodeGetDky(mem, t, k, dky) into device memory at d_out (NY doubles)"""
        flag = lib().shud_ode_get_dky(self.h, float(t), int(k), C.c_void_p(d_out), abi.SHUD_WHERE_DEVICE)
        if flag != abi.ODE_SUCCESS:
            raise RuntimeError(f"shud_ode_get_dky failed with flag {flag}")

    def stats(self):
        s = abi.ShudOdeStats()
        lib().shud_ode_get_stats(self.h, C.byref(s))
        return {k: getattr(s, k) for k, _ in abi.ShudOdeStats._fields_}

    def state_device(self):
        return lib().shud_ode_state_device(self.h)

    def close(self):
        if self.h:
            lib().shud_ode_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Output:
    """The reference's Print_Ctrl set (Control_Data::ExportResults, Model_Control.cpp:123-127) with its buffers
    in HBM (include/shud_out.h): add() = Print_Ctrl::Init[IJ] + open_file, export(t) = ExportResults(t)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        _check(lib().shud_out_create(int(device), None if stream is None else C.c_void_p(stream), C.byref(h)),
               "shud_out_create")
        self.h = h
        self._keep = []

    def add(self, basename, d_src, n_all, interval, iflux, start_time=0, flag_io=None, binary=True, ascii=False,
            radiation_input_mode=0, terrain_radiation=0, solar_lonlat_mode="FORCING_FIRST", lon=0.0, lat=0.0,
            col_src=None, nc=None, legacy=True):
        """col_src [n_all]: column c reads d_src[col_src[c]] (shud_out_add_mapped); flag_io stays by column c.
        nc: "ele" / "riv" / "lake" = a NetCDF sink in the attached file of that kind (shud_out_add_nc); legacy=False
        (OUTPUT_MODE NETCDF) writes no .dat / .csv beside it."""
        flags = None if flag_io is None else np.ascontiguousarray(flag_io, dtype=np.int32)
        cmap = None if col_src is None else np.ascontiguousarray(col_src, dtype=np.int32)
        assert cmap is None or cmap.size == int(n_all)
        bn, sm = str(basename).encode(), str(solar_lonlat_mode).encode()
        spec = abi.ShudPrintSpec(bn, C.c_void_p(d_src), int(n_all), None if flags is None else flags.ctypes.data,
                                 int(interval), int(iflux), int(start_time), int(bool(binary)), int(bool(ascii)),
                                 int(radiation_input_mode), int(terrain_radiation), sm, float(lon), float(lat))
        if nc is not None:
            kind = {"ele": abi.SHUD_NC_ELE, "riv": abi.SHUD_NC_RIV, "lake": abi.SHUD_NC_LAKE}[nc]
            _check(lib().shud_out_add_nc(self.h, C.byref(spec), None if cmap is None else
                                         cmap.ctypes.data_as(abi.c_int32_p), kind, int(bool(legacy))),
                   "shud_out_add_nc")
        elif cmap is None:
            _check(lib().shud_out_add(self.h, C.byref(spec)), "shud_out_add")
        else:
            _check(lib().shud_out_add_mapped(self.h, C.byref(spec), cmap.ctypes.data_as(abi.c_int32_p)),
                   "shud_out_add_mapped")
        self._keep.append((bn, sm, flags))
        return len(self._keep) - 1

    def add_zonal(self, basename, d_src, n_all, interval, iflux, zone, weight=None, op="sum", col_src=None,
                  start_time=0, flag_io=None, binary=True, ascii=False, radiation_input_mode=0, terrain_radiation=0,
                  solar_lonlat_mode="FORCING_FIRST", lon=0.0, lat=0.0, nc=None, n_zone=None):
        """a zonal control (shud_out_add_zonal): zone [n_all] ids by caller column (0: in no zone, 1..NZ), weight
        [n_all] or None, op "sum" (the zone's ordered sum) or "mean" (the weighted mean; needs weight); the file has
        NZ = n_zone (default: the largest id) columns.  col_src and the header keywords are add()'s.  flag_io and nc
        are refused: zone 0 leaves a column out, and a zonal control has no NetCDF sink."""
        if op not in ("sum", "mean"):
            raise ValueError(f"op {op!r}: 'sum' or 'mean'")
        if nc is not None:
            # refused here: the C call has no way to ask for a sink
            raise ShudRhsError(abi.SHUD_ERR_ARG, f"Output.add_zonal({basename}): nc = {nc!r}: a zonal control has no "
                                                 "NetCDF sink")
        zid = np.ascontiguousarray(zone, dtype=np.int32)
        w = None if weight is None else np.ascontiguousarray(weight, dtype=np.float64)
        cmap = None if col_src is None else np.ascontiguousarray(col_src, dtype=np.int32)
        flags = None if flag_io is None else np.ascontiguousarray(flag_io, dtype=np.int32)
        for name, a in (("zone", zid), ("weight", w), ("col_src", cmap), ("flag_io", flags)):
            if a is not None and a.size != int(n_all):
                raise ValueError(f"{name}: {a.size} values, n_all = {int(n_all)}")
        nz = int(zid.max(initial=0)) if n_zone is None else int(n_zone)
        bn, sm = str(basename).encode(), str(solar_lonlat_mode).encode()
        spec = abi.ShudPrintSpec(bn, C.c_void_p(d_src), int(n_all), None if flags is None else flags.ctypes.data,
                                 int(interval), int(iflux), int(start_time), int(bool(binary)), int(bool(ascii)),
                                 int(radiation_input_mode), int(terrain_radiation), sm, float(lon), float(lat))
        zs = abi.ShudZoneSpec(nz, zid.ctypes.data_as(abi.c_int32_p),
                              None if w is None else w.ctypes.data_as(abi.c_double_p),
                              abi.SHUD_ZONE_SUM if op == "sum" else abi.SHUD_ZONE_WMEAN)
        _check(lib().shud_out_add_zonal(self.h, C.byref(spec), None if cmap is None else
                                        cmap.ctypes.data_as(abi.c_int32_p), C.byref(zs)), "shud_out_add_zonal")
        self._keep.append((bn, sm, None))
        return len(self._keep) - 1

    def launches(self):
        """{kernel name: launches the set has enqueued so far} (shud_out_launches)"""
        n = (C.c_int64 * abi.SHUD_OUT_KERNELS)()
        _check(lib().shud_out_launches(self.h, n), "shud_out_launches")
        return {lib().shud_out_kernel_name(k).decode(): int(n[k]) for k in range(abi.SHUD_OUT_KERNELS)}

    def time_pass(self, which, reps):
        """device ms of one export's per-step pass (shud_out_time_pass): which = "zonal" (the two zonal launches) or
        "plain" (k_accumulate over the plain controls); the accumulators grow"""
        ms = C.c_double()
        _check(lib().shud_out_time_pass(self.h, {"zonal": 0, "plain": 1}[which], int(reps), C.byref(ms)),
               "shud_out_time_pass")
        return ms.value

    def attach_nc(self, kind, n_all, forc_start_time, out_dir=None, history=None, crs_wkt=None, mesh=None):
        """attach the NetCDF file of `kind` ("ele", "riv", "lake"; include/shud_nc.h) for add(nc=kind).  out_dir: OUT_DIR
        of the ncoutput cfg (None: beside the legacy files); history: the whole `history` attribute (None: "<UTC now>:
        created by SHUD"); crs_wkt: the WKT text; mesh (kind "ele"): host.Project.mesh_nodes()"""
        spec, keep = nc_spec(kind, n_all, forc_start_time, out_dir, history, crs_wkt, mesh)
        _check(lib().shud_out_attach_nc(self.h, C.byref(spec)), "shud_out_attach_nc")

    def nc_begin(self):
        """write the NetCDF headers now (otherwise at the first export)"""
        _check(lib().shud_out_nc_begin(self.h), "shud_out_nc_begin")

    def time_nc(self, k, reps):
        """device ms per launch of control k's interval-end kernel (shud_out_time_nc; zeroes its accumulator)"""
        ms = C.c_double()
        _check(lib().shud_out_time_nc(self.h, int(k), int(reps), C.byref(ms)), "shud_out_time_nc")
        return ms.value

    def resume(self, on=True):
        """controls added from now on keep the files of an earlier run (shud_out_resume; Checkpoint.restore then cuts
        them back to the checkpoint's length)"""
        _check(lib().shud_out_resume(self.h, int(bool(on))), "shud_out_resume")

    def export(self, t):
        _check(lib().shud_out_export(self.h, float(t)), "shud_out_export")

    def rows(self, k):
        return lib().shud_out_rows(self.h, int(k))

    def flush(self):
        """wait until every exported row is in the files (shud_out_flush)"""
        _check(lib().shud_out_flush(self.h), "shud_out_flush")

    def close(self):
        """shud_out_destroy; raises if the asynchronous writer failed (a lost row or a file write error)"""
        if self.h:
            rc = lib().shud_out_destroy(self.h)
            self.h = None
            _check(rc, "shud_out_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _nc_check(rc, what):
    if rc != abi.SHUD_OK:
        raise ShudRhsError(rc, f"{what}: {lib().shud_nc_last_error().decode(errors='replace')}")


def nc_spec(kind, n_all, forc_start_time, out_dir=None, history=None, crs_wkt=None, mesh=None):
    """abi.ShudNcSpec and the arrays it points at (keep both alive while the spec is in use).  kind: "ele", "riv",
    "lake"; mesh (kind "ele"): dict(node_x, node_y, face_nodes [n_all, 3] 1-based, face_x, face_y)."""
    k = {"ele": abi.SHUD_NC_ELE, "riv": abi.SHUD_NC_RIV, "lake": abi.SHUD_NC_LAKE}[kind]
    enc = lambda v: None if v is None else str(v).encode()
    keep = [enc(out_dir), enc(history), enc(crs_wkt)]
    s = abi.ShudNcSpec(k, int(n_all), keep[0], int(forc_start_time), keep[1], keep[2], 0, None, None, None, None, None)
    if kind == "ele":
        d = [np.ascontiguousarray(mesh[n], dtype=np.float64) for n in ("node_x", "node_y", "face_x", "face_y")]
        fn = np.ascontiguousarray(mesh["face_nodes"], dtype=np.int32).reshape(-1)
        assert d[0].size == d[1].size and d[2].size == d[3].size == int(n_all) and fn.size == 3 * int(n_all)
        s.num_node = d[0].size
        s.node_x, s.node_y, s.face_x, s.face_y = (a.ctypes.data_as(abi.c_double_p) for a in d)
        s.face_nodes = fn.ctypes.data_as(abi.c_int32_p)
        keep += d + [fn]
    return s, keep


class NcFile:
    """One NetCDF output file written on the host (include/shud_nc.h): the reference's NetcdfElementFile /
    NetcdfSimpleFile in the classic 64-bit-offset container.  add_var() = a sink's onInit, put() = its onWrite."""

    def __init__(self, kind, n_all, forc_start_time, out_dir=None, history=None, crs_wkt=None, mesh=None):
        spec, keep = nc_spec(kind, n_all, forc_start_time, out_dir, history, crs_wkt, mesh)
        h = C.c_void_p()
        _nc_check(lib().shud_nc_create(C.byref(spec), C.byref(h)), "shud_nc_create")
        self.h, self.n_all, self.forc_start_time = h, int(n_all), int(forc_start_time)

    def add_var(self, basename, icol, n_all=None):
        """icol: selected columns, 1-based; returns the control's id"""
        ic = np.ascontiguousarray(icol, dtype=np.int32)
        k = C.c_int32()
        _nc_check(lib().shud_nc_add_var(self.h, str(basename).encode(), self.n_all if n_all is None else int(n_all),
                                        self.forc_start_time, ic.ctypes.data_as(abi.c_int32_p), ic.size, C.byref(k)),
                  "shud_nc_add_var")
        return k.value

    def put(self, ctrl, t_quantized, selected):
        v = np.ascontiguousarray(selected, dtype=np.float64)
        _nc_check(lib().shud_nc_put(self.h, int(ctrl), float(t_quantized), v.ctypes.data_as(abi.c_double_p), v.size),
                  "shud_nc_put")

    @property
    def path(self):
        return lib().shud_nc_path(self.h).decode()

    @property
    def num_records(self):
        return lib().shud_nc_num_records(self.h)

    def close(self):
        if self.h:
            rc = lib().shud_nc_close(self.h)
            self.h = None
            _nc_check(rc, "shud_nc_close")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def nc_convert(selected, icol, n_all):
    """the host conversion of a NetCDF put: the n_all slab words as they go to disk (big-endian float, fill at
    unselected positions), as a '>f4' array"""
    v = np.ascontiguousarray(selected, dtype=np.float64)
    ic = np.ascontiguousarray(icol, dtype=np.int32)
    out = np.empty(int(n_all), dtype=">f4")
    _nc_check(lib().shud_nc_convert(v.ctypes.data_as(abi.c_double_p), v.size, ic.ctypes.data_as(abi.c_int32_p), ic.size,
                                    int(n_all), out.ctypes.data), "shud_nc_convert")
    return out


class WaterBalance:
    """The reference's WaterBalanceDiag (SHUD_WB_DIAG) on the device (include/shud_wb.h) over a serial RhsHandle:
    on_et_update() = onETUpdate, sample(t, d_dy) = sample, maybe_write(t) = maybeWrite.  Construct after
    handle.summary(y0).  prefix: <outdir>/<prj>, the five .dat files; None = no files, read() only."""

    def __init__(self, handle, interval, start_time=0.0, trapz=False, prefix=None, forc_start_time=0,
                 radiation_input_mode=0, terrain_radiation=0, solar_lonlat_mode="FORCING_FIRST", lon=0.0, lat=0.0):
        self._rhs = handle
        self.num_ele = handle.model.num_ele
        self._keep = (None if prefix is None else str(prefix).encode(), str(solar_lonlat_mode).encode())
        opt = abi.ShudWbOptions(float(start_time), int(interval), int(bool(trapz)), int(forc_start_time),
                                int(radiation_input_mode), int(terrain_radiation), self._keep[1], float(lon),
                                float(lat), self._keep[0])
        h = C.c_void_p()
        _check(lib().shud_wb_create(handle.h, C.byref(handle._mesh), C.byref(handle._par), C.byref(opt), C.byref(h)),
               "shud_wb_create")
        self.h = h

    def on_et_update(self):
        _check(lib().shud_wb_on_et_update(self.h), "shud_wb_on_et_update")

    def sample(self, t, d_dy):
        _check(lib().shud_wb_sample(self.h, float(t), C.c_void_p(d_dy)), "shud_wb_sample")

    def maybe_write(self, t):
        """True when a row was written"""
        rc = lib().shud_wb_maybe_write(self.h, float(t))
        if rc < 0:
            _check(rc, "shud_wb_maybe_write")
        return rc == 1

    def read(self, arrays=True):
        """dict of host copies: the four accumulators, the residuals of the last written row (arrays=True), the
        basin accumulators / rates / last row, the two storages, last_t, rows, n_outlets"""
        o = abi.ShudWbOut()
        out = {}
        if arrays:
            for name in abi.WB_ARRAYS:
                out[name] = np.zeros(self.num_ele)
                setattr(o, name, out[name].ctypes.data_as(abi.c_double_p))
        _check(lib().shud_wb_read(self.h, C.byref(o)), "shud_wb_read")
        out.update(basin_acc=np.array(o.basin_acc), basin_rate=np.array(o.basin_rate), basin_row=np.array(o.basin_row),
                   storage=np.array(o.storage), last_t=o.last_t, rows=o.rows, n_outlets=o.n_outlets)
        return out

    def time_samples(self, d_dy, reps):
        """milliseconds per sample pass over `reps` passes (HIP events; shud_wb_time_samples)"""
        ms = C.c_double()
        _check(lib().shud_wb_time_samples(self.h, C.c_void_p(d_dy), int(reps), C.byref(ms)), "shud_wb_time_samples")
        return ms.value

    def quad_enable(self):
        """SHUD_WB_DIAG_QUAD: the CV_ONE_STEP monitor and <prefix>.basinwbfull_quad.dat; once, before the first
        sample"""
        _check(lib().shud_wb_quad_enable(self.h), "shud_wb_quad_enable")

    def quad_step(self, t):
        """onCvodeMonitorStep(t) on the flux arrays of the monitor's f() (eval_device + refresh_diagnostics first)"""
        _check(lib().shud_wb_quad_step(self.h, float(t)), "shud_wb_quad_step")

    def read_quad(self):
        """dict of host copies: the seven quad accumulators, the rates of the last integrating monitor step, the
        last written quad row, quad_last_t"""
        acc, rate, row, last_t = np.zeros(7), np.zeros(7), np.zeros(9), C.c_double()
        _check(lib().shud_wb_read_quad(self.h, acc.ctypes.data_as(abi.c_double_p), rate.ctypes.data_as(abi.c_double_p),
                                       row.ctypes.data_as(abi.c_double_p), C.byref(last_t)), "shud_wb_read_quad")
        return {"acc": acc, "rate": rate, "row": row, "last_t": last_t.value}

    def time_quad(self, reps):
        """milliseconds per monitor pass over `reps` passes (HIP events; shud_wb_time_quad)"""
        ms = C.c_double()
        _check(lib().shud_wb_time_quad(self.h, int(reps), C.byref(ms)), "shud_wb_time_quad")
        return ms.value

    def close(self):
        """shud_wb_destroy; raises on a write error.  Call before the handle's close()."""
        if self.h:
            rc = lib().shud_wb_destroy(self.h)
            self.h = None
            _check(rc, "shud_wb_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _dptr(x):
    """device address of a torch tensor (data_ptr) or a raw pointer (int / None)"""
    if x is None:
        return None
    return C.c_void_p(x.data_ptr() if hasattr(x, "data_ptr") else int(x))


class RunMonitors:
    """The reference's run monitors on the device (include/shud_mon.h): add_flood + flood(t) =
    FloodAlert::Init* + FloodWarning(t) into <prj>.flood.csv, add_ic + ic_update(t) = PrintInit(Init_update, t)
    into <prj>.cfg.ic.update.  Independent of the RHS handle: device arrays are torch tensors (float64, contiguous,
    kept alive by the caller) or raw device pointers; rows and snapshots reach the files asynchronously (flush)."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        _check(lib().shud_mon_create(int(device), None if stream is None else C.c_void_p(stream), C.byref(h)),
               "shud_mon_create")
        self.h = h
        self._keep = []

    def add_flood(self, path, d_stage, d_qdown, n_riv, riv_depth, riv_type):
        depth = np.ascontiguousarray(riv_depth, dtype=np.float64)
        typ = np.ascontiguousarray(riv_type, dtype=np.int32)
        assert depth.size == typ.size == int(n_riv)
        pth = str(path).encode()
        spec = abi.ShudFloodSpec(pth, _dptr(d_stage), _dptr(d_qdown), int(n_riv),
                                 depth.ctypes.data_as(abi.c_double_p), typ.ctypes.data_as(abi.c_int32_p))
        self._keep.append((pth, d_stage, d_qdown))
        _check(lib().shud_mon_add_flood(self.h, C.byref(spec)), "shud_mon_add_flood")

    def resume(self, on=True):
        """add_flood keeps the flood file of an earlier run (shud_mon_resume)"""
        _check(lib().shud_mon_resume(self.h, int(bool(on))), "shud_mon_resume")

    def flood(self, t):
        _check(lib().shud_mon_flood(self.h, float(t)), "shud_mon_flood")

    def flood_rows(self):
        """total rows written (waits for the writer)"""
        n = lib().shud_mon_flood_rows(self.h)
        if n < 0:
            _check(int(n), "shud_mon_flood_rows")
        return n

    def flood_last(self):
        """FloodWarning's return value for the last flood() call (waits for the writer)"""
        rc = lib().shud_mon_flood_last(self.h)
        if rc < 0:
            _check(rc, "shud_mon_flood_last")
        return rc

    def add_ic(self, path_update, update_ic_step, d_is, d_snow, d_surf, d_unsat, d_gw, d_riv, d_lake, n_ele, n_riv,
               n_lake=0):
        pth = str(path_update).encode()
        arrs = (d_is, d_snow, d_surf, d_unsat, d_gw, d_riv, d_lake if n_lake else None)
        spec = abi.ShudIcSpec(pth, int(update_ic_step), int(n_ele), int(n_riv), int(n_lake), *[_dptr(a) for a in arrs])
        self._keep.append((pth,) + arrs)
        _check(lib().shud_mon_add_ic(self.h, C.byref(spec)), "shud_mon_add_ic")

    def set_ic_order(self, perm):
        """the snapshot's element arrays are in an internal numbering, perm[k] the file's (0-based) element of source
        element k (shud_mon_set_ic_order); after add_ic"""
        p = np.ascontiguousarray(perm, dtype=np.int32)
        _check(lib().shud_mon_set_ic_order(self.h, p.ctypes.data_as(abi.c_int32_p)), "shud_mon_set_ic_order")

    def ic_update(self, t):
        """True when a snapshot was due and queued"""
        rc = lib().shud_mon_ic_update(self.h, float(t))
        if rc < 0:
            _check(rc, "shud_mon_ic_update")
        return rc == 1

    def ic_snapshots(self):
        n = lib().shud_mon_ic_snapshots(self.h)
        if n < 0:
            _check(int(n), "shud_mon_ic_snapshots")
        return n

    def flush(self):
        """wait until every queued row and snapshot is in its file; raises on the writer's first failure"""
        _check(lib().shud_mon_flush(self.h), "shud_mon_flush")

    def writer_seconds(self):
        return lib().shud_mon_writer_seconds(self.h)

    def time_flood(self, reps):
        """milliseconds per flood pass over `reps` passes (HIP events; shud_mon_time_flood)"""
        ms = C.c_double()
        _check(lib().shud_mon_time_flood(self.h, int(reps), C.byref(ms)), "shud_mon_time_flood")
        return ms.value

    def close(self):
        """shud_mon_destroy; raises if the asynchronous writer failed"""
        if self.h:
            rc = lib().shud_mon_destroy(self.h)
            self.h = None
            _check(rc, "shud_mon_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _ckpt_parts(rhs=None, ode=None, output=None, monitors=None, wb=None):
    def raw(x):
        return None if x is None else x.h
    return abi.ShudCkptParts(raw(rhs), raw(ode), raw(output), raw(monitors), raw(wb))


class Checkpoint:
    """Exact checkpoint / resume of a device run (include/shud_ckpt.h).  snapshot() is called between two solver
    steps, after that step's export and monitors: one device pass packs the live state into a staging slab and the
    call returns; the file is written in the background (flush).  restore() / info() / verify() need no object."""

    def __init__(self, device=0, stream=None):
        h = C.c_void_p()
        _check(lib().shud_ckpt_create(int(device), None if stream is None else C.c_void_p(stream), C.byref(h)),
               "shud_ckpt_create")
        self.h = h

    def snapshot(self, path, t, step, ode, rhs=None, output=None, monitors=None, wb=None):
        """wb: the run's WaterBalance, if any — the checkpoint is then refused (SHUD_ERR_UNSUPPORTED)"""
        parts = _ckpt_parts(rhs, ode, output, monitors, wb)
        _check(lib().shud_ckpt_snapshot(self.h, C.byref(parts), float(t), int(step), str(path).encode()),
               "shud_ckpt_snapshot")

    def flush(self):
        """the last snapshot's file is complete and renamed into place; raises on the writer's first failure"""
        _check(lib().shud_ckpt_flush(self.h), "shud_ckpt_flush")

    def time_pack(self, reps, ode, rhs=None, output=None, monitors=None):
        """(ms per pack pass, bytes it copies) over the live objects (shud_ckpt_time_pack)"""
        parts = _ckpt_parts(rhs, ode, output, monitors)
        ms, nb = C.c_double(), C.c_int64()
        _check(lib().shud_ckpt_time_pack(self.h, C.byref(parts), int(reps), C.byref(ms), C.byref(nb)),
               "shud_ckpt_time_pack")
        return ms.value, nb.value

    @staticmethod
    def restore(path, ode, rhs=None, output=None, monitors=None):
        """-> (t, solver-step index).  The objects are built as for a new run (output controls after
        Output.resume(), the flood monitor after RunMonitors.resume()); a refused restore leaves them untouched."""
        parts = _ckpt_parts(rhs, ode, output, monitors)
        t, step = C.c_double(), C.c_int64()
        _check(lib().shud_ckpt_restore(str(path).encode(), C.byref(parts), C.byref(t), C.byref(step)),
               "shud_ckpt_restore")
        return t.value, step.value

    @staticmethod
    def info(path):
        """header fields (dict) and the section table [(name, offset, words, c0, c1)]"""
        i = abi.ShudCkptInfo()
        _check(lib().shud_ckpt_info(str(path).encode(), C.byref(i)), "shud_ckpt_info")
        d = {k: getattr(i, k) for k, _ in abi.ShudCkptInfo._fields_}
        secs = []
        for k in range(i.n_sections):
            s = abi.ShudCkptSection()
            _check(lib().shud_ckpt_section(str(path).encode(), k, C.byref(s)), "shud_ckpt_section")
            secs.append((s.name.decode(), s.offset, s.words, s.c0, s.c1))
        d["sections"] = secs
        return d

    @staticmethod
    def verify(path):
        _check(lib().shud_ckpt_verify(str(path).encode()), "shud_ckpt_verify")

    def close(self):
        """shud_ckpt_destroy (waits for the drain); raises if the writer failed"""
        if self.h:
            rc = lib().shud_ckpt_destroy(self.h)
            self.h = None
            _check(rc, "shud_ckpt_destroy")

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def write_ic_host(path, t, y_is, y_snow, y_surf, y_unsat, y_gw, y_riv, y_lake=None):
    """PrintInit's file from host arrays (shud_mon_write_ic_host): the .cfg.ic layout, through <path>.tmp + rename"""
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (y_is, y_snow, y_surf, y_unsat, y_gw, y_riv)]
    lake = None if y_lake is None or len(y_lake) == 0 else np.ascontiguousarray(y_lake, dtype=np.float64)
    ne, nr, nl = a[0].size, a[5].size, 0 if lake is None else lake.size
    assert all(v.size == ne for v in a[:5])
    ptr = [v.ctypes.data_as(abi.c_double_p) for v in a] + [None if lake is None else lake.ctypes.data_as(abi.c_double_p)]
    _check(lib().shud_mon_write_ic_host(str(path).encode(), float(t), ne, nr, nl, *ptr), "shud_mon_write_ic_host")


def format_flood_rows(t, idx, riv_type, stage, riv_depth, q):
    """FloodWarning's rows (bytes) for packed records: record k is reach idx[k] (0-based) with stage[k], q[k];
    riv_type / riv_depth are per-reach arrays (shud_mon_format_flood_rows)"""
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    typ = np.ascontiguousarray(riv_type, dtype=np.int32)
    st, dp, qq = (np.ascontiguousarray(v, dtype=np.float64) for v in (stage, riv_depth, q))
    args = (float(t), idx.ctypes.data_as(abi.c_int32_p), typ.ctypes.data_as(abi.c_int32_p),
            st.ctypes.data_as(abi.c_double_p), dp.ctypes.data_as(abi.c_double_p), qq.ctypes.data_as(abi.c_double_p),
            int(idx.size))
    n = lib().shud_mon_format_flood_rows(None, 0, *args)
    if n < 0:
        _check(int(n), "shud_mon_format_flood_rows")
    buf = C.create_string_buffer(n + 1)
    lib().shud_mon_format_flood_rows(buf, n + 1, *args)
    return buf.raw[:n]
