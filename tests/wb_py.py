"""Pure numpy / Python restatement of the reference's water-balance diagnostics (test infrastructure: the checker
of include/shud_wb.h).  Written from the algorithm of src/Model/WaterBalanceDiag.cpp: openFiles (:258-369),
writeDatHeader / writeDatRecord (:90-150), initBasinOutlets (:152-166), the storage and outlet functions
(:168-256), onETUpdate (:399-408), sample (:410-529) and maybeWrite (:531-636).  cbrt is glibc's, through libm as
in oracle/numpy_oracle.py.

Per element every expression keeps the reference's operation order, so the four accumulators and the four
residual arrays are comparable bit for bit.  The basin sums are order dependent: `basin_sum` is either the
reference's sequential loop (math-order "seq") or the device's fixed reduction tree ("device", restated by
`device_sum`), which the byte-identical file tests use; the bound tests compare the device against math.fsum."""
import ctypes
import ctypes.util
import math
import struct

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.cbrt.restype = ctypes.c_double
_libm.cbrt.argtypes = [ctypes.c_double]

GRAV = 9.8
LABELS = [("elewb3_resid", ".elewb3_resid.dat"), ("elewbfull_resid", ".elewbfull_resid.dat"),
          ("elewb3_budget_resid", ".elewb3_budget_resid.dat"),
          ("elewbfull_budget_resid", ".elewbfull_budget_resid.dat"), ("basinwbfull (m3)", ".basinwbfull.dat")]
BASIN = ["P", "ET", "Qout", "Qedge", "Qbc", "Qss", "noncons"]
BLOCK = 1024          # threads per workgroup of the device passes; also the finalize block
FIN_ACC = 4


def env_truthy(s):
    """:21-36"""
    if s is None or s == "":
        return False
    return not (s == "0" or s.lower() == "false" or s.lower() == "off")


def choose_interval(dt_qe_et, dt_ye_surf):
    """:10-19"""
    if dt_qe_et > 0:
        return dt_qe_et
    if dt_ye_surf > 0:
        return dt_ye_surf
    return 1440


def write_gate(t, interval, last_written_floor):
    """maybeWrite's gate (:541-550): the floor to write at, or None"""
    tf = int(math.floor(t))
    if interval <= 0 or tf < interval or tf % interval != 0 or tf == last_written_floor:
        return None
    return tf


def header_bytes(label, num_var, forc_start_time=0, radiation_input_mode=0, terrain_radiation=0,
                 solar_lonlat_mode="FORCING_FIRST", lon=0.0, lat=0.0):
    """writeDatHeader (:90-130): 1024 zero-filled bytes of text, StartTime, NumVar, icol = 1..NumVar"""
    text = ("# SHUD output\n"
            f"# Water-balance diagnostic: {label}\n"
            f"# Radiation input mode: {'SWNET' if radiation_input_mode == 1 else 'SWDOWN'}\n"
            f"# Terrain radiation (TSR): {'ON' if terrain_radiation else 'OFF'}\n"
            f"# Solar lon/lat mode: {solar_lonlat_mode}\n"
            f"# Solar lon/lat (deg): lon={lon:.6f}, lat={lat:.6f}\n").encode()
    return (text[:1023].ljust(1024, b"\0") + struct.pack("<dd", float(forc_start_time), float(num_var)) +
            np.arange(1, num_var + 1, dtype=np.float64).tobytes())


def record_bytes(t, values):
    """writeDatRecord (:132-150)"""
    return struct.pack("<d", float(t)) + np.ascontiguousarray(values, dtype=np.float64).tobytes()


def _tree(v):
    """a wave64 xor butterfly (offsets 32 .. 1) / the wave-results butterfly: halves folded onto each other"""
    while v.shape[-1] > 1:
        h = v.shape[-1] // 2
        v = v[..., :h] + v[..., h:]
    return v[..., 0]


def _block_sum(v):
    """[nblk, BLOCK] -> [nblk]: per wave the butterfly, then the BLOCK/64 wave results by one wave"""
    return _tree(_tree(v.reshape(v.shape[0], BLOCK // 64, 64)))


def device_sum(terms):
    """sum of one value per lane in the device's fixed order: workgroups of BLOCK lanes (idle lanes add 0.0) leave
    one partial each; the one-block finalize gives thread t the partials t + (FIN_ACC*j + k)*BLOCK in accumulator k,
    takes (a0 + a1) + (a2 + a3) and reduces the BLOCK results like a workgroup"""
    v = np.asarray(terms, dtype=np.float64)
    if v.size == 0:
        return 0.0
    nblk = -(-v.size // BLOCK)
    part = _block_sum(np.concatenate([v, np.zeros(nblk * BLOCK - v.size)]).reshape(nblk, BLOCK))
    nj = -(-nblk // (FIN_ACC * BLOCK))
    p = np.concatenate([part, np.zeros(nj * FIN_ACC * BLOCK - nblk)]).reshape(nj, FIN_ACC, BLOCK)
    acc = np.zeros((FIN_ACC, BLOCK))
    for j in range(nj):
        acc = acc + p[j]
    x = (acc[0] + acc[1]) + (acc[2] + acc[3])
    return float(_block_sum(x.reshape(1, BLOCK))[0])


def seq_sum(terms):
    """the reference's loop: s = 0; s += term"""
    s = 0.0
    for x in np.asarray(terms, dtype=np.float64):
        s += float(x)
    return s


def host_summary(m, y):
    """Model_Data::summary (MD_update.cpp:190-216): (ysf, yus, ygw, yriv) with the head boundary conditions"""
    NE, NR = m.num_ele, m.num_riv
    y = np.asarray(y, dtype=np.float64)
    gw = y[2 * NE:3 * NE].copy()
    stg = y[3 * NE:3 * NE + NR].copy()
    ibc, rb = np.asarray(m.ibc), np.asarray(m.riv_bc)
    if (ibc > 0).any():
        gw[ibc > 0] = m.bc_tables["ele_ybc"][ibc[ibc > 0]]
    if (rb > 0).any():
        stg[rb > 0] = m.bc_tables["riv_ybc"][rb[rb > 0]]
    return y[:NE].copy(), y[NE:2 * NE].copy(), gw, stg


def river_geometry(m, stage):
    """_River::updateRiver (River.cpp:49-62): (u_CSarea, u_CSperem), clamped at 0"""
    w0, s = m.riv["riv_bottom_width"], m.riv["riv_bankslope"]
    y = np.asarray(stage, dtype=np.float64)
    area = y * (w0 + y * s)
    ys = y * s
    perem = 2.0 * np.sqrt(y * y + ys * ys) + w0
    return np.where(area < 0.0, 0.0, area), np.where(perem < 0.0, 0.0, perem)


def outlet_list(m):
    """initBasinOutlets (:152-166); lake models are out of scope (no toLake)"""
    return np.nonzero(np.asarray(m.riv_down) < 0)[0]


def manning(area, rough, r, s):
    """ManningEquation (Equations.hpp:54-63) with pow23(R) = cbrt(R)^2"""
    t = _libm.cbrt(float(r))
    p23 = t * t
    if s > 0:
        return math.sqrt(s) * area * p23 / rough
    return -1.0 * math.sqrt(-s) * area * p23 / rough


def outlet_terms(m, stage):
    """the terms of basinOutletDischarge_m3min (:197-230), one per reach (0.0 for a reach that is no outlet)"""
    csarea, perem = river_geometry(m, stage)
    q = np.zeros(m.num_riv)
    with np.errstate(invalid="ignore"):
        for i in outlet_list(m):
            a, p, st = float(csarea[i]), float(perem[i]), float(stage[i])
            r = 0.0 if p <= 0.0 else a / p
            if m.riv_down[i] == -4:
                q[i] = a * float(np.sqrt(np.float64(GRAV * st))) * 60.0
            else:
                s = float(m.riv["riv_bed_slope"][i]) + st * 2.0 / float(m.riv["riv_length"][i])
                q[i] = manning(a, float(m.riv["riv_avg_rough"][i]), r, s)
    return q


def river_storage_terms(m, stage):
    """the terms of basinRiverStorage_m3 (:183-195)"""
    csarea, _ = river_geometry(m, stage)
    return csarea * m.riv["riv_length"]


def ele_qbc(m):
    """Ele[i].QBC (MD_update.cpp:114-125): the flux table's column -iBC where iBC < 0, else 0"""
    ibc = np.asarray(m.ibc)
    q = np.zeros(m.num_ele)
    if (ibc < 0).any():
        q[ibc < 0] = m.bc_tables["ele_qbc"][-ibc[ibc < 0]]
    return q


def riv_qbc(m):
    rb = np.asarray(m.riv_bc)
    q = np.zeros(m.num_riv)
    if (rb < 0).any():
        q[rb < 0] = m.bc_tables["riv_qbc"][-rb[rb < 0]]
    return q


def sample_terms(m, ic_raw, d, prcp, stage):
    """per-lane terms of the seven basin rates of sample (:465-497) as {name: array}; Qbc has the element and the
    reach terms apart ("Qbc", "Qbc_riv"), the edge sums one value per element (edges j = 0, 1, 2 in order)"""
    NE = m.num_ele
    area = m.ele["area"]
    nb = np.asarray(m.nabr).reshape(3, NE)
    qe = d["qele_surf"].reshape(3, NE) + d["qele_sub"].reshape(3, NE)
    nc, edge = np.zeros(NE), np.zeros(NE)
    for j in range(3):
        nc = np.where(nb[j] >= 0, nc + qe[j], nc)
        edge = np.where(nb[j] < 0, edge + qe[j], edge)
    return {"P": prcp * area,
            "ET": (ic_raw + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * area,
            "Qout": outlet_terms(m, stage), "Qedge": edge if not m.close_boundary else np.zeros(0),
            "Qbc": ele_qbc(m), "Qbc_riv": riv_qbc(m), "Qss": np.zeros(NE), "noncons": nc,
            **edge_terms(m, qe, nb)}


def edge_terms(m, qe, nb):
    """the edge sums as the reference's loops add them: one term per edge in the order (element i, edge j), each
    added to the running total on its own (:244-254, :483-488), not one value per element; 0.0 where an edge does
    not count (adding it leaves the total as it is)"""
    nc = np.where(nb >= 0, qe, 0.0).T.ravel()
    edge = np.where(nb < 0, qe, 0.0).T.ravel() if not m.close_boundary else np.zeros(0)
    return {"noncons_edges": nc, "Qedge_edges": edge}


def basin_rates(tm, total, seq):
    """the seven rates from the terms.  seq: the reference's association (every edge its own term; the reach
    boundary fluxes go on adding to the element ones in one accumulator, :477-494); else one value per element
    and two sums for Qbc, the device's"""
    if seq:
        return np.array([total(tm["P"]), total(tm["ET"]), total(tm["Qout"]), total(tm["Qedge_edges"]),
                         total(np.concatenate([tm["Qbc"], tm["Qbc_riv"]])), total(tm["Qss"]),
                         total(tm["noncons_edges"])])
    return np.array([total(tm["P"]), total(tm["ET"]), total(tm["Qout"]), total(tm["Qedge"]),
                     total(tm["Qbc"]) + total(tm["Qbc_riv"]), total(tm["Qss"]), total(tm["noncons"])])


class WaterBalancePy:
    """state: (ysf, yus, ygw, yriv, snow, is) of host_summary + the ET prelude's storages (zeros without one)"""

    def __init__(self, m, interval, state, start_time=0.0, trapz=False, prefix=None, order="device", **header):
        self.m, self.interval, self.trapz = m, int(interval), bool(trapz)
        self.sum = device_sum if order == "device" else seq_sum
        self.seq = order != "device"
        NE = m.num_ele
        self.sy, self.area = m.par["Sy"], m.ele["area"]
        self.ic_raw = np.zeros(NE)
        self.acc = [np.zeros(NE) for _ in range(4)]            # flux3, fluxfull, budget3, budgetfull
        self.prev = [np.zeros(NE) for _ in range(4)]
        self.resid = [np.zeros(NE) for _ in range(4)]
        self.s3_prev, self.sfull_prev = self._storage(state)
        self.s_ele_prev = self.sum(self.sfull_prev * self.area)
        self.s_riv_prev = self.sum(river_storage_terms(m, state[3]))
        self.storage = (self.s_ele_prev, self.s_riv_prev)
        self.basin_acc = np.zeros(7)
        self.basin_prev = np.zeros(7)
        self.basin_rate = np.zeros(7)
        self.basin_row = np.zeros(9)
        self.has_prev_rate = False
        self.last_t = float(start_time)
        self.last_written_floor = -1
        self.rows = 0
        self.fp = []
        if prefix is not None:
            for k, (label, ext) in enumerate(LABELS):
                f = open(str(prefix) + ext, "wb")
                f.write(header_bytes(label, NE if k < 4 else 9, **header))
                self.fp.append(f)

    def _storage(self, state):
        ysf, yus, ygw, _, snow, is_ = state
        s3 = ysf + self.sy * yus + self.sy * ygw
        return s3, s3 + snow + is_

    def on_et_update(self, e_ic):
        self.ic_raw = np.array(e_ic, dtype=np.float64)

    def _integrate(self, acc, prev, rate, dt):
        if self.trapz and self.has_prev_rate:
            return acc + 0.5 * (prev + rate) * dt
        return acc + rate * dt

    def sample(self, t, dy, d, prcp, net_prep, stage):
        """d: the flux arrays of the last f() (RhsHandle.diagnostics()); stage: yRivStg"""
        dt = t - self.last_t
        if not dt > 0.0:
            self.last_t = t
            return
        m = self.m
        NE = m.num_ele
        sy, area, ic = self.sy, self.area, self.ic_raw
        dy = np.asarray(dy, dtype=np.float64)
        net3 = dy[:NE] + sy * dy[NE:2 * NE] + sy * dy[2 * NE:3 * NE]
        netfull = net3 + (prcp - net_prep) - ic
        et3 = d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]
        qlat3 = (d["qele_surf_tot"] + d["qele_sub_tot"]) / area
        qbc = np.where(np.asarray(m.ibc) < 0, ele_qbc(m) / area, 0.0)
        qss = np.where(np.asarray(m.iss) != 0, 0.0 / area, 0.0)
        net3_b = net_prep - et3 - qlat3 + qbc + qss
        netfull_b = prcp - (ic + et3) - qlat3 + qbc + qss
        for k, rate in enumerate((net3, netfull, net3_b, netfull_b)):
            self.acc[k] = self._integrate(self.acc[k], self.prev[k], rate, dt)
            self.prev[k] = rate
        tm = sample_terms(m, ic, d, prcp, stage)
        rate = basin_rates(tm, self.sum, self.seq)
        for k in range(7):
            self.basin_acc[k] = float(self._integrate(self.basin_acc[k], self.basin_prev[k], rate[k], dt))
        self.basin_prev = rate.copy()
        self.basin_rate = rate
        self.has_prev_rate = True
        self.last_t = t

    def maybe_write(self, t, state):
        tf = write_gate(t, self.interval, self.last_written_floor)
        if tf is None:
            return False
        s3, sfull = self._storage(state)
        self.resid = [s3 - self.s3_prev - self.acc[0], sfull - self.sfull_prev - self.acc[1],
                      s3 - self.s3_prev - self.acc[2], sfull - self.sfull_prev - self.acc[3]]
        self.s3_prev, self.sfull_prev = s3, sfull
        self.acc = [np.zeros(self.m.num_ele) for _ in range(4)]
        tq = float(tf - self.interval)
        s_ele = self.sum(sfull * self.area)
        s_riv = self.sum(river_storage_terms(self.m, state[3]))
        ds_total = (s_ele - self.s_ele_prev) + (s_riv - self.s_riv_prev)
        A = [float(x) for x in self.basin_acc]
        net = A[0] + A[4] + A[5] - A[1] - A[2] - A[3]
        self.basin_row = np.array([ds_total] + A + [ds_total - net])
        for k, f in enumerate(self.fp):
            f.write(record_bytes(tq, self.resid[k] if k < 4 else self.basin_row))
        self.s_ele_prev, self.s_riv_prev = s_ele, s_riv
        self.storage = (s_ele, s_riv)
        self.basin_acc = np.zeros(7)
        self.last_written_floor = tf
        self.rows += 1
        return True

    def close(self):
        for f in self.fp:
            f.close()
        self.fp = []
