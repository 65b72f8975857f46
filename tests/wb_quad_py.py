"""Pure numpy / Python restatement of the reference's SHUD_WB_DIAG_QUAD monitor (test infrastructure: the checker of
shud_wb_quad_enable / shud_wb_quad_step / the quad row of shud_wb_maybe_write, include/shud_wb.h).  Written from
the algorithm of src/Model/WaterBalanceDiag.cpp: the enable (:271,315,326-338,359-364), onCvodeMonitorStep
(:681-717), the quad row of maybeWrite (:597-623); and of the basin rates f() forms for the monitor
(src/ModelData/MD_f.cpp:57-86,115-128,193-213).  It sits on wb_py's helpers and leaves wb_py as it is.

The seven rates are sums: `quad_rates` takes the summation order like wb_py.WaterBalancePy does (the device's fixed
tree, wb_py.device_sum, or the reference's sequential loop).  The monitor step and the row are scalar IEEE
operations in the reference's order, so given the rates everything after them is comparable bit for bit."""
import numpy as np

import wb_py

QUAD_LABEL, QUAD_EXT = "basinwbfull_quad (m3)", ".basinwbfull_quad.dat"


def quad_terms(m, ic_raw, d, prcp):
    """per-lane terms of the seven rates as {name: array}, from the flux arrays `d` of the monitor's f()
    (RhsHandle.diagnostics()).  They are wb_py.sample_terms' except Qout: QrivDown as f() computed it, one value
    per reach (0.0 for a reach that is no outlet), not the outlet discharge re-evaluated from the stage."""
    NE = m.num_ele
    area = m.ele["area"]
    nb = np.asarray(m.nabr).reshape(3, NE)
    qe = d["qele_surf"].reshape(3, NE) + d["qele_sub"].reshape(3, NE)
    nc, edge = np.zeros(NE), np.zeros(NE)
    for j in range(3):
        nc = np.where(nb[j] >= 0, nc + qe[j], nc)
        edge = np.where(nb[j] < 0, edge + qe[j], edge)
    qout = np.zeros(m.num_riv)
    outs = wb_py.outlet_list(m)
    qout[outs] = np.asarray(d["qriv_down"], dtype=np.float64)[outs]
    return {"P": prcp * area,
            "ET": (ic_raw + d["q_es"] + d["q_eu"] + d["q_eg"] + d["q_tu"] + d["q_tg"]) * area,
            "Qout": qout, "Qedge": edge if not m.close_boundary else np.zeros(0),
            "Qbc": wb_py.ele_qbc(m), "Qbc_riv": wb_py.riv_qbc(m), "Qss": np.zeros(NE), "noncons": nc,
            **wb_py.edge_terms(m, qe, nb)}


def quad_rates(m, ic_raw, d, prcp, order="device"):
    """the seven rates [P, ET, Qout, Qedge, Qbc, Qss, noncons] in m3/min"""
    s = wb_py.device_sum if order == "device" else wb_py.seq_sum
    tm = quad_terms(m, ic_raw, d, prcp)
    return wb_py.basin_rates(tm, s, order != "device")


def quad_row(ds_total, acc):
    """:598-617: {dS, P, ET, Qout, Qedge, Qbc, Qss, noncons, dS - (P + Qbc + Qss - ET - Qout - Qedge)}"""
    A = [float(x) for x in acc]
    net = A[0] + A[4] + A[5] - A[1] - A[2] - A[3]
    return np.array([float(ds_total)] + A + [float(ds_total) - net])


class QuadMonitorPy:
    """the monitor's state; `basin`: the wb_py.WaterBalancePy whose rows the quad rows accompany (it supplies the
    write gate, t_quantized and ds_total; its trapz switch is not read)"""

    def __init__(self, basin, start_time=0.0, prefix=None, **header):
        self.basin = basin
        self.acc = np.zeros(7)
        self.prev = np.zeros(7)
        self.rate = np.zeros(7)
        self.row = np.zeros(9)
        self.last_t = float(start_time)
        self.has_prev = False
        self.steps = 0                   # integrating steps
        self.rows = 0
        self.fp = None
        if prefix is not None:
            self.fp = open(str(prefix) + QUAD_EXT, "wb")
            self.fp.write(wb_py.header_bytes(QUAD_LABEL, 9, **header))

    def step(self, t, rates):
        """onCvodeMonitorStep(t) with the rates of the f() just before it"""
        dt = t - self.last_t
        if not dt > 0.0:
            self.last_t = t
            return
        r = np.array(rates, dtype=np.float64)
        for k in range(7):
            if self.has_prev:
                self.acc[k] = self.acc[k] + 0.5 * (self.prev[k] + r[k]) * dt
            else:
                self.acc[k] = self.acc[k] + r[k] * dt
        self.has_prev = True
        self.prev = r.copy()
        self.rate = r
        self.last_t = t
        self.steps += 1

    def write(self, tq, ds_total):
        """:597-623: the row from the basin row's ds_total at its t_quantized; the accumulators are zeroed, the
        previous rates and quad_last_t are kept"""
        self.row = quad_row(ds_total, self.acc)
        if self.fp is not None:
            self.fp.write(wb_py.record_bytes(tq, self.row))
        self.acc = np.zeros(7)
        self.rows += 1

    def maybe_write(self, t, state):
        """maybeWrite(t): the basin restatement's rows, then the quad row at the same gate and row time"""
        b = self.basin
        if not b.maybe_write(t, state):
            return False
        self.write(float(b.last_written_floor - b.interval), b.basin_row[0])
        return True

    def close(self):
        if self.fp is not None:
            self.fp.close()
            self.fp = None
