"""Plain numpy restatement of a zonal print control (include/shud_out.h: shud_out_add_zonal), written from the header's
definition and built on ode_kernels_py.device_order_sum, the restatement of csrc/shud_reduce.h's order that
tests/test_ode_kernels.py pins.  Every operation is one IEEE addition, multiplication or division in a stated order, so
the same expression in numpy is a bit-exact reference: no tolerance anywhere.  Not a test module.

  members of zone z: the columns c with zone[c] == z, ascending c
  term             : p_c = weight[c] * x_c (x_c when there is no weight), x_c = src[col_src[c]] (src[c] without col_src)
  S_z              : device_order_sum(p over the members); +0.0 for a zone without members
  every export     : buf_z += S_z
  interval's end   : row_z = buf_z * (tau / NumUpdate), for "mean" divided by W_z = device_order_sum(weights of z);
                     then buf_z = 0
"""
import numpy as np

import ode_kernels_py as K


def members(zone, nz):
    """[columns of zone 1, ..., columns of zone nz], each ascending"""
    zone = np.asarray(zone)
    order = np.argsort(zone, kind="stable")
    cuts = np.searchsorted(zone[order], np.arange(1, nz + 2))
    return [order[cuts[k]:cuts[k + 1]] for k in range(nz)]


def zone_sums(src, zone, nz, weight=None, col_src=None, mem=None):
    """S_z, z = 1..nz, of one export"""
    src = np.asarray(src, dtype=np.float64)
    x = src if col_src is None else src[np.asarray(col_src)]
    p = x if weight is None else np.asarray(weight, dtype=np.float64) * x
    mem = members(zone, nz) if mem is None else mem
    return np.array([K.device_order_sum(p[m]) if m.size else 0.0 for m in mem])


def serial_zone_sums(src, zone, nz, weight=None):
    """the same terms summed left to right (not the device's order: what the restatement must differ from)"""
    p = np.asarray(src, dtype=np.float64) if weight is None else np.asarray(weight) * np.asarray(src)
    return np.array([np.cumsum(p[m])[-1] if m.size else 0.0 for m in members(zone, nz)])


class ZonalControl:
    """one zonal control: export(src) at every step, row(tau) at an interval's end -> the row's NZ values"""

    def __init__(self, zone, nz, weight=None, op="sum", col_src=None):
        assert op in ("sum", "mean")
        self.zone, self.nz, self.weight, self.op, self.col_src = np.asarray(zone), nz, weight, op, col_src
        self.mem = members(self.zone, nz)
        self.buf = np.zeros(nz)
        self.num_update = 0
        if op == "mean":
            w = np.asarray(weight, dtype=np.float64)
            self.wsum = np.array([K.device_order_sum(w[m]) for m in self.mem])

    def export(self, src):
        self.buf = self.buf + zone_sums(src, self.zone, self.nz, self.weight, self.col_src, self.mem)
        self.num_update += 1

    def row(self, tau=1.0):
        with np.errstate(invalid="ignore", over="ignore"):
            v = self.buf * (tau / self.num_update)
            if self.op == "mean":
                v = v / self.wsum
        self.buf = np.zeros(self.nz)
        self.num_update = 0
        return v
