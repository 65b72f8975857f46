"""Plain-Python restatement of the run monitors' files (include/shud_mon.h), byte for byte, from numpy arrays:
  flood_header / flood_rows / flood_file   FloodAlert::InitFile + FloodWarning (src/classes/FloodAlert.cpp:62-87)
  ic_file                                  Model_Data::PrintInit (src/ModelData/MD_update.cpp:268-299)
  ic_due                                   PrintInit's schedule test
Python's '%f' % x and '%.1f' % x are correctly rounded like glibc's for finite values; non-finite values (whose
sign and spelling are glibc's business, e.g. '-nan') go through glibc's snprintf via ctypes, as
oracle/numpy_oracle.py does for libm."""
import ctypes as C
import ctypes.util
import math

import numpy as np

_LIBC = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
_LIBC.snprintf.restype = C.c_int

FLOOD_HEADER = b"time\tID\tType\tStage_m\tBank_m\tDischarge_m3/day\n"


def _f(x, fmt="%f"):
    x = float(x)
    if math.isfinite(x):
        return (fmt % x).encode()
    buf = C.create_string_buffer(64)
    _LIBC.snprintf(buf, C.c_size_t(64), fmt.encode(), C.c_double(x))
    return buf.value


def flood_rows(t, stage, depth, rtype, qdown):
    """rows of one FloodWarning(t) call (bytes) and their count: reach i iff stage[i] > depth[i], ascending i"""
    stage, depth, qdown = (np.asarray(v, dtype=np.float64) for v in (stage, depth, qdown))
    out = []
    for i in range(stage.size):
        if stage[i] > depth[i]:                  # strict: False for NaN, True for +inf
            out.append(b"%s\t%d\t%d\t%s\t%s\t%s\n" % (_f(t, "%.1f"), i + 1, int(rtype[i]), _f(stage[i]),
                                                      _f(depth[i]), _f(qdown[i])))
    return b"".join(out), len(out)


def flood_file(calls, depth, rtype):
    """the whole file after calls = [(t, stage, qdown), ...]; returns (bytes, total rows, last call's flag)"""
    txt, total, last = FLOOD_HEADER, 0, 0
    for t, stage, qdown in calls:
        rows, n = flood_rows(t, stage, depth, rtype, qdown)
        txt += rows
        total += n
        last = int(n > 0)
    return txt, total, last


def ic_due(t, update_ic_step):
    """((unsigned long)(long)t) % UpdateICStep == 0"""
    return (int(t) % (1 << 64)) % int(update_ic_step) == 0


def ic_file(t, y_is, y_snow, y_surf, y_unsat, y_gw, y_riv, y_lake=None):
    cols = [np.asarray(v, dtype=np.float64) for v in (y_is, y_snow, y_surf, y_unsat, y_gw)]
    riv = np.asarray(y_riv, dtype=np.float64)
    ne = cols[0].size
    out = [b"%d\t %d \t%s\n" % (ne, 6, _f(t)), b"Index\tCanopy\tSnow\tSurface\tUnsat\tGW\n"]
    for i in range(ne):
        out.append(b"%d\t%s\n" % (i + 1, b"\t".join(_f(c[i]) for c in cols)))
    out.append(b"%d\t%d\n" % (riv.size, 2))
    out.append(b"Index\tStage\n")
    for i in range(riv.size):
        out.append(b"%d\t%s\n" % (i + 1, _f(riv[i])))
    if y_lake is not None and len(y_lake) > 0:
        lake = np.asarray(y_lake, dtype=np.float64)
        out.append(b"%d\t%d\n" % (lake.size, 2))
        out.append(b"Index\tLakeStage\n")
        for i in range(lake.size):
            out.append(b"%d\t%s\n" % (i + 1, _f(lake[i])))
    return b"".join(out)


def read_back(text):
    """the double the project reader makes of a number's text: strtold, then the conversion to double
    (TabularData::read, src/classes/TabularData.cpp:27-55).  About one 6-decimal text in 15,000 lands one ulp
    from float(text) through the intermediate 64-bit mantissa."""
    return np.float64(np.longdouble(text.decode() if isinstance(text, bytes) else text))


def parse_ic(path):
    """(t, element table [n][5], river stages, lake stages or None) of a .cfg.ic-layout file, values as text"""
    ln = open(path).read().split("\n")
    ne = int(ln[0].split()[0])
    t = float(ln[0].split()[2])
    ele = [r.split("\t")[1:] for r in ln[2:2 + ne]]
    k = 2 + ne
    nr = int(ln[k].split()[0])
    riv = [r.split("\t")[1] for r in ln[k + 2:k + 2 + nr]]
    k += 2 + nr
    lake = None
    if k < len(ln) and ln[k].strip():
        nl = int(ln[k].split()[0])
        lake = [r.split("\t")[1] for r in ln[k + 2:k + 2 + nl]]
    return t, ele, riv, lake
