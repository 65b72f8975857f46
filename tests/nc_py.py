"""Pure-Python restatement of the NetCDF output files (include/shud_nc.h), packed with `struct` from the NetCDF
classic format specification (64-bit-offset variant, magic "CDF\\x02") and the reference's list of dimensions, variables
and attributes (NetcdfElementFile / NetcdfSimpleFile, src/classes/NetcdfOutputContext.cpp:314-951).

    header   = magic numrecs dim_list gatt_list var_list
    dim_list = NC_DIMENSION nelems [name length]...          gatt_list / vatt_list = NC_ATTRIBUTE nelems [attr]...
    attr     = name nc_type nelems values(padded to 4)       an absent list is ZERO ZERO
    var      = name ndims [dimid]... vatt_list nc_type vsize(4 bytes) begin(8 bytes)
    data     = fixed variables in definition order, then numrecs records (the record variables' slabs in order)

`build(spec, ctrls, puts)` returns the bytes of the whole file after the given puts."""
import struct

import numpy as np

NC_CHAR, NC_INT, NC_FLOAT, NC_DOUBLE = 2, 4, 5, 6
NC_DIMENSION, NC_VARIABLE, NC_ATTRIBUTE = 10, 11, 12
FILL = np.float32(9.96921e36)
FILL_INT = -2147483647

META = {
    "eleyic": ("m", "interception storage"), "eleysnow": ("m", "snow depth"),
    "eleysurf": ("m", "surface water depth"), "eleyunsat": ("m", "unsaturated zone storage depth"),
    "eleygw": ("m", "groundwater head"), "elevprcp": ("m/day", "precipitation to land"),
    "elevnetprcp": ("m/day", "net precipitation"), "elevetp": ("m/day", "potential evapotranspiration"),
    "eleveta": ("m/day", "actual evapotranspiration"), "elevrech": ("m/day", "recharge"),
    "elevinfil": ("m/day", "infiltration"), "elevexfil": ("m/day", "exfiltration"),
    "elevetic": ("m/day", "evapotranspiration: interception"),
    "elevettr": ("m/day", "evapotranspiration: transpiration"),
    "elevetev": ("m/day", "evapotranspiration: evaporation"),
    "eleqrsurf": ("m3/day", "element to river surface flow"),
    "eleqrsub": ("m3/day", "element to river subsurface flow"),
    "eleqsub": ("m3/day", "subsurface flow: total"), "eleqsub1": ("m3/day", "subsurface flow: direction 1"),
    "eleqsub2": ("m3/day", "subsurface flow: direction 2"), "eleqsub3": ("m3/day", "subsurface flow: direction 3"),
    "eleqsurf": ("m3/day", "surface flow: total"), "eleqsurf1": ("m3/day", "surface flow: direction 1"),
    "eleqsurf2": ("m3/day", "surface flow: direction 2"), "eleqsurf3": ("m3/day", "surface flow: direction 3"),
    "rivqdown": ("m3/day", "river downstream discharge"), "rivqup": ("m3/day", "river upstream discharge"),
    "rivqsurf": ("m3/day", "river surface discharge"), "rivqsub": ("m3/day", "river subsurface discharge"),
    "rivystage": ("m", "river stage"), "lakystage": ("m", "lake stage"), "lakatop": ("m2", "lake top area"),
    "lakvevap": ("m/day", "lake evaporation"), "lakvprcp": ("m/day", "lake precipitation"),
    "lakqrivin": ("m3/day", "lake river inflow"), "lakqrivout": ("m3/day", "lake river outflow"),
    "lakqsurf": ("m3/day", "lake surface discharge"), "lakqsub": ("m3/day", "lake subsurface discharge"),
    "rn_h": ("W m-2", "shortwave radiation on horizontal surface"),
    "rn_t": ("W m-2", "terrain-corrected shortwave radiation"),
    "rn_factor": ("1", "terrain radiation correction factor"),
}
KIND = {"ele": ("mesh_face", "element", ".ele.nc"), "riv": ("river", "river", ".riv.nc"),
        "lake": ("lake", "lake", ".lake.nc")}


def _pad(b):
    return b + b"\0" * (-len(b) % 4)


def _name(s):
    b = s.encode()
    return struct.pack(">i", len(b)) + _pad(b)


def _atts(atts):
    if not atts:
        return struct.pack(">ii", 0, 0)
    out = struct.pack(">ii", NC_ATTRIBUTE, len(atts))
    for k, v in atts:
        out += _name(k)
        if isinstance(v, str):
            b = v.encode()
            out += struct.pack(">ii", NC_CHAR, len(b)) + _pad(b)
        elif isinstance(v, (np.float32, float)):
            out += struct.pack(">iif", NC_FLOAT, 1, v)
        else:
            out += struct.pack(">iii", NC_INT, 1, int(v))
    return out


def split_basename(basename):
    leaf = basename.replace("\\", "/").rsplit("/", 1)[-1]
    prefix, _, var = leaf.rpartition(".")
    return prefix, var


def variables(kind, n_all, names, num_node=0, crs_wkt="", forc_start=20000101):
    """[(name, dimids, atts, type, is_record, vsize)] in definition order, and the dimension list"""
    dim, obj, _ = KIND[kind]
    ymd = int(forc_start)
    iso = "%04d-%02d-%02d" % (ymd // 10000, ymd // 100 % 100, ymd % 100)
    dims = [("time", 0), (dim, n_all)]
    v = [("time", [0], [("units", f"minutes since {iso} 00:00:00 UTC"), ("calendar", "standard")], NC_DOUBLE, True, 8)]
    crs = kind == "ele" and bool(crs_wkt)
    if kind == "ele":
        dims += [("mesh_node", num_node), ("max_face_nodes", 3)]
        xa = [("standard_name", "projection_x_coordinate"), ("units", "m")]
        ya = [("standard_name", "projection_y_coordinate"), ("units", "m")]
        v += [("mesh_node_x", [2], xa, NC_DOUBLE, False, 8 * num_node),
              ("mesh_node_y", [2], ya, NC_DOUBLE, False, 8 * num_node),
              ("mesh_face_nodes", [1, 3], [("start_index", 1)], NC_INT, False, 12 * n_all),
              ("mesh_face_x", [1], xa, NC_DOUBLE, False, 8 * n_all),
              ("mesh_face_y", [1], ya, NC_DOUBLE, False, 8 * n_all)]
        if crs:
            v.append(("crs", [], [("long_name", "coordinate reference system"), ("spatial_ref", crs_wkt),
                                  ("crs_wkt", crs_wkt)], NC_INT, False, 4))
        v.append(("mesh", [], [("cf_role", "mesh_topology"), ("topology_dimension", 2),
                               ("node_coordinates", "mesh_node_x mesh_node_y"),
                               ("face_node_connectivity", "mesh_face_nodes"),
                               ("face_coordinates", "mesh_face_x mesh_face_y")], NC_INT, False, 4))
    v += [(f"{obj}_id", [1], [("start_index", 1)], NC_INT, False, 4 * n_all),
          (f"{obj}_output_mask", [1], [], NC_INT, False, 4 * n_all)]
    for nm in names:
        a = [("_FillValue", FILL)]
        if kind == "ele":
            a += [("mesh", "mesh"), ("location", "face"), ("coordinates", "mesh_face_x mesh_face_y")]
            if crs:
                a.append(("grid_mapping", "crs"))
        if nm in META:
            a += [("long_name", META[nm][1]), ("units", META[nm][0])]
        else:
            a.append(("long_name", "SHUD output variable: " + nm))
        v.append((nm, [0, 1], a, NC_FLOAT, True, 4 * n_all))
    return dims, v


def build(kind, n_all, ctrls, puts, history, mesh=None, crs_wkt="", forc_start=20000101):
    """ctrls: [(basename, icol 1-based list)] in registration order; puts: [(ctrl index, t_quantized, selected doubles)]
    in call order; mesh: dict(node_x, node_y, face_nodes [n,3] 1-based, face_x, face_y) for kind "ele"."""
    prefix = split_basename(ctrls[0][0])[0]
    names = []
    for bn, _ in ctrls:
        nm = split_basename(bn)[1]
        if nm not in names:
            names.append(nm)
    num_node = 0 if mesh is None else len(mesh["node_x"])
    dims, var = variables(kind, n_all, names, num_node, crs_wkt, forc_start)
    gatts = [("Conventions", "CF-1.10 UGRID-1.0" if kind == "ele" else "CF-1.10"), ("title", "SHUD output: " + prefix),
             ("source", "SHUD"), ("history", history)]
    # records: one per distinct llround(t), in order of first appearance
    times = []
    for _, t, _ in puts:
        tm = int(np.floor(abs(t) + 0.5) * np.sign(t)) if t != 0 else 0       # llround: halves away from zero
        if tm not in times:
            times.append(tm)

    def header(begins):
        h = b"CDF\x02" + struct.pack(">i", len(times))
        h += struct.pack(">ii", NC_DIMENSION, len(dims)) + b"".join(_name(d) + struct.pack(">i", n) for d, n in dims)
        h += _atts(gatts)
        h += struct.pack(">ii", NC_VARIABLE, len(var))
        for (nm, dd, aa, ty, _, vs), bg in zip(var, begins):
            h += _name(nm) + struct.pack(">i", len(dd)) + b"".join(struct.pack(">i", d) for d in dd)
            h += _atts(aa) + struct.pack(">iiq", ty, vs, bg)
        return h

    off = len(header([0] * len(var)))
    begins = [0] * len(var)
    for k, x in enumerate(var):
        if not x[4]:
            begins[k] = off
            off += x[5]
    rec_begin = off
    for k, x in enumerate(var):
        if x[4]:
            begins[k] = off
            off += x[5]
    out = header(begins)
    mask = np.zeros(n_all, dtype=">i4")
    for c in ctrls[0][1]:
        if 1 <= c <= n_all:
            mask[c - 1] = 1
    if kind == "ele":
        out += np.asarray(mesh["node_x"], dtype=">f8").tobytes() + np.asarray(mesh["node_y"], dtype=">f8").tobytes()
        out += np.asarray(mesh["face_nodes"], dtype=">i4").reshape(-1).tobytes()
        out += np.asarray(mesh["face_x"], dtype=">f8").tobytes() + np.asarray(mesh["face_y"], dtype=">f8").tobytes()
        out += struct.pack(">i", FILL_INT) * (2 if crs_wkt else 1)
    out += np.arange(1, n_all + 1, dtype=">i4").tobytes() + mask.tobytes()
    assert len(out) == rec_begin
    slabs = np.full((len(times), len(names), n_all), FILL, dtype=">f4")
    for ci, t, sel in puts:
        bn, icol = ctrls[ci]
        tm = int(np.floor(abs(t) + 0.5) * np.sign(t)) if t != 0 else 0
        with np.errstate(over="ignore"):
            vals = np.asarray(sel, dtype=np.float64).astype(">f4")
        row = slabs[times.index(tm), names.index(split_basename(bn)[1])]
        for j in range(min(len(vals), len(icol))):
            if 1 <= icol[j] <= n_all:
                row[icol[j] - 1] = vals[j]
    for r, tm in enumerate(times):
        out += struct.pack(">d", float(tm)) + slabs[r].tobytes()
    return out
