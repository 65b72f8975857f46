"""CPU: the checkpoint container (include/shud_ckpt.h, csrc/shud_ckpt_fmt.cpp) through ctypes, no device —
write/read round trips, the checksums against a numpy uint64 restatement, and every kind of damaged file refused."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from shud_rhs import abi, runtime

LIB = os.path.join(ROOT, "shud-up_amd", "libshud_rhs.so")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "shud-up_amd"), "libshud_rhs.so"])
    return runtime.lib()


def np_checksum(w):
    """c0 = sum w_i, c1 = sum (i + 1) w_i, mod 2^64 (numpy uint64 arithmetic wraps)"""
    w = np.asarray(w, dtype=np.uint64)
    with np.errstate(over="ignore"):
        i1 = np.arange(1, w.size + 1, dtype=np.uint64)
        return int(w.sum(dtype=np.uint64)), int((i1 * w).sum(dtype=np.uint64))


def sections(seed=5):
    rng = np.random.default_rng(seed)
    words = [0, 1, 7, 0, 1025, 2]                       # zero-length, 1-word and odd-length sections
    names = [f"sec.{k}" for k in range(len(words))]
    data = [rng.integers(0, 2**64, size=n, dtype=np.uint64) for n in words]
    return names, data


def write(lib, path, names, data, **hdr):
    info = abi.ShudCkptInfo()
    for k, v in hdr.items():
        setattr(info, k, v)
    n = len(names)
    c_names = (C.c_char_p * n)(*[s.encode() for s in names])
    c_data = (C.c_void_p * n)(*[d.ctypes.data if d.size else None for d in data])
    c_words = (C.c_uint64 * n)(*[d.size for d in data])
    rc = lib.shud_ckpt_write_sections(str(path).encode(), C.byref(info), n, c_names, c_data, c_words)
    assert rc == abi.SHUD_OK, lib.shud_rhs_last_error_string()


def read(lib, path, name, cap=4096):
    out = np.zeros(cap, dtype=np.uint64)
    n = C.c_uint64()
    rc = lib.shud_ckpt_read_section(str(path).encode(), name.encode(), out.ctypes.data_as(abi.c_uint64_p), cap,
                                    C.byref(n))
    return rc, out[:n.value]


def last_error(lib):
    return lib.shud_rhs_last_error_string().decode()


def test_checksum_equals_numpy_restatement(lib):
    rng = np.random.default_rng(1)
    for n in (0, 1, 2, 255, 1025, 70001):
        w = rng.integers(0, 2**64, size=n, dtype=np.uint64)
        if n > 3:
            w[:3] = [2**64 - 1, 0, 2**63]                # all-ones, zero and the sign bit
        c0, c1 = C.c_uint64(), C.c_uint64()
        lib.shud_ckpt_checksum(w.ctypes.data_as(abi.c_uint64_p), n, C.byref(c0), C.byref(c1))
        assert (c0.value, c1.value) == np_checksum(w), n


def test_round_trip_and_info(lib, tmp_path):
    names, data = sections()
    p = tmp_path / "a.ckpt"
    write(lib, p, names, data, ne=1147, nr=103, ns=77, nl=2, ny=3546, mode=1, layout=abi.SHUD_CKPT_LAYOUT_HYBRID,
          n_classes=9, n_streamed=2, n_shared=31, order_kind=3, t=1234.5, step=41, ode_reltol=1e-4, ode_maxl=5,
          statics_c0=0xDEADBEEF, perm_c1=7, abi_version=2)
    for nm, d in zip(names, data):
        rc, got = read(lib, p, nm)
        assert rc == abi.SHUD_OK and got.tobytes() == d.tobytes(), nm
    info = runtime.Checkpoint.info(p)
    assert info["magic"] == abi.SHUD_CKPT_MAGIC and info["version"] == abi.SHUD_CKPT_VERSION
    assert (info["ne"], info["nr"], info["ns"], info["nl"], info["ny"]) == (1147, 103, 77, 2, 3546)
    assert (info["mode"], info["layout"], info["n_classes"], info["n_streamed"], info["n_shared"]) == (1, 2, 9, 2, 31)
    assert (info["order_kind"], info["t"], info["step"], info["ode_reltol"], info["ode_maxl"]) == (3, 1234.5, 41, 1e-4, 5)
    assert info["statics_c0"] == 0xDEADBEEF and info["perm_c1"] == 7 and info["abi_version"] == 2
    assert info["n_sections"] == len(names) and info["payload_words"] == sum(d.size for d in data)
    off = 0
    for (nm, o, w, c0, c1), want, d in zip(info["sections"], names, data):
        assert (nm, o, w) == (want, off, d.size)
        assert (c0, c1) == np_checksum(d)
        off += d.size
    runtime.Checkpoint.verify(p)
    assert os.path.getsize(p) == info["header_bytes"] + 8 * info["payload_words"]
    assert not os.path.exists(str(p) + ".tmp")


def test_flipped_payload_byte_names_the_section(lib, tmp_path):
    names, data = sections()
    p = tmp_path / "a.ckpt"
    write(lib, p, names, data)
    info = runtime.Checkpoint.info(p)
    raw = bytearray(open(p, "rb").read())
    sec = info["sections"][4]                            # sec.4, 1025 words
    raw[info["header_bytes"] + 8 * sec[1] + 8 * 500 + 3] ^= 0x10
    open(p, "wb").write(raw)
    assert lib.shud_ckpt_verify(str(p).encode()) == abi.SHUD_ERR_ARG
    assert "sec.4" in last_error(lib) and "checksum" in last_error(lib)
    runtime.Checkpoint.info(p)                           # the header itself is intact
    rc, _ = read(lib, p, "sec.2")
    assert rc == abi.SHUD_ERR_ARG


@pytest.mark.parametrize("damage", ["header_byte", "table_byte", "truncated", "truncated_header", "magic", "version"])
def test_damaged_files_are_refused(lib, tmp_path, damage):
    names, data = sections()
    p = tmp_path / "a.ckpt"
    write(lib, p, names, data, t=3.0)
    raw = bytearray(open(p, "rb").read())
    if damage == "header_byte":
        raw[abi.ShudCkptInfo.t.offset + 2] ^= 1
        want = "header checksum"
    elif damage == "table_byte":
        raw[C.sizeof(abi.ShudCkptInfo) + C.sizeof(abi.ShudCkptSection) + 30] ^= 1
        want = "header checksum"
    elif damage == "truncated":
        raw = raw[:-9]
        want = "truncated"
    elif damage == "truncated_header":
        raw = raw[:100]
        want = "truncated header"
    elif damage == "magic":
        raw[0] ^= 0x20
        want = "magic"
    else:
        raw[8:12] = (abi.SHUD_CKPT_VERSION + 1).to_bytes(4, "little")
        want = "version"
    open(p, "wb").write(raw)
    info = abi.ShudCkptInfo()
    for rc in (lib.shud_ckpt_info(str(p).encode(), C.byref(info)), lib.shud_ckpt_verify(str(p).encode())):
        assert rc == abi.SHUD_ERR_ARG
        assert want in last_error(lib), last_error(lib)


def test_leftover_tmp_is_ignored_and_replaced(lib, tmp_path):
    names, data = sections()
    p = tmp_path / "a.ckpt"
    write(lib, p, names, data, step=1)
    open(str(p) + ".tmp", "wb").write(b"half a checkpoint of a killed run")
    runtime.Checkpoint.verify(p)
    assert runtime.Checkpoint.info(p)["step"] == 1
    write(lib, p, names, data, step=2)                   # the next write goes through the same .tmp and replaces it
    assert runtime.Checkpoint.info(p)["step"] == 2 and not os.path.exists(str(p) + ".tmp")


def test_missing_section_and_short_buffer(lib, tmp_path):
    names, data = sections()
    p = tmp_path / "a.ckpt"
    write(lib, p, names, data)
    rc, _ = read(lib, p, "nope")
    assert rc == abi.SHUD_ERR_ARG and "nope" in last_error(lib)
    rc, _ = read(lib, p, "sec.4", cap=10)
    assert rc == abi.SHUD_ERR_ARG
    assert lib.shud_ckpt_verify(str(tmp_path / "absent").encode()) == abi.SHUD_ERR_ARG


def test_header_functions_exported_and_mirrored(lib):
    """every function of include/shud_ckpt.h is exported and bound in abi.py, and the new resume entries of
    shud_out.h / shud_mon.h are; the struct mirrors match the C layout (tests/test_abi.py's manner)"""
    txt = open(os.path.join(ROOT, "include", "shud_ckpt.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set(re.findall(r"\b(shud_ckpt_\w+)\s*\(", txt))
    assert len(names) >= 10
    assert names == set(abi.CKPT_FUNCTIONS), names ^ set(abi.CKPT_FUNCTIONS)
    raw = C.CDLL(LIB)
    for n in sorted(names) + ["shud_out_resume", "shud_mon_resume"]:
        assert hasattr(raw, n), n
    assert "shud_out_resume" in abi.OUT_FUNCTIONS and "shud_mon_resume" in abi.MON_FUNCTIONS
    for name, cls in (("ShudCkptInfo", abi.ShudCkptInfo), ("ShudCkptSection", abi.ShudCkptSection),
                      ("ShudCkptParts", abi.ShudCkptParts)):
        src = f'#include "shud_ckpt.h"\n#include <stdio.h>\nint main(){{printf("%zu\\n", sizeof({name}));return 0;}}\n'
        exe = f"/tmp/sz_{name}_{os.getpid()}"
        subprocess.run(["gcc", "-x", "c", "-", "-I", os.path.join(ROOT, "include"), "-o", exe], input=src.encode(),
                       check=True)
        out = int(subprocess.check_output([exe]).decode().strip())
        os.unlink(exe)
        assert out == C.sizeof(cls), (name, out, C.sizeof(cls))
