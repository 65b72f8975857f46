"""Shared by the GPU tests that start the C++ host driver shud-up_amd/shud_gpu.  Not a test module."""
import json
import os
import subprocess

from conftest import PKG_DIR

SHUD_GPU = os.path.join(PKG_DIR, "shud_gpu")


def run(args, env=None, check=True):
    """shud_gpu with `args` -> CompletedProcess (text).  env: changes to this process's environment, a value of None
    removes the variable.  check: the run must exit with 0."""
    e = dict(os.environ)
    for k, v in (env or {}).items():
        e.pop(k, None)
        if v is not None:
            e[k] = v
    r = subprocess.run([SHUD_GPU] + [str(a) for a in args], capture_output=True, text=True, timeout=240, env=e)
    if check:
        assert r.returncode == 0, r.stdout + r.stderr
    return r


def json_line(r, key="shud_gpu"):
    """the last machine-readable line of the run's stdout that opens with `key`, parsed"""
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('{"%s"' % key)]
    assert line, r.stdout + r.stderr
    return json.loads(line[-1])[key]
