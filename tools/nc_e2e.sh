#!/bin/bash
# GPU box: OUTPUT_MODE LEGACY / NETCDF / BOTH end to end through shud_gpu on a synthetic project (NE elements, one
# simulated day, hourly forcing, hourly outputs: the set-up of DESIGN.md §5f), then the NetCDF conversion kernels against
# the STREAM copy (tools/nc_bench.py).  LEGACY runs alternate between this tree's shud_gpu and a baseline build of it
# (BASE=path/to/shud_gpu, e.g. the parent commit's; skipped when unset) in ABBA order, with a sync before every run.
# usage: [BASE=...] bash tools/nc_e2e.sh [NE] [OUTDIR]        logs: OUTDIR/<label>.log, OUTDIR/nc_bench.jsonl
set -o pipefail
cd "$(dirname "$0")/.."
NE=${1:-1000000}
OUT=${2:-$PWD/out/nc_measure}
mkdir -p "$OUT"
D=${TMPDIR:-/tmp}/shud_nc_e2e_$NE
rm -rf "$D"
timeout -k 10 400 python3 -c "
import sys; sys.path.insert(0, 'shud-up_amd')
from shud_rhs import synth
synth.write_project('$D/input/syn', 'syn', $NE, days=1.0)
print('project written', flush=True)" || exit 1
IN=$D/input/syn
cp $IN/syn.cfg.para $D/para.base
echo "OUT_DIR ncout" > $IN/syn.cfg.ncoutput
run() {   # label binary mode
    local label=$1 bin=$2 mode=$3
    cp $D/para.base $IN/syn.cfg.para
    if [ "$mode" != LEGACY ]; then printf 'OUTPUT_MODE\t%s\nNCOUTPUT_CFG\tsyn.cfg.ncoutput\n' $mode >> $IN/syn.cfg.para; fi
    rm -rf $D/out $D/ncout
    sync
    SHUD_NC_HISTORY=bench timeout -k 10 240 $bin -o $D/out -C $IN $IN syn > "$OUT/$label.log" 2>&1
    local rc=$?
    tail -1 "$OUT/$label.log"
    { echo "# files:"; (cd $D && du -sb out ncout 2>/dev/null); } >> "$OUT/$label.log"
    return $rc
}
T=shud-up_amd/shud_gpu
if [ -n "$BASE" ]; then
    run legacy_tree_1 $T LEGACY && run legacy_parent_1 $BASE LEGACY && run legacy_parent_2 $BASE LEGACY && \
    run legacy_tree_2 $T LEGACY && run legacy_tree_3 $T LEGACY && run legacy_parent_3 $BASE LEGACY && \
    run legacy_parent_4 $BASE LEGACY && run legacy_tree_4 $T LEGACY || { echo "a run failed: stopping"; rm -rf "$D"; exit 1; }
else
    run legacy_tree_1 $T LEGACY && run legacy_tree_2 $T LEGACY || { echo "a run failed: stopping"; rm -rf "$D"; exit 1; }
fi
run netcdf_1 $T NETCDF && run both_1 $T BOTH && run netcdf_2 $T NETCDF && run both_2 $T BOTH || \
    { echo "a run failed: stopping"; rm -rf "$D"; exit 1; }
# the last BOTH run: the NetCDF file reads back and holds float32 of the .dat rows
timeout -k 10 120 python3 -c "
import sys, numpy as np; sys.path.insert(0, 'shud-up_amd')
from scipy.io import netcdf_file
from shud_rhs import shudio
d = shudio.read_dat('$D/out/syn.eleygw.dat')
with netcdf_file('$D/ncout/syn.ele.nc', 'r', mmap=False) as f:
    v = f.variables['eleygw']
    ok = all(np.array_equal(np.array(v[r]).astype(np.float32), d['data'][r].astype(np.float32)) for r in (0, 11, 23))
    print('records', f._recs, 'eleygw rows 0/11/23 equal float32(.dat):', ok, 'version', f.version_byte)
" 2>&1 | tee "$OUT/readback.log"
rm -rf "$D"
timeout -k 10 300 python3 tools/nc_bench.py --out "$OUT/nc_bench.jsonl" 2>&1 | tail -4
