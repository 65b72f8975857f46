"""The element kernel's load order (shud_ele_packed.hip): an element's first river segment is
loaded under the vertical physics and the rest in a two-step loop, a reach's stage is loaded before its BC flag is
known, and the two straight-line edge stages load ahead of the barrier in front of them.  None of it may change a bit:
0 to 7 segments per element (heihe, qhh with its lake instantiation, ccw), stage BCs on first and later segments, no
segment arrays at all, tiles that end in idle waves and partial tiles, and the folded partition launch with a ghost
reach under a boundary element."""
import numpy as np
import pytest

import cases
from conftest import assert_close
from shud_rhs import abi, partition, synth, workload

pytestmark = pytest.mark.gpu

SEG_DIAG = ("qseg_surf", "qseg_sub")        # per-segment fluxes in reference segment order (read back from qseg2)


def _rt():
    from shud_rhs import runtime
    return runtime


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape, what
    bad = np.nonzero(a.view(np.uint64) != b.view(np.uint64))[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"


def _segs_per_element(m):
    return np.bincount(np.asarray(m.seg_ele, np.int64), minlength=m.num_ele)


def _check(m, ys, mode, oracle_mod, monkeypatch, label, soa=True, ncalls=2):
    """packed against the oracle (conftest tolerance) and, bit for bit, against the SoA kernel: DY of `ncalls`
    stateful evals per state, then the per-segment diagnostics"""
    rt = _rt()
    monkeypatch.setenv("SHUD_RHS_PACKED", "1")
    g = rt.RhsHandle(m, mode=mode)
    assert g.layout()["packed"], g.layout()
    s = None
    if soa:
        monkeypatch.setenv("SHUD_RHS_PACKED", "0")
        s = rt.RhsHandle(m, mode=mode)
        assert not s.layout()["packed"], s.layout()
    monkeypatch.delenv("SHUD_RHS_PACKED")
    o = oracle_mod.OracleRhs(m, mode)
    for h in (g, s, o):
        if h is not None:
            h.set_step_inputs()
    try:
        for si, y in enumerate(ys):
            for c in range(ncalls):
                ref, code, _, _ = o.eval(0.0, y)
                assert code == 0, f"{label}: oracle exit {code}"
                got = g.eval(0.0, y)
                assert_close(got, ref, what=f"{label} state {si} call {c}")
                if s is not None:
                    _same_bits(got, s.eval(0.0, y), f"{label} packed vs SoA, state {si} call {c}")
        if m.num_riv:
            dg, do = g.diagnostics(), o.diagnostics()
            ds = s.diagnostics() if s is not None else None
            for k in SEG_DIAG:
                assert dg[k].size == len(m.seg_ele)
                assert_close(dg[k], do[k], what=f"{label} diag {k}")
                if ds is not None:
                    _same_bits(dg[k], ds[k], f"{label} diag {k} packed vs SoA")
    finally:
        g.close()
        if s is not None:
            s.close()


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
@pytest.mark.parametrize("name", ["heihe", "qhh", "ccw"])
def test_segments_per_element(name, mode, oracle_mod, monkeypatch):
    """heihe and qhh hold 0 to 7 segments per element, qhh takes the lake instantiation (serial semantics and the
    packed layout only: the handle rejects lakes otherwise), ccw the plain sharing one"""
    m, y0 = getattr(cases, name)()
    lake = getattr(m, "num_lake", 0) > 0
    if lake and mode == abi.SHUD_MODE_OMP:
        with pytest.raises(_rt().ShudRhsError):
            _rt().RhsHandle(m, mode=mode)
        return
    n = _segs_per_element(m)
    if name != "ccw":
        assert n.min() == 0 and n.max() >= 5, (n.min(), n.max())
    _check(m, cases.states(m, None, 2, seed=300), mode, oracle_mod, monkeypatch, name, soa=not lake, ncalls=3)


def _bc_reaches(m, seed=3):
    """a seeded choice of reaches: one that owns the first segment of an element with >= 3 segments, one that owns
    a later segment of such an element, and a few more"""
    se, sr = np.asarray(m.seg_ele, np.int64), np.asarray(m.seg_riv, np.int64)
    n = _segs_per_element(m)
    rng = np.random.default_rng(seed)
    big = rng.permutation(np.nonzero(n >= 3)[0])
    assert big.size >= 2
    first_of = lambda e: int(np.nonzero(se == e)[0][0])          # noqa: E731  ascending reference segment index
    e1 = int(big[0])
    r_first = int(sr[first_of(e1)])
    r_later = None
    for e in big[1:]:
        ks = np.nonzero(se == e)[0]
        if sr[ks[0]] == r_first:
            continue
        later = [int(sr[k]) for k in ks[1:] if sr[k] != sr[ks[0]] and sr[k] != r_first]
        if later:
            r_later, e2 = later[0], int(e)
            break
    assert r_later is not None, "no element with >= 3 segments on two reaches"
    others = [int(r) for r in rng.choice(m.num_riv, 6, replace=False) if sr[first_of(e2)] != r]
    return sorted({r_first, r_later, *others}), e1, e2


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
def test_reach_bc_on_peeled_and_loop_segments(mode, oracle_mod, monkeypatch):
    """stage BCs (riv_bc = 1, the stage from riv_ybc) on a reach under an element's first segment and on one under a
    later segment only: the stage loaded from y must be replaced by the BC value on both paths"""
    m, _ = cases.heihe()
    reaches, e1, e2 = _bc_reaches(m)
    rbc = np.zeros(m.num_riv, dtype=np.int32)
    rbc[reaches] = 1
    m.riv_bc = rbc
    m.bc_tables = dict(ele_ybc=np.array([0.0, 12.5, 25.0]), ele_qbc=np.array([0.0, -3.0, 5.0, 0.25]),
                       riv_ybc=np.array([0.0, 0.8]), riv_qbc=np.array([0.0, 2.0, -1.5]))
    m.finalize()
    se, sr = np.asarray(m.seg_ele, np.int64), np.asarray(m.seg_riv, np.int64)
    n = _segs_per_element(m)
    k1, k2 = np.nonzero(se == e1)[0], np.nonzero(se == e2)[0]
    assert n[e1] >= 3 and m.riv_bc[sr[k1[0]]] == 1                       # a BC reach owns a first segment
    assert n[e2] >= 3 and m.riv_bc[sr[k2[0]]] == 0 and (m.riv_bc[sr[k2[1:]]] == 1).any()   # and a later one only
    _check(m, cases.states(m, None, 2, seed=310), mode, oracle_mod, monkeypatch, "heihe reach BC")


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
def test_variant_branches_segchain(mode, oracle_mod, monkeypatch):
    """cases.variant(): the fu != 1 instantiation, open boundary, element and reach BCs"""
    m, y = cases.variant()
    assert (m.riv_bc > 0).any() and m.close_boundary == 0
    _check(m, [y, workload.random_state(m, seed=320)], mode, oracle_mod, monkeypatch, "variant")


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
@pytest.mark.parametrize("case", ["riverless", "single_element"])
def test_no_segments_anywhere(case, mode, oracle_mod, monkeypatch):
    """no river network: the model has no segment arrays, so no lane may issue a segment load"""
    m, y = getattr(cases, case)()
    assert m.num_riv == 0 and len(m.seg_ele) == 0
    _check(m, [y] + cases.states(m, None, 1, seed=330), mode, oracle_mod, monkeypatch, case)


@pytest.fixture(scope="module")
def tile_mesh():
    m = synth.synth_model(2000, seed=47)
    m.step = workload.random_step_inputs(m, seed=9)
    return m


@pytest.mark.parametrize("ne", [1, 63, 65, 255, 257])
def test_tile_ends_share_on_off(ne, tile_mesh, oracle_mod, monkeypatch):
    """the first `ne` elements of a synthetic mesh: waves that are idle or partly active and a partial second tile
    meet the edge loads now issued ahead of the sharing barriers.  Sharing on against off bit for bit, both modes,
    and against the oracle"""
    rt = _rt()
    m = cases._subset(tile_mesh, np.arange(ne))
    assert m.num_ele == ne
    ys = cases.states(m, None, 2, seed=340 + ne)
    for mode in (abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP):
        monkeypatch.setenv("SHUD_RHS_SHARE", "1")
        a = rt.RhsHandle(m, mode=mode)
        monkeypatch.setenv("SHUD_RHS_SHARE", "0")
        b = rt.RhsHandle(m, mode=mode)
        monkeypatch.delenv("SHUD_RHS_SHARE")
        o = oracle_mod.OracleRhs(m, mode)
        try:
            assert a.layout()["packed"] and b.layout()["packed"] and "shared_edges" not in b.layout()
            if ne >= 63:
                assert a.layout().get("shared_edges", 0) > 0, a.layout()
            for h in (a, b, o):
                h.set_step_inputs()
            for si, y in enumerate(ys):
                for c in range(2):
                    ga, gb = a.eval(0.0, y), b.eval(0.0, y)
                    _same_bits(ga, gb, f"NE={ne} mode {mode} state {si} call {c}")
                    assert_close(ga, o.eval(0.0, y)[0], what=f"NE={ne} mode {mode} state {si} call {c}")
        finally:
            a.close()
            b.close()


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
def test_partition_fold_ghost_reach(mode, monkeypatch):
    """a 2-way split of heihe on one GPU through the folded launch: owned DY bit for bit against the single handle.
    A boundary element of the split owns a segment on a ghost reach, whose stage arrives with the halo"""
    import test_gpu_partition as tp
    monkeypatch.setenv("SHUD_RHS_FOLD", "1")
    m, _ = cases.heihe()
    ep, _ = partition.cpp_partition(m, 2, partition.PART_AUTO)
    locs = [partition.CppPlan(m, ep, 2, r).local_model() for r in range(2)]
    ghost_seg = 0
    for lm, part in locs:
        se, sr = np.asarray(lm.seg_ele, np.int64), np.asarray(lm.seg_riv, np.int64)
        ghost_seg += int(((se < part.n_own_ele) & (sr >= part.n_own_riv)).sum())
    assert ghost_seg > 0, "no owned element with a segment on a ghost reach"
    tp._run_ranks(m, cases.states(m, None, 2, seed=350), locs, mode, ncalls=2, device_eval=True)
