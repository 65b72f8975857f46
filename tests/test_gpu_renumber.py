"""GPU: the RHS must not depend on how the mesh is numbered (tests/renumber.py).

Every other GPU test runs meshes whose numbering has one shape: elements in grid rows (or the reference's own
order), segments sorted by reach.  The host tables that follow from the numbering (the in-tile edge-sharing
assignment, neighbour gathers, the element-sorted and reach-sorted segment streams, the junction lists) are run here
on renumbered models:
 a. elements renumbered only: DY and every diagnostic are the permuted ones of the original model, bit for bit, in
    every device layout (test_renumber.py shows the same of the oracle);
 b. elements, reaches, segments and edge slots all renumbered: parity with the oracle at the project's tolerance;
 c. in-tile edge sharing under tile-local numberings that reach every sharing state (test_renumber.py asserts that
    they do): sharing on vs off bit for bit, and against the oracle;
 d. partitioned handles of a fully renumbered mesh: bit-identical to one GPU.
And shud_rhs_create with depression = NULL (the default 0.0002 everywhere) while sharing is on."""
import copy

import numpy as np
import pytest

import cases
import renumber as rn
import test_gpu_parity as tp
import test_gpu_partition as tpart
import test_gpu_share as ts
from conftest import assert_close
from shud_rhs import abi, partition, workload

pytestmark = pytest.mark.gpu

MODES = [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP]
layout = tp.layout      # the packed / SoA fixture of the parity tests
OMP_SKIPPED = ("q_es", "q_eu", "q_eg", "q_tu", "q_tg", "q_eta", "i_beta")       # as tp._compare_sequence


# ---------------------------------------------------------------- a. numbering invariance, bit for bit
_layout_model = cases.layout_model


def _gpu_sequence(m, ys, mode, check, ncalls=2):
    """every DY of a stateful sequence, the diagnostics after it, and the handle's layout"""
    g = tp._runtime().RhsHandle(m, mode=mode)
    try:
        lay = g.layout()
        assert check(lay), lay
        plan = tp._runtime().plan_layout(m, mode=mode)      # the host tables alone say the same
        assert {k: v for k, v in plan.items() if k not in ("n_int", "riv_sb")} == lay, (plan, lay)
        g.set_step_inputs()
        seq = [g.eval(0.0, y) for y in ys for _ in range(ncalls)]       # raises on an error exit
        return seq, g.diagnostics(), lay
    finally:
        g.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["packed_share", "mid_class", "hybrid4", "big_table", "l2", "soa"])
def test_element_numbering_invariance(kind, mode, monkeypatch):
    """gpu(m2)(map_y(y)) == map_y(gpu(m)(y)) word for word for m2 = m with its elements block-shuffled, randomly
    permuted, or rolled by 101: DY over 3 states x 2 stateful calls and every diagnostic, in each device layout.
    With sharing, the host's count of shared edges is that of the restated rule for each numbering."""
    m, y, check = _layout_model(kind, monkeypatch)
    NE = m.num_ele
    ys = [y] + cases.states(m, None, 2, seed=61)
    ref_seq, ref_dg, ref_lay = _gpu_sequence(m, ys, mode, check)
    if kind == "packed_share":
        assert ref_lay["shared_edges"] == int((rn.share_assignment(m)[1] >= 0).sum())
    rng = np.random.default_rng(17)
    for name, pe in (("block_shuffle", rn.block_shuffle(NE, rng)), ("random_perm", rn.random_perm(NE, rng)),
                     ("roll", rn.roll(NE, 101))):
        m2, map_y = rn.renumber(m, pe=pe)
        nb = map_y.__self__
        seq, dg, lay = _gpu_sequence(m2, [map_y(v) for v in ys], mode, check)
        assert {k: v for k, v in lay.items() if k != "shared_edges"} == \
               {k: v for k, v in ref_lay.items() if k != "shared_edges"}, (lay, ref_lay)
        if kind == "packed_share":
            assert lay["shared_edges"] == int((rn.share_assignment(m2)[1] >= 0).sum()), (name, lay)
        for c, (a, b) in enumerate(zip(ref_seq, seq)):
            ts._same_bits(map_y(a), b, f"{kind} {name} mode {mode} eval {c}")
        for k in abi.FLUXOUT_ORDER:
            if mode == abi.SHUD_MODE_OMP and k in OMP_SKIPPED:
                continue
            ts._same_bits(ref_dg[k], nb.unmap_diag(k, dg[k]), f"{kind} {name} mode {mode} diag {k}")


# ---------------------------------------------------------------- b. full renumbering against the oracle
def _nup(m):
    d = m.riv_down
    return np.bincount(d[d >= 0], minlength=m.num_riv)


def _full(name):
    """-> (fully renumbered model, states in its numbering)"""
    if name == "junctions":
        m, _ = tp._junction_model()
        m.step = workload.random_step_inputs(m, seed=777)
        y = workload.random_state(m, seed=21)
    elif name == "variant3000":
        m, y = cases.variant(3000, seed=5)
    else:
        m, y = getattr(cases, name)()
    m2, map_y = rn.renumber(m, **rn.full_numbering(m, np.random.default_rng(23)))
    assert m.num_seg == 0 or ((np.diff(m2.seg_riv) < 0).any() and (np.diff(m2.seg_ele) < 0).any())
    if name == "junctions":
        assert {0, 1, 2, 3, 5, 14} <= set(_nup(m2).tolist()), sorted(set(_nup(m2).tolist()))
        assert sorted(_nup(m2).tolist()) == sorted(_nup(m).tolist())
        big = int(np.argmax(_nup(m2)))
        ups = np.nonzero(m2.riv_down == big)[0]
        assert ups.size == 14 and (np.diff(ups) > 1).any()                # upstream ids no longer a band
    if name.startswith("qhh"):
        ys = [map_y(y), workload.random_state(m2, seed=31)]
        ys[1][-1] = 300.0                                                  # lake above its banks, as tp.test_lakes
    else:
        ys = [map_y(y)] + cases.states(m2, None, 2, seed=67)
    return m2, ys


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["ccw", "heihe", "variant3000", "junctions"])
def test_full_renumbering_oracle(name, mode, oracle_mod, layout):
    """pe, rot, pr, ps all drawn: segments sorted neither by reach nor by element, upstream reaches of a junction at
    random ids, neighbours anywhere; DY over 3 states x 2 stateful calls and every diagnostic against the oracle"""
    m2, ys = _full(name)
    tp._compare_sequence(m2, ys, mode, oracle_mod, ncalls=2, label=f"renumbered {name}", layout=layout)


@pytest.mark.parametrize("name", ["qhh", "qhh_variant"])
def test_full_renumbering_lakes(name, oracle_mod):
    """lakes (serial, packed only); the lake sums run in element order, so only parity holds here, not invariance"""
    m2, ys = _full(name)
    tp._compare_sequence(m2, ys, abi.SHUD_MODE_SERIAL, oracle_mod, ncalls=2, label=f"renumbered {name}",
                         layout="packed")


@pytest.mark.parametrize("mode", MODES)
def test_river_paths_bit_identical_renumbered(mode, oracle_mod, monkeypatch):
    """the river kernel's build paths (SHUD_RHS_QD x SHUD_RIV_SB, tp.test_river_paths_bit_identical) on the fully
    renumbered junction model: the same bits on every path, and one path against the oracle"""
    rt = tp._runtime()
    m2, ys = _full("junctions")
    ys = ys[:2]
    outs = {}
    for qd in ("1", "0"):
        for sb in ("6", "8"):
            monkeypatch.setenv("SHUD_RHS_QD", qd)
            monkeypatch.setenv("SHUD_RIV_SB", sb)
            g = rt.RhsHandle(m2, mode=mode)
            assert g.layout()["packed"]
            g.set_step_inputs()
            seq = [g.eval(0.0, y) for y in ys for _ in range(3)]
            dg = g.diagnostics()
            outs[(qd, sb)] = (seq, {k: dg[k] for k in ("qriv_down", "qriv_up", "qriv_surf", "qriv_sub")})
            g.close()
    ref_seq, ref_dg = outs[("0", "8")]
    for key, (seq, dg) in outs.items():
        for c, (a, b) in enumerate(zip(seq, ref_seq)):
            assert np.array_equal(a, b, equal_nan=True), f"QD={key[0]} SB={key[1]} call {c}"
        for k in dg:
            assert np.array_equal(dg[k], ref_dg[k], equal_nan=True), f"QD={key[0]} SB={key[1]} {k}"
    o = oracle_mod.OracleRhs(m2, mode)
    o.set_step_inputs()
    seq, k = outs[("1", "6")][0], 0
    for si, y in enumerate(ys):
        for c in range(3):
            ref, code, _, _ = o.eval(0.0, y)
            assert code == 0
            assert_close(seq[k], ref, what=f"renumbered junctions QD SB6 state {si} call {c}")
            k += 1


# ---------------------------------------------------------------- c. sharing under tile-local numbering
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("numbering", rn.SHARE_NUMBERINGS)
@pytest.mark.parametrize("mesh", list(rn.SHARE_MESHES))
def test_share_tile_local_numbering(mesh, numbering, mode, oracle_mod, monkeypatch):
    """ts.test_share_same_bits_and_oracle on numberings that reach every (published, received) slot state, the
    cross-wave LDS hand-off and both index orders of a pair: sharing on vs off bit for bit over the four sign-rule
    states x 2 stateful calls, sharing on against the oracle, and the host's pairing against the restated rule"""
    m2, _ = rn.share_input(mesh, numbering)
    a, b = ts._handles(m2, mode, monkeypatch)
    try:
        assert a.layout()["shared_edges"] == int((rn.share_assignment(m2)[1] >= 0).sum())
        o = oracle_mod.OracleRhs(m2, mode)
        o.set_step_inputs()
        for si, y in enumerate(ts._states(m2, 70)):
            for c in range(2):
                ga, ea = ts._run(a, y)
                gb, eb = ts._run(b, y)
                ref, code, _, _ = o.eval(0.0, y)
                assert ea is None and eb is None and code == 0, (ea, eb, code)
                ts._same_bits(ga, gb, f"{mesh} {numbering} state {si} call {c}")
                assert_close(ga, ref, what=f"{mesh} {numbering} shared, state {si} call {c}")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("kind", ["nan_surface", "nan_gw", "inf_surface"])
@pytest.mark.parametrize("mesh", list(rn.SHARE_MESHES))
def test_share_nonfinite_heads_on_shared_edges(mesh, kind, oracle_mod, monkeypatch):
    """ts.test_share_nonfinite_heads with the NaN / infinite heads placed on shared edges of the block-shuffled mesh,
    taken from the restated assignment: both ends of 8 shared edges (an infinite head on both ends puts inf - inf on
    a published edge), the publisher alone on 2 and the receiver alone on 2; half of the edges cross a wave.  The
    error exit and its first element are those of the unshared kernel and of the oracle."""
    m2, _ = rn.share_input(mesh, "block")
    a, b = ts._handles(m2, abi.SHUD_MODE_SERIAL, monkeypatch)
    try:
        o = oracle_mod.OracleRhs(m2, 0)
        o.set_step_inputs()
        NE = m2.num_ele
        pub, rcv = rn.share_assignment(m2)
        assert a.layout()["shared_edges"] == int((rcv >= 0).sum())
        recv = np.nonzero(rcv >= 0)[0]
        pubr = m2.nabr.reshape(3, NE)[rcv[recv], recv]
        cross = (recv % 256) // 64 != (pubr % 256) // 64
        rng = np.random.default_rng(9)
        pick = np.concatenate([rng.choice(np.nonzero(cross)[0], 6, replace=False),
                               rng.choice(np.nonzero(~cross)[0], 6, replace=False)])
        r, p = recv[pick], pubr[pick]
        assert (pub[p] >= 0).all() and (m2.nabr.reshape(3, NE)[pub[p], p] == r).all()
        ends = np.concatenate([r[[0, 1, 2, 3, 6, 7, 8, 9]], p[[0, 1, 2, 3, 6, 7, 8, 9]], p[[4, 10]], r[[5, 11]]])
        y = workload.random_state(m2, seed=5)
        bad = np.nan if kind.startswith("nan") else np.inf
        y[(2 * NE if kind == "nan_gw" else 0) + ends] = bad
        ga, ea = ts._run(a, y)
        gb, eb = ts._run(b, y)
        _, code, idx, ekind = o.eval(0.0, y)
        assert ea == eb, (ea, eb)
        if code:
            assert ea is not None and ea["exit_code"] == code
            if ekind == abi.EF_NAN_QELE:                  # CheckNANij: the first element with a NaN lateral flux
                assert ea["first_index"][0] == idx, (ea["first_index"], idx)
        else:
            ts._same_bits(ga, gb, kind)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- d. partitioned handles
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nranks,method", [(3, partition.PART_MULTILEVEL), (8, partition.PART_AUTO)])
def test_partitions_of_renumbered_mesh(nranks, method, mode):
    """a fully renumbered mesh (global ids say nothing about adjacency) through the C++ partitioner, planner and
    local-mesh gather: every rank's owned DY bit-identical to one GPU"""
    m, y = cases.variant(6000, seed=2)
    m2, map_y = rn.renumber(m, **rn.full_numbering(m, np.random.default_rng(29)))
    ep, _ = partition.cpp_partition(m2, nranks, method)
    locs = [partition.CppPlan(m2, ep, nranks, r).local_model() for r in range(nranks)]
    tpart._run_ranks(m2, [map_y(y), workload.random_state(m2, seed=3)], locs, mode, ncalls=2)


# ---------------------------------------------------------------- depression = NULL
@pytest.mark.parametrize("layout_", ["packed", "soa"])
def test_depression_null(layout_, oracle_mod, monkeypatch):
    """ShudMeshSoA.depression = NULL means 0.0002 everywhere (include/shud_rhs.h): a handle built from it (edge
    sharing on, the default) gives the DY bits and the shared-edge count of a handle built from the explicit array,
    and agrees with the oracle"""
    monkeypatch.setenv("SHUD_RHS_PACKED", "1" if layout_ == "packed" else "0")
    rt = tp._runtime()
    m, y = rn.share_input("v3000", "block")
    m.ele["depression"] = np.full(m.num_ele, 0.0002)
    m.finalize()
    mn = copy.deepcopy(m)
    del mn.ele["depression"]
    assert not mn.mesh_struct().depression and m.mesh_struct().depression      # NULL vs the array
    a, b = rt.RhsHandle(m), rt.RhsHandle(mn)
    try:
        la, lb = a.layout(), b.layout()
        assert la == lb and la["packed"] == (layout_ == "packed"), (la, lb)
        if layout_ == "packed":
            assert la["shared_edges"] == int((rn.share_assignment(m)[1] >= 0).sum()) > 0.3 * m.num_ele
        o = oracle_mod.OracleRhs(mn, 0)
        a.set_step_inputs()
        b.set_step_inputs()
        o.set_step_inputs()
        for si, yy in enumerate([y, workload.random_state(m, seed=8)]):
            for c in range(2):
                ga, gb = a.eval(0.0, yy), b.eval(0.0, yy)
                ref, code, _, _ = o.eval(0.0, yy)
                assert code == 0
                ts._same_bits(ga, gb, f"depression NULL {layout_} state {si} call {c}")
                assert_close(gb, ref, what=f"depression NULL {layout_} state {si} call {c}")
    finally:
        a.close()
        b.close()
