"""CPU: the renumbering helper (tests/renumber.py) and the preconditions of the GPU renumbering tests.

The oracle is the yardstick of test_gpu_renumber.py, so it is pinned under renumbering first: renumbering the
elements alone leaves every element's operation order as it was, hence the oracle's DY must be the permuted DY of the
original model word for word; under a full renumbering (reaches, segments, edge slots as well) the sums change order
and only the two restatements (C and numpy) can be compared bit for bit.  The coverage test states, as a condition on
the inputs, which in-tile edge-sharing states the GPU sharing tests reach."""
import numpy as np
import pytest

import cases
import renumber as rn
from shud_rhs import abi

MODELS = ["ccw", "heihe", "variant3000"]


def _model(name):
    return cases.variant(3000, seed=5) if name == "variant3000" else getattr(cases, name)()


def _bit_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype == np.float64:
        return bool((a.view(np.uint64) == b.view(np.uint64)).all())
    return bool((a == b).all())


def _two_states(m, y):
    return [y] + cases.states(m, None, 1, seed=31)


def test_conventions():
    """what the maps mean, checked directly on a drawn full renumbering: new element k is old pe[k] with its slots
    rotated by rot[k], neighbours / segment owners / downstream reaches name the same entities as before"""
    m, y = cases.variant(3000, seed=5)
    rng = np.random.default_rng(2)
    kw = rn.full_numbering(m, rng)
    m2, map_y = rn.renumber(m, **kw)
    nb = map_y.__self__
    pe, pr, ps, rot = kw["pe"], kw["pr"], kw["ps"], kw["rot"]
    NE = m.num_ele
    assert (m2.num_ele, m2.num_riv, m2.num_seg) == (m.num_ele, m.num_riv, m.num_seg)
    old_nabr, new_nabr = m.nabr.reshape(3, NE), m2.nabr.reshape(3, NE)
    for j in range(3):
        old = old_nabr[(j + rot) % 3, pe]
        new = new_nabr[j]
        assert np.array_equal(new < 0, old < 0) and np.array_equal(new[new < 0], old[old < 0])
        assert np.array_equal(pe[new[new >= 0]], old[old >= 0])
        for k in ("edge", "dist2nabor", "dist2edge", "avg_rough"):
            assert _bit_equal(m2.ele[k].reshape(3, NE)[j], m.ele[k].reshape(3, NE)[(j + rot) % 3, pe]), k
    assert _bit_equal(m2.ele["z_surf"], m.ele["z_surf"][pe]) and _bit_equal(m2.par["KsatH"], m.par["KsatH"][pe])
    assert _bit_equal(m2.step["ugw_stale"], m.step["ugw_stale"][pe]) and np.array_equal(m2.ibc, m.ibc[pe])
    assert np.array_equal(pe[m2.seg_ele], m.seg_ele[ps]) and np.array_equal(pr[m2.seg_riv], m.seg_riv[ps])
    assert _bit_equal(m2.seg_length, m.seg_length[ps])
    od, nd = m.riv_down[pr], m2.riv_down
    assert np.array_equal(nd < 0, od < 0) and np.array_equal(nd[nd < 0], od[od < 0])
    assert np.array_equal(pr[nd[nd >= 0]], od[od >= 0])
    assert (np.diff(m2.seg_riv) < 0).any() and (np.diff(m2.seg_ele) < 0).any()    # sorted by neither
    y2 = map_y(y)
    assert _bit_equal(y2[NE:2 * NE], y[NE:2 * NE][pe]) and _bit_equal(y2[3 * NE:], y[3 * NE:][pr])
    assert _bit_equal(nb.unmap_y(y2), y)
    e3 = rng.random(3 * NE)
    assert _bit_equal(nb.unmap_edge(nb.edge(e3)), e3) and _bit_equal(nb.unmap_seg(nb.seg(m.seg_cwr)), m.seg_cwr)
    assert _bit_equal(nb.unmap_ele(nb.ele(e3[:NE])), e3[:NE])
    assert _bit_equal(nb.unmap_riv(nb.riv(m.riv["riv_depth"])), m.riv["riv_depth"])


@pytest.mark.parametrize("name", MODELS + ["qhh"])
def test_round_trip(name):
    """renumbering, then renumbering back by the inverse maps, returns every array bit for bit"""
    m, _ = cases.qhh() if name == "qhh" else _model(name)
    rng = np.random.default_rng(3)
    m2, map_y = rn.renumber(m, **rn.full_numbering(m, rng))
    m3, _ = rn.renumber(m2, **map_y.__self__.inverse_args())
    assert not _bit_equal(m2.nabr, m.nabr)
    for field in ("ele", "par", "step", "riv", "bc_tables"):
        a, b = getattr(m, field), getattr(m3, field)
        assert a.keys() == b.keys(), field
        for k in a:
            assert _bit_equal(a[k], b[k]), (field, k)
    for k in ("nabr", "ibc", "iss", "ilake", "riv_down", "riv_bc", "seg_ele", "seg_riv", "seg_length", "seg_cwr",
              "lake_bathy_off", "lake_bathy_y", "lake_bathy_a"):
        a, b = getattr(m, k), getattr(m3, k)
        assert (a is None and b is None) or _bit_equal(a, b), k
    for k in ("x", "y") if "x" in m.meta else ():                     # element centroids (the partitioner's input)
        assert not _bit_equal(m2.meta[k], m.meta[k]) and _bit_equal(m3.meta[k], np.asarray(m.meta[k]))
    assert (m3.num_ele, m3.num_riv, m3.num_seg, m3.num_lake, m3.close_boundary) == \
           (m.num_ele, m.num_riv, m.num_seg, m.num_lake, m.close_boundary)


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
@pytest.mark.parametrize("numbering", ["random_perm", "block_shuffle"])
@pytest.mark.parametrize("name", MODELS)
def test_oracle_invariant_under_element_renumbering(name, numbering, mode, oracle_mod):
    """elements renumbered only (reaches, segment order, each element's slot order kept): every element's operation
    order is unchanged, so oracle(m2)(map_y(y)) == map_y(oracle(m)(y)) word for word, 2 states x 2 stateful calls"""
    m, y = _model(name)
    rng = np.random.default_rng(7)
    pe = rn.random_perm(m.num_ele, rng) if numbering == "random_perm" else rn.block_shuffle(m.num_ele, rng)
    m2, map_y = rn.renumber(m, pe=pe)
    o, o2 = oracle_mod.OracleRhs(m, mode), oracle_mod.OracleRhs(m2, mode)
    o.set_step_inputs()
    o2.set_step_inputs()
    for si, yy in enumerate(_two_states(m, y)):
        for c in range(2):
            a, code, _, _ = o.eval(0.0, yy)
            b, code2, _, _ = o2.eval(0.0, map_y(yy))
            assert code == 0 and code2 == 0
            assert _bit_equal(map_y(a), b), f"{name} {numbering} mode {mode} state {si} call {c}"


@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
@pytest.mark.parametrize("name", MODELS)
def test_two_restatements_full_renumbering(name, mode, oracle_mod):
    """pe, pr, ps and rot all drawn (segments sorted neither by reach nor by element): the C and the numpy
    restatement still agree bit for bit, DY and every diagnostic (as test_oracle.py on the original numbering)"""
    import numpy_oracle
    m, y = _model(name)
    m2, map_y = rn.renumber(m, **rn.full_numbering(m, np.random.default_rng(11)))
    o, n = oracle_mod.OracleRhs(m2, mode), numpy_oracle.NumpyRhs(m2, mode)
    o.set_step_inputs()
    n.set_step_inputs()
    for si, yy in enumerate(_two_states(m, y)):
        for c in range(2):
            a, code, _, _ = o.eval(0.0, map_y(yy))
            assert code == 0
            assert _bit_equal(a, n.eval(0.0, map_y(yy))), f"{name} mode {mode} state {si} call {c}"
    d = o.diagnostics()
    for k, v in n.diag.items():
        assert _bit_equal(v, d[k]), k


def test_share_assignment_grid_numbering():
    """the restated rule on the generator's own numbering: the counts of shared edges are those of the grid (one
    shared edge per element at the most, publisher and receiver are neighbours of one tile, no edge shared twice)"""
    m, _ = cases.variant(3000, seed=5)
    NE = m.num_ele
    pub, rcv = rn.share_assignment(m)
    nabr = m.nabr.reshape(3, NE)
    recv = np.nonzero(rcv >= 0)[0]
    pubr = nabr[rcv[recv], recv]
    assert recv.size == (pub >= 0).sum() > 0.3 * NE
    assert (pubr // 256 == recv // 256).all() and np.unique(pubr).size == pubr.size
    assert (nabr[pub[pubr], pubr] == recv).all()                     # the published slot is the edge back
    both = recv[pub[recv] >= 0]                                      # never both directions of one edge
    assert (pub[both] != rcv[both]).all()
    p0, r0 = rn.share_assignment(m, lim=1000)
    assert (p0[1000:] < 0).all() and (r0[1000:] < 0).all() and (r0 >= 0).sum() > 300


@pytest.mark.parametrize("numbering", rn.SHARE_NUMBERINGS)
@pytest.mark.parametrize("mesh", list(rn.SHARE_MESHES))
def test_share_inputs_cover_the_sharing_states(mesh, numbering):
    """A condition on the inputs of test_gpu_renumber.py's sharing tests, not a measurement: the assignment on each
    reaches all 13 (published slot, received slot) states on >= 10 elements each, >= 25 % of the shared edges cross
    a 64-lane wave, either index order of publisher and receiver holds >= 10 % of them, the last tile is partial.

    One state is out of reach of one input: on the 20,022-element mesh under block_shuffle alone no element is left
    with neither a published nor a received edge (0 such elements for every seed tried: its tiles are 1.3 grid rows
    long, so every element has two in-tile neighbours and the greedy rule always pairs it).  That state is the
    kernel's path without sharing; the same mesh reaches it under block_roll, and the small mesh under both.  There
    the other 12 states are required as everywhere."""
    m2, _ = rn.share_input(mesh, numbering)
    pub, rcv = rn.share_assignment(m2)
    s = rn.share_stats(m2, pub, rcv)
    print(mesh, numbering, s)
    need = dict(s["states"])
    assert len(need) == 13
    if (mesh, numbering) == ("v20000", "block"):
        del need[(-1, -1)]
    assert min(need.values()) >= 10, s["states"]
    assert s["cross_wave"] >= 0.25 and s["pub_below"] >= 0.10 and s["pub_above"] >= 0.10, s
    assert s["last_tile_partial"]
    assert s["shared"] > 0.3 * m2.num_ele
