"""CPU: element locality ordering without a device (include/shud_order.h): the planner against a numpy restatement
of its rule, the appliers against tests/renumber.py, the refusal of lake models, and what the breadth-first order is
worth to the in-tile edge sharing on the shipped meshes (the restated assignment, renumber.share_assignment, and the
host's own plan, shud_rhs_plan_layout)."""
from collections import deque

import numpy as np
import pytest

import cases
import renumber as rn
from shud_rhs import abi, runtime


def bfs_restated(m):
    """the rule of shud_order_plan(SHUD_ORDER_BFS): components start from the unvisited elements in ascending (number
    of nabr >= 0 slots, index); FIFO queue; neighbours enqueued in slot order 0, 1, 2 when first seen"""
    NE = m.num_ele
    nabr = np.asarray(m.nabr).reshape(3, NE)
    deg = (nabr >= 0).sum(0)
    starts = np.lexsort((np.arange(NE), deg))
    seen = np.zeros(NE, dtype=bool)
    out = []
    for r in starts:
        if seen[r]:
            continue
        seen[r] = True
        q = deque([int(r)])
        while q:
            i = q.popleft()
            out.append(i)
            for j in range(3):
                v = int(nabr[j, i])
                if v >= 0 and not seen[v]:
                    seen[v] = True
                    q.append(v)
    return np.array(out, dtype=np.int32)


MODELS = {"ccw": cases.ccw, "heihe": cases.heihe, "qhh": cases.qhh, "v3000": lambda: cases.variant(3000, seed=5)}
_cache = {}


def model(name):
    if name not in _cache:
        _cache[name] = MODELS[name]()[0]
    return _cache[name]


@pytest.mark.parametrize("name", list(MODELS))
def test_bfs_plan_equals_restated_rule(name):
    m = model(name)
    perm = runtime.order_plan(m, "bfs")
    assert np.array_equal(np.sort(perm), np.arange(m.num_ele))
    assert np.array_equal(perm, bfs_restated(m))


def test_bfs_plan_random_numbering_cut_edges():
    """a randomly numbered mesh with every seventh element's edges cut on its own side only (more boundary slots,
    several search starts, an adjacency that is no longer symmetric): still the restated rule's order"""
    m = model("v3000")
    rng = np.random.default_rng(3)
    m2, _ = rn.renumber(m, pe=rng.permutation(m.num_ele))
    nb = np.asarray(m2.nabr).reshape(3, -1).copy()
    nb[:, ::7] = np.where(nb[:, ::7] >= 0, -1, nb[:, ::7])      # cut edges one way: asymmetric adjacency is still planned
    m2.nabr = nb.reshape(-1).astype(np.int32)
    perm = runtime.order_plan(m2, "bfs")
    assert np.array_equal(perm, bfs_restated(m2))


def test_identity_and_user_plans():
    m = model("ccw")
    NE = m.num_ele
    assert np.array_equal(runtime.order_plan(m, "identity"), np.arange(NE))
    p = np.random.default_rng(1).permutation(NE).astype(np.int32)
    assert np.array_equal(runtime.order_plan(m, p), p)


@pytest.mark.parametrize("bad", ["repeat", "negative", "too_big"])
def test_user_plan_rejects_non_permutation(bad):
    m = model("ccw")
    p = np.arange(m.num_ele, dtype=np.int32)
    if bad == "repeat":
        p[5] = p[6]
    elif bad == "negative":
        p[0] = -1
    else:
        p[-1] = m.num_ele
    with pytest.raises(runtime.ShudRhsError) as e:
        runtime.order_plan(m, p)
    assert e.value.code == abi.SHUD_ERR_ARG
    with pytest.raises(runtime.ShudRhsError) as e:
        runtime.order_apply(m, p)
    assert e.value.code == abi.SHUD_ERR_ARG


@pytest.mark.parametrize("name", ["ccw", "heihe", "v3000"])
def test_apply_equals_renumber(name):
    """shud_order_apply == renumber.renumber(m, pe=perm), field for field (bits), for the breadth-first plan and for
    a random permutation"""
    m = model(name)
    for perm in (runtime.order_plan(m, "bfs"), np.random.default_rng(7).permutation(m.num_ele).astype(np.int32)):
        a = runtime.order_apply(m, perm)
        r, _ = rn.renumber(m, pe=perm)
        assert (a.num_ele, a.num_riv, a.num_seg, a.close_boundary) == (r.num_ele, r.num_riv, r.num_seg, r.close_boundary)
        for grp in ("ele", "par", "step", "riv"):
            da, dr = getattr(a, grp), getattr(r, grp)
            assert set(da) == set(dr), grp
            for k in dr:
                assert da[k].dtype == dr[k].dtype and np.array_equal(da[k].view(np.uint64), dr[k].view(np.uint64)), (grp, k)
        for k in ("nabr", "ibc", "iss", "riv_down", "riv_bc", "seg_ele", "seg_riv"):
            assert np.array_equal(getattr(a, k), getattr(r, k)), k
        for k in ("seg_length", "seg_cwr"):
            assert np.array_equal(getattr(a, k).view(np.uint64), getattr(r, k).view(np.uint64)), k
        assert a.ilake is None and r.ilake is None or np.array_equal(a.ilake, r.ilake)


def test_gather_host_planes_and_widths():
    rng = np.random.default_rng(2)
    n = 257
    perm = rng.permutation(n).astype(np.int32)
    for dt, planes in ((np.float64, 1), (np.float64, 3), (np.int32, 1), (np.int16, 2), (np.dtype("V24"), 1)):
        if dt == np.dtype("V24"):
            a = rng.integers(0, 255, n * 24, dtype=np.uint8).view(dt)
        else:
            a = rng.integers(-1000, 1000, planes * n).astype(dt)
        got = runtime.order_gather(perm, a, planes)
        assert got.tobytes() == a.reshape(planes, n)[:, perm].tobytes()


def test_lake_model_refused():
    m = model("qhh")
    perm = runtime.order_plan(m, "bfs")         # planning needs only the adjacency
    with pytest.raises(runtime.ShudRhsError) as e:
        runtime.order_apply(m, perm)
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED
    # ordered create refuses it before it touches a device
    with pytest.raises(runtime.ShudRhsError) as e:
        runtime.RhsHandle(m, order="bfs")
    assert e.value.code == abi.SHUD_ERR_UNSUPPORTED


def _share(m):
    """share of elements that receive a shared edge, by the restated assignment"""
    return float((rn.share_assignment(m)[1] >= 0).sum()) / m.num_ele


@pytest.mark.parametrize("name,floor", [("ccw", 0.80), ("heihe", 0.80)])
def test_bfs_recovers_sharing_on_shipped_meshes(name, floor):
    """file order -> breadth-first: at least `floor` of the elements receive a shared edge (measured: ccw 0.861,
    heihe 0.856), strictly more than in file order (ccw 0.615, heihe 0.486); the host's plan counts the same"""
    m = model(name)
    a = runtime.order_apply(m, runtime.order_plan(m, "bfs"))
    before, after = _share(m), _share(a)
    print(f"{name}: file order {before:.3f}, breadth-first {after:.3f}")
    assert after >= floor
    assert after > before
    lay = runtime.plan_layout(a)
    assert lay["packed"] and lay["shared_edges"] == int((rn.share_assignment(a)[1] >= 0).sum())


def test_bfs_recovers_sharing_after_random_permutation():
    """variant(20000, 43) under a seeded random permutation (share 0.018), then breadth-first: >= 0.70 (measured
    0.743); the host's plan counts the same"""
    m, _ = cases.variant(20000, seed=43)
    m2, _ = rn.renumber(m, pe=np.random.default_rng(43).permutation(m.num_ele))
    a = runtime.order_apply(m2, runtime.order_plan(m2, "bfs"))
    rnd, after = _share(m2), _share(a)
    print(f"variant(20000, 43): random {rnd:.3f}, then breadth-first {after:.3f}")
    assert rnd < 0.05
    assert after >= 0.70
    assert runtime.plan_layout(a)["shared_edges"] == int((rn.share_assignment(a)[1] >= 0).sum())
