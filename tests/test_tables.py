"""CPU: the host tables a handle uploads at create (shud_tables.cpp), through shud_rhs_plan_layout.

The pairing and evaluation-order rules, the interior prefix of a partitioned handle, the layout choice, the fallbacks
to the SoA layout and the validation messages are all decided on the host before anything reaches a device; here they
are compared with their numpy restatements (renumber.share_assignment / eval_order) and with what the GPU layout tests
assert, on the inputs those tests use."""
import copy
import functools

import numpy as np
import pytest

import cases
import renumber as rn
from shud_rhs import abi, partition, runtime


def decode_plan(bits):
    """edge_plan words (shud_dev.h kEvoShift, shifted down) -> (e [3, NE], published flag, received flag): bits 0-1
    the stored slot that holds reference slot 0; bit 2: of the other two stored slots, ascending, the first holds
    reference slot 2 (else 1); bit 3: stored slot 0 is a publication; bit 4: stored slot 2 is received"""
    bits = np.asarray(bits, dtype=np.int64)
    assert ((bits >= 0) & (bits < 32)).all() and ((bits & 3) < 3).all()
    s0, sw, k = bits & 3, (bits >> 2) & 1, np.arange(bits.size)
    lo, hi = np.where(s0 == 0, 1, 0), np.where(s0 == 2, 1, 2)
    e = np.empty((3, bits.size), dtype=np.int64)
    e[s0, k] = 0
    e[lo, k] = np.where(sw == 1, 2, 1)
    e[hi, k] = np.where(sw == 1, 1, 2)
    return e, (bits >> 3) & 1 == 1, (bits >> 4) & 1 == 1


def _assert_plan(m, pl, pub, rcv):
    """the plan of model m is the restated assignment (pub, rcv) in the restated order"""
    NE = m.num_ele
    nabr = np.asarray(m.nabr).reshape(3, NE)
    e, pflag, rflag = decode_plan(pl["edge_plan"])
    assert np.array_equal(e, rn.eval_order(pub, rcv))
    assert np.array_equal(pflag, pub >= 0) and np.array_equal(rflag, rcv >= 0)
    assert np.array_equal(pl["stored_nabr"], nabr[e, np.arange(NE)[None, :]])
    assert pl.get("shared_edges", 0) == int((rcv >= 0).sum())


def _assert_unshared(m, pl):
    assert not pl["edge_plan"].any()
    assert np.array_equal(pl["stored_nabr"], np.asarray(m.nabr).reshape(3, -1))
    assert "shared_edges" not in pl


# ---------------------------------------------------------------- sharing
@pytest.mark.parametrize("numbering", rn.SHARE_NUMBERINGS)
def test_share_plan_is_the_restated_rule(numbering):
    m, _ = rn.share_input("v3000", numbering)
    pl = runtime.plan_layout(m, arrays=True)
    pub, rcv = rn.share_assignment(m)
    assert pl["packed"] and (rcv >= 0).sum() > 0.3 * m.num_ele
    _assert_plan(m, pl, pub, rcv)


def test_share_off(monkeypatch):
    monkeypatch.setenv("SHUD_RHS_SHARE", "0")
    m, _ = rn.share_input("v3000", "block")
    pl = runtime.plan_layout(m, arrays=True)
    assert pl["packed"]
    _assert_unshared(m, pl)


def test_share_needs_two_elements():
    """one element below lim: the packed layout without a plan, as with SHUD_RHS_SHARE=0"""
    m, _ = cases.single_element()
    pl = runtime.plan_layout(m, arrays=True)
    assert pl["packed"]
    _assert_unshared(m, pl)


def test_depression_null_plans():
    """depression = NULL (0.0002 everywhere) with sharing on: the plan of the explicit array"""
    m, _ = rn.share_input("v3000", "block")
    m.ele["depression"] = np.full(m.num_ele, 0.0002)
    m.finalize()
    mn = copy.deepcopy(m)
    del mn.ele["depression"]
    assert not mn.mesh_struct().depression and m.mesh_struct().depression
    a, b = runtime.plan_layout(m, arrays=True), runtime.plan_layout(mn, arrays=True)
    assert a["packed"] and a["shared_edges"] == int((rn.share_assignment(m)[1] >= 0).sum()) > 0.3 * m.num_ele
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---------------------------------------------------------------- partitioned
@functools.lru_cache(maxsize=None)
def _locals():
    m, _ = cases.variant(3000, seed=5)
    ep, _ = partition.cpp_partition(m, 4, partition.PART_AUTO)
    return [partition.CppPlan(m, ep, 4, r).local_model() for r in range(4)]


def test_partitioned_interior_prefix_and_sharing():
    shared = []
    for lm, part in _locals():
        pl = runtime.plan_layout(lm, partition=part, arrays=True)
        n_own, n_own_riv = part.n_own_ele, part.n_own_riv
        dep = (np.asarray(lm.nabr).reshape(3, -1)[:, :n_own] >= n_own).any(0)
        dep[lm.seg_ele[(lm.seg_riv >= n_own_riv) & (lm.seg_ele < n_own)]] = True
        n_int = int(np.argmax(dep)) if dep.any() else n_own
        assert pl["n_int"] == n_int and pl["packed"], (pl["n_int"], n_int)
        pub, rcv = rn.share_assignment(lm, lim=n_int)
        _assert_plan(lm, pl, pub, rcv)
        shared.append(pl.get("shared_edges", 0))
    assert max(shared) > 0, shared            # the input must share on some rank, or the above compares nothing


# ---------------------------------------------------------------- layout choice
@pytest.mark.parametrize("mode", [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP])
@pytest.mark.parametrize("kind", ["packed_share", "mid_class", "hybrid4", "big_table", "l2", "soa"])
def test_layout_choice(kind, mode, monkeypatch):
    """what test_gpu_renumber.test_element_numbering_invariance asserts of each handle's layout"""
    m, _, check = cases.layout_model(kind, monkeypatch)
    pl = runtime.plan_layout(m, mode=mode)
    assert check(pl), pl


@pytest.mark.parametrize("sy", [False, True])
def test_layout_hybrid_1_and_2(sy):
    """test_gpu_parity.test_many_classes, hybrid1 / hybrid"""
    m, _ = cases.many_class_model(sy=sy)
    lay = runtime.plan_layout(m)
    assert lay["packed"] and lay.get("streamed_fields") == (2 if sy else 1), lay
    assert lay["n_classes"] <= 128, lay


def test_layout_many_classes_soa(monkeypatch):
    """test_gpu_parity.test_many_classes, soa: no hybrid layout and no L2 class table"""
    monkeypatch.setenv("SHUD_RHS_HYB", "0")
    monkeypatch.setenv("SHUD_RHS_L2_CLASS", "0")
    m, _ = cases.many_class_model()
    assert not runtime.plan_layout(m)["packed"]


@pytest.mark.parametrize("target", ["mid", "max"])
def test_layout_big_class_table(target, monkeypatch):
    """test_gpu_parity.test_lds_big_class_table"""
    monkeypatch.setenv("SHUD_RHS_HYB", "0")
    m, _, n = cases.big_table_model(target)
    lay = runtime.plan_layout(m)
    assert lay["packed"] and not lay.get("streamed_fields") and lay["n_classes"] == n, lay


# ---------------------------------------------------------------- fallbacks to the SoA layout
def _avg_rough(m):
    m.ele["avg_rough"][m.num_ele + 7] *= 1.0 + 1e-9


def _aquifer(m):
    m.par["aquifer_depth"][3] += 1e-3


def _beta(m):
    m.par["Beta"][11] = 1.0                   # a class of its own with Beta <= 1: the full pow of the SoA kernel


def _seg64(m):
    m.seg_ele = np.concatenate([m.seg_ele, np.full(64, 17, np.int32)])
    m.seg_riv = np.concatenate([m.seg_riv, np.zeros(64, np.int32)])
    m.seg_length = np.concatenate([m.seg_length, np.full(64, 1.5)])
    m.seg_cwr = np.concatenate([m.seg_cwr, np.full(64, 0.6)])
    m.num_seg += 64


@pytest.mark.parametrize("change", [_avg_rough, _aquifer, _beta, _seg64])
def test_fallback_to_soa(change):
    m, _ = cases.variant(3000, seed=5)
    assert runtime.plan_layout(m)["packed"]
    change(m)
    m.finalize()
    pl = runtime.plan_layout(m, arrays=True)            # no error
    assert not pl["packed"] and pl["n_classes"] == 0 and pl["riv_sb"] == 0, pl
    _assert_unshared(m, pl)


# ---------------------------------------------------------------- validation
def _bad_nabr(m):
    m.nabr[5] = m.num_ele
    return f"nabr[5]={m.num_ele} out of range"


def _bad_riv_down(m):
    m.riv_down[2] = -7
    return "Fatal Error: River Routing Boundary Condition Type Is Wrong! (reach 2 down -7)"


def _bad_segment(m):
    m.seg_ele[4] = m.num_ele
    return "segment 4 references element/reach out of range"


def _lake_without_bathymetry(m):
    m.ilake = np.zeros(m.num_ele, dtype=np.int32)
    m.ilake[5] = 1
    return "lake elements present but no lake bathymetry (num_lake 0)"


@pytest.mark.parametrize("change", [_bad_nabr, _bad_riv_down, _bad_segment, _lake_without_bathymetry])
def test_validation(change):
    m, _ = cases.ccw()
    text = change(m)
    with pytest.raises(runtime.ShudRhsError) as ei:
        runtime.plan_layout(m)
    assert ei.value.code == abi.SHUD_ERR_ARG and str(ei.value).endswith(": " + text), str(ei.value)


def test_validation_partition_counts():
    lm, part = _locals()[0]
    part = copy.copy(part)
    part.ele_gid = np.concatenate([part.ele_gid, [0]])      # n_own + n_segghost = num_ele + 1
    assert part.n_own_ele + part.n_segghost_ele > lm.num_ele
    with pytest.raises(runtime.ShudRhsError) as ei:
        runtime.plan_layout(lm, partition=part)
    assert ei.value.code == abi.SHUD_ERR_ARG
    assert str(ei.value).endswith(": partition counts inconsistent with mesh sizes"), str(ei.value)
