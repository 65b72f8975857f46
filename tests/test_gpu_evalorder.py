"""Edges stored in evaluation order (shud_tables.cpp share_plan, shud_dev.h kEvoShift; shud_ele_packed.hip SH).

On a handle that shares edges the host stores every element's three neighbours and {edge, Dist2Nabor} records in the
order the sharing kernel evaluates them — the published slot first, the received slot last — and the kernels go back
to the reference's slot order for the sums, the per-slot diagnostics and dist2edge.  Nothing a caller can see may
change: DY, the error words and every diagnostic array are compared bit for bit with the handle built with
SHUD_RHS_SHARE=0 (reference order, every edge evaluated from both sides), and DY with the oracle.  The inputs are
chosen on the CPU (renumber.share_assignment restates the host's pairing, renumber.eval_order its ordering rule) so
that all six orders and all four publish / receive states occur."""
import functools

import numpy as np
import pytest

import cases
import renumber as rn
import test_gpu_partition as tpart
from renumber import eval_order
from conftest import assert_close
from shud_rhs import abi, partition, synth, workload

pytestmark = pytest.mark.gpu

MODES = [abi.SHUD_MODE_SERIAL, abi.SHUD_MODE_OMP]
MESHES = ("syn", "variant")
NUMBERINGS = rn.SHARE_NUMBERINGS
ORDERS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]


def _rt():
    from shud_rhs import runtime
    return runtime


@functools.lru_cache(maxsize=None)
def _model(mesh, numbering):
    """-> (renumbered model, pub, rcv): syn-20000 (closed boundary, fu = 1) or the branch-variant mesh (open boundary,
    BC elements, SS flags, fu != 1) under a tile-local numbering with a random rotation of every element's slots"""
    if mesh == "syn":
        m = synth.synth_model(20000, seed=41)
        m.step = workload.random_step_inputs(m, seed=3)
    else:
        m, _ = cases.variant(20000, seed=43)
    m2, _ = rn.renumber(m, **rn.share_numbering(m.num_ele, numbering, 2000 + len(mesh)))
    pub, rcv = rn.share_assignment(m2)
    return m2, pub, rcv


def _handles(m, mode, monkeypatch, rcv):
    rt = _rt()
    monkeypatch.setenv("SHUD_RHS_SHARE", "1")
    a = rt.RhsHandle(m, mode=mode)
    monkeypatch.setenv("SHUD_RHS_SHARE", "0")
    b = rt.RhsHandle(m, mode=mode)
    monkeypatch.delenv("SHUD_RHS_SHARE")
    la, lb = a.layout(), b.layout()
    n = int((rcv >= 0).sum())
    assert n > 0 and la["packed"] and la.get("shared_edges", 0) == n, (la, n)
    assert "shared_edges" not in lb, lb
    a.set_step_inputs()
    b.set_step_inputs()
    return a, b


def _run(h, y):
    """(DY, error words): the DY vector is returned even when the reference would have exited"""
    g = h.eval(0.0, y, raise_on_physics=False)
    e = h.get_error()
    e.pop("message", None)
    h.clear_error()
    return g, e


def _same_bits(a, b, what):
    assert a.shape == b.shape
    ua, ub = a.view(np.uint64), b.view(np.uint64)
    bad = np.nonzero(ua != ub)[0]
    assert bad.size == 0, f"{what}: {bad.size} words differ, first {bad[:5]}: {a[bad[:5]]} vs {b[bad[:5]]}"


def _states(m, seed):
    """test_gpu_share._states: a random state plus the sign-rule cases, each on a random half of the elements"""
    NE = m.num_ele
    rng = np.random.default_rng(seed)
    zs, zb = np.asarray(m.ele["z_surf"]), np.asarray(m.ele["z_bottom"])
    out = [workload.random_state(m, seed=seed)]
    y = workload.random_state(m, seed=seed + 1)
    half = rng.random(NE) < 0.5
    H = float(np.max(zs)) + 0.25                     # zs/2 <= H <= 2 zs: H - zs and (H - zs) + zs exact
    Hg = float(np.max(zb)) + 5.0
    y[:NE][half] = H - zs[half]                       # equal surface heads: dh == +0 across such edges
    y[2 * NE:3 * NE][half] = Hg - zb[half]            # equal groundwater heads: dhg == +0
    out.append(y)
    y = workload.random_state(m, seed=seed + 2)
    y[:NE][rng.random(NE) < 0.5] = 0.0                # dry cells: ym = 0, no Manning
    low = rng.random(NE) < 0.4
    y[2 * NE:3 * NE][low] = rng.uniform(0.0, 0.02, low.sum())   # the groundwater zero branches
    out.append(y)
    y = workload.random_state(m, seed=seed + 3)
    neg = rng.random(NE) < 0.3
    y[:NE][neg] = -rng.uniform(0.0, 0.1, neg.sum())   # negative surface (MODE 1 clamps it)
    out.append(y)
    return out


def _assert_coverage(m, pub, rcv, what, neither):
    """neither: the numbering leaves elements that share nothing (block_roll: a tile holds parts of two shuffled
    blocks; under `block` every tile is one connected strip of the mesh, and the greedy rule pairs all of it)"""
    e = eval_order(pub, rcv)
    for o in ORDERS:
        assert (e == np.array(o)[:, None]).all(0).sum() >= 100, f"{what}: (nearly) no element evaluated in order {o}"
    p, r = pub >= 0, rcv >= 0
    states = [("publishes only", p & ~r), ("receives only", ~p & r), ("both", p & r)]
    for name, mask in states + ([("neither", ~p & ~r)] if neither else []):
        assert mask.sum() >= 100, f"{what}: (nearly) no element that {name}"
    # boundary edges in every evaluation stage (dist2edge goes back to the reference slot on the open boundary)
    nb = np.asarray(m.nabr).reshape(3, -1)
    for s in range(3):
        assert (nb[e[s], np.arange(m.num_ele)] < 0).any(), f"{what}: no boundary edge evaluated in stage {s}"


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("mesh", MESHES)
def test_all_orders_same_bits_and_oracle(mesh, numbering, mode, oracle_mod, monkeypatch):
    """all six evaluation orders and the publish / receive states (all four under block_roll) in one model: sharing
    on vs off bit for bit over the four state families x 2 stateful calls, and both against the oracle"""
    m, pub, rcv = _model(mesh, numbering)
    _assert_coverage(m, pub, rcv, f"{mesh} {numbering}", neither=numbering == "block_roll")
    a, b = _handles(m, mode, monkeypatch, rcv)
    try:
        o = oracle_mod.OracleRhs(m, mode)
        o.set_step_inputs()
        for si, y in enumerate(_states(m, 70)):
            for c in range(2):
                (ga, ea), (gb, eb) = _run(a, y), _run(b, y)
                ref, code, _, _ = o.eval(0.0, y)
                assert ea == eb and ea["exit_code"] == 0 and code == 0, (ea, eb, code)
                _same_bits(ga, gb, f"{mesh} {numbering} state {si} call {c}")
                assert_close(ga, ref, what=f"{mesh} {numbering} shared, state {si} call {c}")
                assert_close(gb, ref, what=f"{mesh} {numbering} unshared, state {si} call {c}")
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("numbering", NUMBERINGS)
@pytest.mark.parametrize("mesh", MESHES)
def test_per_slot_diagnostics(mesh, numbering, mode, monkeypatch):
    """the diagnostic replay reads the reordered neighbours and geometry: every diagnostic array — the per-slot
    qele_surf / qele_sub in reference slot order and the totals among them — equals the unshared handle's bits"""
    m, pub, rcv = _model(mesh, numbering)
    a, b = _handles(m, mode, monkeypatch, rcv)
    try:
        for si, y in enumerate(_states(m, 90)[:2]):
            (ga, ea), (gb, eb) = _run(a, y), _run(b, y)
            assert ea == eb and ea["exit_code"] == 0, (ea, eb)
            _same_bits(ga, gb, f"state {si}")
            a.refresh_diagnostics()
            b.refresh_diagnostics()
            da, db = a.diagnostics(), b.diagnostics()
            assert set(da) == set(db) and {"qele_surf", "qele_sub", "qele_surf_tot", "qele_sub_tot"} <= set(da)
            assert da["qele_surf"].size == 3 * m.num_ele and da["qele_sub"].size == 3 * m.num_ele
            for k in da:
                _same_bits(da[k], db[k], f"{mesh} {numbering} mode {mode} state {si} diagnostic {k}")
            assert np.count_nonzero(da["qele_surf"]) and np.count_nonzero(da["qele_sub"])
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["nan_surface", "nan_gw", "inf_surface", "inf_gw"])
def test_void_fallback_through_stored_slot_2(kind, mode, monkeypatch):
    """NaN / infinite surface and groundwater heads on both ends of shared edges (inf - inf: a NaN head difference on
    a published edge, which its receiver must evaluate itself as its last stored slot), on the publisher alone and on
    the receiver alone; half of the edges cross a wave.  Same DY bits, same error flags, same first elements."""
    m, pub, rcv = _model("variant", "block")
    NE = m.num_ele
    a, b = _handles(m, mode, monkeypatch, rcv)
    try:
        nb = np.asarray(m.nabr).reshape(3, NE)
        recv = np.nonzero(rcv >= 0)[0]
        pubr = nb[rcv[recv], recv]
        assert (pub[pubr] >= 0).all() and (nb[pub[pubr], pubr] == recv).all()
        cross = (recv % 256) // 64 != (pubr % 256) // 64
        rng = np.random.default_rng(9)
        pick = np.concatenate([rng.choice(np.nonzero(cross)[0], 8, replace=False),
                               rng.choice(np.nonzero(~cross)[0], 8, replace=False)])
        r, p = recv[pick], pubr[pick]
        both = [0, 1, 2, 3, 4, 8, 9, 10, 11, 12]
        ends = np.concatenate([r[both], p[both], p[[5, 6, 13, 14]], r[[7, 15]]])
        y = workload.random_state(m, seed=5)
        bad = np.nan if kind.startswith("nan") else np.inf
        y[(2 * NE if kind.endswith("gw") else 0) + ends] = bad
        for c in range(2):
            (ga, ea), (gb, eb) = _run(a, y), _run(b, y)
            print(kind, mode, c, ea)
            assert ea == eb, (ea, eb)
            _same_bits(ga, gb, f"{kind} mode {mode} call {c}")
    finally:
        a.close()
        b.close()


@functools.lru_cache(maxsize=None)
def _tile_base():
    return cases.variant(3000, seed=5)[0]


@pytest.mark.parametrize("close_boundary", [0, 1])
@pytest.mark.parametrize("ne", [2, 50, 255, 256, 257, 1000])
def test_tile_shapes(ne, close_boundary, monkeypatch):
    """a single tile, a partial last wave, a one-lane last tile (257) and a last tile that is neither; open and closed
    boundary: sharing on vs off bit for bit, both modes"""
    base = _tile_base()
    m = cases._subset(base, np.arange(ne), close_boundary)
    m.bc_tables = dict(base.bc_tables)
    m.finalize()
    rng = np.random.default_rng(ne)
    m2, _ = rn.renumber(m, rot=rn.random_rot(ne, rng))
    pub, rcv = rn.share_assignment(m2)
    for mode in MODES:
        a, b = _handles(m2, mode, monkeypatch, rcv)
        try:
            for si, y in enumerate(_states(m2, 30 + ne)):
                (ga, ea), (gb, eb) = _run(a, y), _run(b, y)
                assert ea == eb, (ea, eb)
                _same_bits(ga, gb, f"NE {ne} close_boundary {close_boundary} mode {mode} state {si}")
        finally:
            a.close()
            b.close()


ELE_DIAGS = ("qele_surf", "qele_sub", "qele_surf_tot", "qele_sub_tot", "q_infil", "q_exfil", "q_recharge")


@pytest.mark.parametrize("rank", [0, 1])
def test_partition_whole_range_launches(rank):
    """the two launches of a partitioned handle that run the ghost instantiation over the reordered interior prefix as
    well — the kernel timer's whole-range launch and the diagnostic replay: owned DY and the per-element / per-slot
    diagnostics bit for bit against the full-mesh handle (the halo placed through the test hook)"""
    rt = _rt()
    m, y = cases.variant(20000, seed=23)
    ep, _ = partition.cpp_partition(m, 2, partition.PART_AUTO)
    lm, part = partition.CppPlan(m, ep, 2, rank).local_model()
    n_own, gid = part.n_own_ele, np.asarray(lm.meta["ele_gid"])
    single = rt.RhsHandle(m)
    single.set_step_inputs()
    h = rt.RhsHandle(lm, partition=part)
    h.set_step_inputs()
    assert h.layout().get("shared_edges", 0) > 0, h.layout()
    ny = 3 * n_own + part.n_own_riv
    ge, gr = partition.ghost_values(y, m, part)
    bufs = [h.device_alloc(8 * ny), h.device_alloc(8 * ny), h.device_alloc(8 * max(1, ge.size)),
            h.device_alloc(8 * max(1, gr.size))]
    try:
        yb, dyb, st_e, st_r = bufs
        if ge.size:
            h.h2d(st_e, ge)
        if gr.size:
            h.h2d(st_r, gr)
        h.debug_halo(d_ele_src=st_e, d_riv_src=st_r)
        h.h2d(yb, partition.local_state(y, m, part))
        for call in range(2):                         # the folded launch, then the timer's whole-range launch
            ref = single.eval(0.0, y)
            if call == 0:
                h.eval_device(0.0, yb, dyb)
            else:
                h.time_kernels(0.0, yb, dyb, 1)
            got = h.d2h(np.zeros(ny), dyb)
            _same_bits(got, partition.local_state(ref, m, part), f"rank {rank} call {call}")
        ds, dl = single.diagnostics(), h.diagnostics()
        for k in ELE_DIAGS:
            if k in abi.DIAG_ELE3:
                want, got = ds[k].reshape(3, -1)[:, gid[:n_own]], dl[k].reshape(3, -1)[:, :n_own]
            else:
                want, got = ds[k][gid[:n_own]], dl[k][:n_own]
            _same_bits(np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(want).reshape(-1),
                       f"rank {rank} diagnostic {k}")
    finally:
        for b in bufs:
            h.device_free(b)
        h.close()
        single.close()


@pytest.mark.parametrize("device_eval", [False, True])
@pytest.mark.parametrize("nranks", [2, 4])
def test_partitioned_handles(nranks, device_eval):
    """a 20,000-element mesh in 2 and 4 parts on one GPU: every rank's owned DY bit for bit against the full-mesh
    handle — the interior prefix stored in evaluation order, the boundary and ghost elements in reference order, as
    two launches (eval_compute) and as the folded launch (the device eval)"""
    m, y = cases.variant(20000, seed=23)
    ep, _ = partition.cpp_partition(m, nranks, partition.PART_AUTO)
    locs = [partition.CppPlan(m, ep, nranks, r).local_model() for r in range(nranks)]
    for mode in MODES:
        tpart._run_ranks(m, [y, workload.random_state(m, seed=8)], locs, mode, ncalls=2, device_eval=device_eval)
