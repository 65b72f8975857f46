"""Renumbering of a ShudModel: the same mesh, rivers and segments under another numbering.

The C-ABI promises nothing about numbering (include/shud_rhs.h: "reference order"), and the kernels' host tables
(the in-tile edge-sharing assignment, the element-sorted and reach-sorted segment streams, the junction lists) all
follow from it.  `renumber` permutes elements, reaches and segments and rotates each element's three edge slots;
`share_assignment` and `eval_order` restate the host's edge-sharing rule (shud_tables.cpp share_plan) in numpy, so that
tests can state which sharing states an input reaches and check the host's plan itself (test_tables.py).

Conventions: new element k is old pe[k], new reach k is old pr[k], new segment k is old ps[k]; new edge slot j of
new element k is old slot (j + rot[k]) % 3 of old element pe[k].
"""
import copy

import numpy as np

from shud_rhs import abi


class Numbering:
    """the four maps of one renumbering, with the helpers that carry vectors between the two numberings"""

    def __init__(self, m, pe=None, pr=None, ps=None, rot=None):
        NE, NR, NS = m.num_ele, m.num_riv, m.num_seg
        self.NE, self.NR, self.NS, self.NL = NE, NR, NS, getattr(m, "num_lake", 0)
        self.pe = np.arange(NE) if pe is None else np.asarray(pe, dtype=np.int64)
        self.pr = np.arange(NR) if pr is None else np.asarray(pr, dtype=np.int64)
        self.ps = np.arange(NS) if ps is None else np.asarray(ps, dtype=np.int64)
        self.rot = np.zeros(NE, dtype=np.int64) if rot is None else np.asarray(rot, dtype=np.int64)
        for p, n in ((self.pe, NE), (self.pr, NR), (self.ps, NS)):
            assert p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n)), "not a permutation"
        assert self.rot.shape == (NE,) and ((self.rot >= 0) & (self.rot <= 2)).all()
        self.inv_e, self.inv_r, self.inv_s = (_inverse(p) for p in (self.pe, self.pr, self.ps))
        # old slot of every new (slot, element)
        self.slot = (np.arange(3)[:, None] + self.rot[None, :]) % 3

    # ---- old numbering -> new numbering ----
    def ele(self, a):
        return np.asarray(a)[self.pe]

    def edge(self, a):
        """a [3*NE] edge-major array: elements permuted, each element's slots rotated"""
        a3 = np.asarray(a).reshape(3, self.NE)
        return a3[self.slot, self.pe[None, :]].reshape(-1)

    def riv(self, a):
        return np.asarray(a)[self.pr]

    def seg(self, a):
        return np.asarray(a)[self.ps]

    def map_y(self, y):
        """a state or DY vector [sf|us|gw|riv|lake], block by block; lake entries unchanged"""
        y = np.asarray(y)
        NE, NR = self.NE, self.NR
        assert y.size == 3 * NE + NR + self.NL
        return np.concatenate([y[:NE][self.pe], y[NE:2 * NE][self.pe], y[2 * NE:3 * NE][self.pe],
                               y[3 * NE:3 * NE + NR][self.pr], y[3 * NE + NR:]])

    # ---- new numbering -> old numbering (diagnostics of the renumbered model, to compare in the old order) ----
    def unmap_ele(self, a):
        return np.asarray(a)[self.inv_e]

    def unmap_edge(self, a):
        out = np.empty((3, self.NE), dtype=np.asarray(a).dtype)
        out[self.slot, self.pe[None, :]] = np.asarray(a).reshape(3, self.NE)
        return out.reshape(-1)

    def unmap_riv(self, a):
        return np.asarray(a)[self.inv_r]

    def unmap_seg(self, a):
        return np.asarray(a)[self.inv_s]

    def unmap_y(self, y):
        y = np.asarray(y)
        NE, NR = self.NE, self.NR
        return np.concatenate([y[:NE][self.inv_e], y[NE:2 * NE][self.inv_e], y[2 * NE:3 * NE][self.inv_e],
                               y[3 * NE:3 * NE + NR][self.inv_r], y[3 * NE + NR:]])

    def unmap_diag(self, name, a):
        """a ShudFluxOut array of the renumbered model, by its kind (abi.DIAG_*)"""
        if name in abi.DIAG_ELE3:
            return self.unmap_edge(a)
        if name in abi.DIAG_SEG:
            return self.unmap_seg(a)
        if name in abi.DIAG_RIV:
            return self.unmap_riv(a)
        if name in abi.DIAG_LAKE:
            return np.asarray(a)
        return self.unmap_ele(a)

    def inverse_args(self):
        """renumber(m2, **inverse_args()) returns m"""
        return dict(pe=self.inv_e, pr=self.inv_r, ps=self.inv_s, rot=(-self.rot[self.inv_e]) % 3)


def _inverse(p):
    inv = np.empty(p.size, dtype=np.int64)
    inv[p] = np.arange(p.size)
    return inv


def _remap(v, inv):
    """indices through the inverse map; negative codes (boundary, outlet kinds) kept"""
    v = np.asarray(v)
    return np.where(v >= 0, inv[np.maximum(v, 0)], v).astype(v.dtype) if inv.size else v.copy()


def renumber(m, pe=None, pr=None, ps=None, rot=None):
    """-> (deep copy of m under the new numbering, map_y).  map_y carries the Numbering as map_y.__self__."""
    nb = Numbering(m, pe, pr, ps, rot)
    NE = m.num_ele
    r = copy.deepcopy(m)                        # bc_tables, lake bathymetry, meta, sizes: unchanged
    for k, v in m.ele.items():
        r.ele[k] = nb.edge(v) if np.asarray(v).size == 3 * NE else nb.ele(v)
    r.nabr = _remap(nb.edge(m.nabr), nb.inv_e)
    for k in ("ibc", "iss", "ilake"):
        if getattr(m, k) is not None:
            setattr(r, k, nb.ele(getattr(m, k)))
    r.par = {k: nb.ele(v) for k, v in m.par.items()}
    r.step = {k: nb.ele(v) for k, v in m.step.items()}          # every step array is [NE]
    r.riv = {k: nb.riv(v) for k, v in m.riv.items()}
    r.riv_bc = nb.riv(m.riv_bc)
    r.riv_down = _remap(nb.riv(m.riv_down), nb.inv_r)
    r.seg_ele = _remap(nb.seg(m.seg_ele), nb.inv_e)
    r.seg_riv = _remap(nb.seg(m.seg_riv), nb.inv_r)
    r.seg_length = nb.seg(m.seg_length)
    r.seg_cwr = nb.seg(m.seg_cwr)
    for k in ("x", "y"):                        # element centroids (the partitioner's coordinates), where present
        if k in m.meta and np.asarray(m.meta[k]).shape == (NE,):
            r.meta[k] = nb.ele(m.meta[k])
    return r.finalize(), nb.map_y


# ---- named numberings ----
def block_shuffle(NE, rng, tile=256):
    """elements shuffled inside each consecutive block of `tile`: every tile keeps its set of elements"""
    p = np.arange(NE)
    for s in range(0, NE, tile):
        rng.shuffle(p[s:s + tile])
    return p


def random_perm(n, rng):
    return rng.permutation(n)


def roll(NE, k):
    """new element i is old (i + k) % NE: the tile boundaries land elsewhere in the mesh"""
    return (np.arange(NE) + k) % NE


def random_rot(NE, rng):
    return rng.integers(0, 3, NE)


def full_numbering(m, rng):
    """pe, pr, ps and rot all drawn: segments sorted neither by reach nor by element"""
    return dict(pe=random_perm(m.num_ele, rng), pr=random_perm(m.num_riv, rng), ps=random_perm(m.num_seg, rng),
                rot=random_rot(m.num_ele, rng))


# ---- the inputs of the GPU sharing tests (test_gpu_renumber.py), whose coverage test_renumber.py asserts ----
SHARE_MESHES = {"v3000": (3000, 5), "v20000": (20000, 43)}          # cases.variant(n, seed)
SHARE_NUMBERINGS = ("block", "block_roll")


def share_numbering(NE, numbering, seed):
    """block: block_shuffle + a rotation per element (tile-local numbering, every tile keeps its elements);
    block_roll: the same, then rolled by 101, so that every tile holds parts of two shuffled blocks"""
    rng = np.random.default_rng(seed)
    pe, rot = block_shuffle(NE, rng), random_rot(NE, rng)
    if numbering == "block_roll":
        pe = pe[roll(NE, 101)]
    return dict(pe=pe, rot=rot)


def share_input(mesh, numbering):
    """-> (renumbered model, its variant state in the new numbering); seeds fixed (test_renumber.py asserts what the
    assignment on these inputs covers)"""
    import cases
    n, seed = SHARE_MESHES[mesh]
    m, y = cases.variant(n, seed=seed)
    m2, map_y = renumber(m, **share_numbering(m.num_ele, numbering, 1000 + seed))
    return m2, map_y(y)


# ---- the host's in-tile edge-sharing assignment, restated ----
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def share_assignment(m, lim=None, tile=256):
    """(pub, rcv): per element the edge slot it publishes and the slot it receives, -1 for none.

    Greedy in element order over elements [0, lim).  Element i receives its first slot k whose neighbour v is
    another element below lim in the same tile that publishes nothing yet, names i in exactly one of its own slots
    kk, has the same edge, dist2nabor, depression and avg_rough bits across the edge (avg_rough positive and
    finite), with neither a lake element, and i does not itself publish slot k (never both directions of one
    edge).  Then v publishes kk and i receives k: at most one of each per element."""
    NE = m.num_ele
    lim = NE if lim is None else lim
    nabr = np.asarray(m.nabr).reshape(3, NE)
    edge, d2n, ar = (_bits(m.ele[k]).reshape(3, NE) for k in ("edge", "dist2nabor", "avg_rough"))
    arv = np.asarray(m.ele["avg_rough"], dtype=np.float64).reshape(3, NE)
    dep = _bits(m.ele["depression"]) if "depression" in m.ele else np.zeros(NE, dtype=np.uint64)
    lake = np.asarray(m.ilake) > 0 if m.ilake is not None else np.zeros(NE, dtype=bool)
    pub, rcv = np.full(NE, -1, dtype=np.int8), np.full(NE, -1, dtype=np.int8)
    for i in range(lim):
        for k in range(3):
            if rcv[i] >= 0:
                break
            v = int(nabr[k, i])
            if v < 0 or v >= lim or v == i or v // tile != i // tile or pub[v] >= 0:
                continue
            back = np.nonzero(nabr[:, v] == i)[0]
            if back.size != 1 or pub[i] == k:
                continue
            kk = int(back[0])
            a = arv[k, i]
            if (edge[k, i] != edge[kk, v] or d2n[k, i] != d2n[kk, v] or dep[i] != dep[v] or ar[k, i] != ar[kk, v]
                    or not (a > 0.0 and np.isfinite(a)) or lake[i] or lake[v]):
                continue
            pub[v] = kk
            rcv[i] = k
    return pub, rcv


def eval_order(pub, rcv):
    """[3, NE]: the reference slot evaluated first, second and last (the host's rule): first the published slot,
    else the lowest slot that is not the received one; last the received slot, else the highest remaining one"""
    pub, rcv = np.asarray(pub, dtype=np.int64), np.asarray(rcv, dtype=np.int64)
    e0 = np.where(pub >= 0, pub, np.where(rcv == 0, 1, 0))
    e2 = np.where(rcv >= 0, rcv, np.where(e0 == 2, 1, 2))
    return np.stack([e0, 3 - e0 - e2, e2])


def share_stats(m, pub, rcv, wave=64, tile=256):
    """what an assignment covers: counts of the 13 (pub, rcv) states, the share of shared edges whose publisher and
    receiver sit in different waves of the tile, and the share with publisher index < receiver index"""
    NE = m.num_ele
    states = {}
    for p in (-1, 0, 1, 2):
        for r in (-1, 0, 1, 2):
            if p == r and p >= 0:
                continue
            states[(p, r)] = int(((pub == p) & (rcv == r)).sum())
    recv = np.nonzero(rcv >= 0)[0]
    pubr = np.asarray(m.nabr).reshape(3, NE)[rcv[recv], recv]
    cross = ((recv % tile) // wave) != ((pubr % tile) // wave)
    n = max(1, recv.size)
    return dict(shared=int(recv.size), states=states, cross_wave=float(cross.sum()) / n,
                pub_below=float((pubr < recv).sum()) / n, pub_above=float((pubr > recv).sum()) / n,
                last_tile_partial=NE % tile != 0)
