"""Plain numpy fp64 restatement of the integrator's vector kernels (shud-up_amd/csrc/shud_ode_kernels.hip).

Every kernel there uses only IEEE-exact operations without contraction (+, -, *, /, sqrt, fmin, fabs), so the same
expression in the same order in numpy is a bit-exact reference: no tolerance anywhere.

Reductions: device_order_sum / device_order_min restate the device order from its one statement in the source
(shud-up_amd/csrc/shud_reduce.h: block_partial, waves_tree, ordered_total and the comment at its head), not from the
C oracle; tests/test_ode_kernels.py pins them against the oracle's own restatement and against math.fsum.  The
water-balance kernels (shud_wb.hip) sum through the same header, so tests/test_gpu_wb.py and
tests/test_gpu_wb_quad.py hold their basin sums to device_order_sum as well.

Launchers: one function per launcher of shud_ode_dev.h.  Each returns (outputs, accs): outputs maps a vector name
to its new value (zn is the whole (columns, n) slab), accs lists (terms, is_min) per accumulator in slot order —
reduce_accs() turns them into the finalize's results.
"""
import numpy as np

RED_THREADS = 1024      # kRedThreads
FIN_THREADS = 1024      # kFinThreads
FIN_ACC = 4             # kFinAcc
QMAX = 5                # kQMax
MAXL = 32               # kMaxL

# device scalar slots (shud_ode_dev.h enum Slot)
S_EWTMIN, S_NRM, S_RES, S_SIG, S_WN, S_DEL, S_YCOR, S_ETAQM1, S_ETAQP1, S_SCRATCH = range(10)
S_W = 15
S_H0 = 16
S_R0 = S_H0 + MAXL + 1
S_COUNT = S_R0 + MAXL + 1


def grid_blocks(n):
    return max(1, -(-int(n) // RED_THREADS))


def _tree(x, op):
    """x[..., m] (m a power of two) -> lane 0 of the xor butterfly over offsets m/2 .. 1.

    One butterfly stage leaves lane l with x[l] op x[l ^ off]; a op b and b op a are the same bits for + and fmin,
    so lane 0 after all stages is the halving tree: stage `off` combines lane l < off with lane l + off."""
    m = x.shape[-1]
    while m > 1:
        m //= 2
        x = op(x[..., :m], x[..., m:2 * m])
    return x[..., 0]


def block_partials(term, ident, op, accumulated=True):
    """block_partial: thread i holds ident op term[i] (lanes past n: ident); wave64 butterfly (offsets 32 .. 1),
    then the 16 wave results by waves_tree (offsets 8 .. 1).  One partial per block of 1024.
    accumulated=False: the lane holds term[i] itself, as in the water-balance kernels (v = term, not v += term)."""
    term = np.asarray(term, dtype=np.float64)
    nb = grid_blocks(term.size)
    lanes = np.full(nb * RED_THREADS, ident)
    lanes[:term.size] = op(ident, term) if accumulated else term
    waves = _tree(lanes.reshape(nb, RED_THREADS // 64, 64), op)
    return _tree(waves, op)


def finalize(part, ident, op, fin_acc=FIN_ACC):
    """ordered_total: lane t, acc[k] op= part[t + (fin_acc*j + k)*1024] for j = 0, 1, ... (identity past nblk);
    (acc0 op acc1) op (acc2 op acc3); wave butterfly; waves_tree.  fin_acc = 1 is the single-accumulator tree the
    discriminating-power test compares with (not a device order)."""
    span = fin_acc * FIN_THREADS
    trips = max(1, -(-part.size // span))
    p = np.full(trips * span, ident)
    p[:part.size] = part
    p = p.reshape(trips, fin_acc, FIN_THREADS)
    acc = np.full((fin_acc, FIN_THREADS), ident)
    for j in range(trips):
        acc = op(acc, p[j])
    x = op(op(acc[0], acc[1]), op(acc[2], acc[3])) if fin_acc == 4 else acc[0]
    return float(_tree(_tree(x.reshape(FIN_THREADS // 64, 64), op), op))


def device_order_sum(term, fin_acc=FIN_ACC):
    return finalize(block_partials(term, 0.0, np.add), 0.0, np.add, fin_acc)


def device_order_min(term):
    """the same tree with fmin and identity +inf; fmin drops a NaN operand"""
    return finalize(block_partials(term, np.inf, np.fmin), np.inf, np.fmin)


def reduce_accs(accs):
    return [device_order_min(t) if mn else device_order_sum(t) for t, mn in accs]


# ---- sizes and input families shared by tests/test_ode_kernels.py (CPU) and tests/test_gpu_ode_kernels.py ----------
# partial waves, partial blocks, the 256-thread and the 1024-thread grid edges, lanes past n inside waves_tree
SMALL_SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 16 * 1024 + 1]
# nblk = 1024 (acc[0] exactly full), 1025 (first use of acc[1]), 4096 (one full trip), 4097 (second trip, three
# guarded loads), 5122 (second trip with acc[1] live and a ragged tail)
LARGE_SIZES = [1024 * 1024, 1024 * 1024 + 1, 4096 * 1024, 4096 * 1024 + 1, 5121 * 1024 + 389]


def signed_pair(n, seed=11):
    """strongly cancelling dot-product operands: magnitudes over six decades times a sign-symmetric factor, so the
    value of sum(x*y) carries the summation order in many bits.  Two orders still round to the same double about
    one time in three, so the seed is fixed to one for which tests/test_ode_kernels.py's discriminating-power
    assertions hold at every size (the smallest such seed from 7 up)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    y = rng.standard_normal(n)
    return x, y


def integer_entries(n):
    """entry i = 1 + (block of i) mod 7: every partial and every total is an exact integer in any order"""
    return 1.0 + ((np.arange(n) // RED_THREADS) % 7).astype(np.float64)


def integer_counts(n):
    """how many entries of integer_entries(n) hold each value 1..7 (closed form, Python ints)"""
    full, tail = divmod(int(n), RED_THREADS)
    cnt = [RED_THREADS * (full // 7 + (1 if v < full % 7 else 0)) for v in range(7)]
    cnt[full % 7] += tail
    return cnt


def _zeros(n):
    return np.zeros(n)


# ---- launchers ------------------------------------------------------------------------------------------------------
def _ewt_terms(y, rtol, atol):
    t = rtol * np.abs(y) + atol
    w = 1.0 / t
    p = y * w
    return w, [(t, True), (p * p, False)]


def ewt_set(zn0, rtol, atol):
    w, accs = _ewt_terms(zn0, rtol, atol)
    return dict(ewt=w), accs


def _pascal(zn, q, fwd, with_y, pend):
    zn = zn.copy()
    a = [zn[j].copy() for j in range(q + 1)]
    if pend is not None:
        ac, l, r = pend["acor"], pend["l"], pend["r"]
        if pend["j0"] == 0:
            a[0] = l[0] * ac + a[0]
        for j in range(1, q + 1):
            a[j] = l[j] * ac + a[j]
        if pend["resc"]:
            for j in range(1, q + 1):
                a[j] = a[j] * r[j]
    for k in range(1, q + 1):
        for j in range(q, k - 1, -1):
            a[j - 1] = a[j - 1] + a[j] if fwd else a[j - 1] - a[j]
    for j in range(q):
        zn[j] = a[j]
    if pend is not None:
        zn[q] = a[q]
        if pend["copy_to"] >= 0:
            zn[pend["copy_to"]] = pend["acor"]
    out = dict(zn=zn)
    if fwd and with_y:
        out["y"] = a[0] + 0.0
    return out, []


def predict(zn, q, with_y):
    return _pascal(zn, q, True, with_y, None)


def predict_pend(zn, q, with_y, acor, l, r, j0, resc, copy_to):
    return _pascal(zn, q, True, with_y, dict(acor=acor, l=l, r=r, j0=j0, resc=resc, copy_to=copy_to))


def restore(zn, q):
    return _pascal(zn, q, False, False, None)


def rescale(zn, q, c):
    zn = zn.copy()
    for j in range(1, q + 1):
        zn[j] = zn[j] * c[j]
    return dict(zn=zn), []


def vsum(x, y):
    return dict(z=x + y), []


def vsum_zero(x):
    return dict(ycor=_zeros(x.size), z=x + 0.0), []


def scale_to(c, x):
    return dict(z=c * x), []


def axpy_multi(zn, src, coef, jlo, jhi):
    zn = zn.copy()
    for j in range(jlo, jhi + 1):
        zn[j] = coef[j] * zn[src] + zn[j]
    return dict(zn=zn), []


def residual(zn1, ycor, ftemp, rl1, ngamma, ewt):
    r1 = rl1 * zn1 + (0.0 if ycor is None else ycor)
    r2 = r1 + ngamma * ftemp
    d = -r2
    p = d * ewt
    return dict(delta=d), [(p * p, False)]


def krylov_v0(delta, ewt, c):
    x = c * (ewt * delta)
    p = (x / ewt) * ewt
    return dict(V0=x), [(p * p, False)]


def dq_sig(ds, n):
    return 1.0 / np.sqrt(np.float64(ds[S_SIG]) / np.float64(n))


def dq_work(V, ewt, y, ds):
    sig = dq_sig(ds, V.size)
    return dict(work=sig * (V / ewt) + y), []


def atimes(w, fy, V, ewt, V0, ngamma, ds):
    sig = dq_sig(ds, w.size)
    siginv = 1.0 / sig
    jv = siginv * (w - fy)
    z = ngamma * jv + V / ewt
    x = ewt * z
    return dict(w=x), [(x * x, False), (V0 * x, False)]


def mgs(w, Vprev, ds, hslot, Vnext):
    x = w
    out = {}
    if Vprev is not None:
        nh = -np.float64(ds[hslot])
        x = x + nh * Vprev
        out["w"] = x
    return out, [(Vnext * x if Vnext is not None else x * x, False)]


def normalize(w, c, ewt):
    x = w * c
    p = (x / ewt) * ewt
    return dict(w=x), [(p * p, False)]


def newton_update(V, krydim, yg, dsrc, ewt, ycor, ycor_zero):
    n = ewt.size
    if krydim > 0:
        xc = _zeros(n)
        for k in range(krydim):
            xc = xc + yg[k] * V[k]
        d = xc / ewt
    else:
        d = _zeros(n) if dsrc is None else dsrc
    yc = (_zeros(n) if ycor_zero else ycor) + d
    p, q = d * ewt, yc * ewt
    return dict(ycor=yc), [(p * p, False), (q * q, False)]


def complete_step(zn, acor, l, jlo, q, copy_to):
    zn = zn.copy()
    for j in range(jlo, q + 1):
        zn[j] = l[j] * acor + zn[j]
    if copy_to >= 0:
        zn[copy_to] = acor
    return dict(zn=zn), []


def complete_step_ewt(zn, acor, l, q, copy_to, jst, rtol, atol):
    zn = zn.copy()
    z0 = None
    for j in range(q + 1):
        z = l[j] * acor + zn[j]
        if j >= jst:
            zn[j] = z
        if j == 0:
            z0 = z
    if copy_to >= 0:
        zn[copy_to] = acor
    w, accs = _ewt_terms(z0, rtol, atol)
    return dict(zn=zn, ewt_next=w), accs


def eta_norms(znq, znqmax, acor, ncquot, ewt, pend_q, lq):
    n = ewt.size
    t0, t1 = _zeros(n), _zeros(n)
    if znq is not None:
        zq = lq * acor + znq if pend_q else znq
        p = zq * ewt
        t0 = p * p
    if znqmax is not None:
        p = (ncquot * znqmax + acor) * ewt
        t1 = p * p
    return {}, [(t0, False), (t1, False)]


def lin_sum2(a, x, b, y):
    """N_VLinearSum_Serial's case analysis for z distinct from x and y"""
    if a == 1.0 and b == 1.0:
        return x + y
    if a == 1.0 and b == -1.0:
        return x - y
    if a == -1.0 and b == 1.0:
        return y - x
    if a == 1.0:
        return (b * y) + x
    if b == 1.0:
        return (a * x) + y
    if a == -1.0:
        return (b * y) - x
    if b == -1.0:
        return (a * x) - y
    if a == b:
        return a * (x + y)
    if a == -b:
        return a * (x - y)
    return (a * x) + (b * y)


def dky(zn, js, c, nvec, rscale, pend=None):
    """pend: None or dict(acor, l, j0, q) — zn[j], j0 <= j <= q, taken as l[j]*acor + zn[j]"""
    def Z(j):
        if pend is not None and pend["j0"] <= j <= pend["q"]:
            return pend["l"][j] * pend["acor"] + zn[j]
        return zn[j]
    if nvec == 1:
        z = c[0] * Z(js[0])
    elif nvec == 2:
        z = lin_sum2(c[0], Z(js[0]), c[1], Z(js[1]))
    else:
        z = c[0] * Z(js[0])
        for k in range(1, nvec):
            z = z + c[k] * Z(js[k])
    if rscale != 0.0:
        z = z * rscale
    return dict(out=z), []
