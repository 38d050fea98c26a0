"""Helpers of the dual-step shape tests (test infrastructure, no GPU needed to import):

  synth_round   the state in FRONT of one round of the dual step, written by hand: exact bundle sizes, slots in random order, NaN
                in everything the kernel must not read, the current y and the new cut (f, g)
  one_round     the body of oracle.solve_batch's sample loop on such a state, with the oracle's own simplex_newton,
                interior_point and numpy.linalg.matrix_rank: the expected outcome of the round
  perturbed     the same state with h and f moved by a relative 1e-15 (one float64 rounding): how far the oracle itself moves
  CASES         the instance / bundle-size / row-width table of tests/test_dual_step_shapes.py

One round is a pure function of the bundle: the reference restarts Newton from lam = 1/k in every outer iteration
(oracle/bundle_entropy_oracle.py simplex_newton, interior_point), so a state written by hand has an exact expected outcome.
"""
import functools
import zlib

import numpy as np

from icnn_amd._lib import FLAG_F64_ENERGY, FLAG_GLOBAL_BUNDLE, FLAG_MFMA_CONTRACTION, FLAG_WAVE_PER_SAMPLE
from oracle import bundle_entropy_oracle as oracle

LD = np.longdouble
F32, F64 = np.float32, np.float64
SCALES = (1.0, 0.3, 0.05)          # mixed inside a batch: pruning happens without being constructed
CONTROL = ("count", "n_iters", "finished", "status", "newton_iters", "t_next", "phase", "skip_fg")
NEWTON_CAP = {"dual": 100, "rl": 20, "pdipm": 20}     # oracle.VARIANTS[*].newton_cap; interior_point's range(20)


class RoundState:
    """Host arrays of a BundleState in front of round t (struct icnn_be_state) + the round's new cut: y [B, n], G [B, slots, n]
    in the cut dtype, h / lam / fvals [B, slots], ys [B, slots, n], active [B, slots], the control words [B], f [B], g [B, n];
    kind[u]: 'live', 'fin' (finished = 1), 'dup' (the new cut repeats an active cut), 'zero' (k = 1, g = 0)."""

    ARRAYS = ("y", "G", "h", "ys", "lam", "active", "fvals") + CONTROL

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def copy(self):
        kw = dict(self.__dict__)
        for name in self.ARRAYS + ("f", "g"):
            kw[name] = kw[name].copy()
        return RoundState(**kw)

    def to_device(self, flags=0):
        """BundleState whose tensors hold this state, and (f, g) on the device (needs the GPU).  park and the staging area are
        filled with NaN bit patterns: nothing may be read there before it is written."""
        import torch
        from icnn_amd import bundle_entropy
        y = torch.from_numpy(self.y.copy()).cuda()
        st = bundle_entropy.BundleState(y, self.iters if self.iters else self.slots, self.variant,
                                        torch.float64 if self.cut_dtype == F64 else torch.float32, flags, self.slots)
        assert st.T == self.slots and st.c_state.iters == self.iters
        for name in ("G", "h", "ys", "lam", "active", "fvals"):
            getattr(st, name).copy_(torch.from_numpy(getattr(self, name)))
        for name in CONTROL:
            getattr(st, name)[:self.B].copy_(torch.from_numpy(getattr(self, name)))
        st.park.fill_(float("nan"))
        if st.scratch is not None:
            st.scratch.fill_(0xFF)
        return st, torch.from_numpy(self.f.copy()).cuda(), torch.from_numpy(self.g.copy()).cuda()


def _sample_rng(seed, u, bump):
    return np.random.RandomState([seed, u, bump])


def full_bundle(rng, n, cnt, cut_dtype, c, sigma):
    """cnt + 1 cuts that survive the round: tangents of phi(y) = c/2 |y - ybar|^2, ybar uniform in [0.2, 0.8]^n, at points
    y* + sigma randn clipped to [0.01, 0.99], y* the minimiser of phi - H (Newton on c (y - ybar) + logit(y) = 0).  Cuts of one
    strongly convex function taken around the round's own solution all carry weight there, where random cuts prune each other.
    Returns (points [cnt + 1, n], g = c (p - ybar) in the cut dtype, h = phi(p) - <g, p>, phi(p)); the last is the round's."""
    ybar = 0.2 + 0.6 * rng.rand(n)
    ystar = np.full(n, 0.5)
    for _ in range(60):
        ystar = np.clip(ystar - (c * (ystar - ybar) + np.log(ystar / (1 - ystar))) / (c + 1 / (ystar * (1 - ystar))), 1e-9, 1 - 1e-9)
    pts = np.clip(ystar + sigma * rng.randn(cnt + 1, n), 0.01, 0.99)
    g = (c * (pts - ybar)).astype(cut_dtype)
    phi = 0.5 * c * np.sum((pts - ybar) ** 2, axis=1)
    return pts, g, phi - np.sum(g.astype(F64) * pts, axis=1), phi


def synth_round(seed, n, slots, cut_dtype, variant, t, ks, iters=0, f64_energy=False, reseed=(), full=None):
    """The state in front of round t.  ks[u] is the bundle size k the round works on (count = k - 1 older cuts + the new one), or
    (kind, k) for a special sample.  The older cuts sit in a random subset of the slots 0..t-1 in random order -- with iters >
    slots in a random subset of ALL slots, so that the new cut must take the lowest free one.  G = scale randn in the cut dtype,
    ys uniform, h = 0.3 randn at those slots; NaN in every other slot of G, ys, h, fvals and in all of lam; active[u, count:]
    repeats an inactive slot.  Every sample has its own RandomState([seed, u, bump]), bump = dict(reseed).get(u, 0).
    full = (c, sigma): the live samples' cuts, points and energies are full_bundle's instead -- bundles that stay full."""
    cut_dtype = np.dtype(cut_dtype).type
    f_dtype = F64 if (f64_energy or cut_dtype == F64) else F32
    B = len(ks)
    bumps = dict(reseed)
    G = np.full((B, slots, n), np.nan, dtype=cut_dtype)
    ys = np.full((B, slots, n), np.nan)
    h = np.full((B, slots), np.nan)
    fvals = np.full((B, slots), np.nan)
    lam = np.full((B, slots), np.nan)
    active = np.zeros((B, slots), dtype=np.int32)
    y = np.empty((B, n))
    g = np.empty((B, n), dtype=cut_dtype)
    f = np.empty(B, dtype=f_dtype)
    count = np.zeros(B, dtype=np.int32)
    finished = np.zeros(B, dtype=np.int32)
    kinds = []
    pool = slots if iters > slots else t
    assert 0 <= t < (iters if iters else slots)
    for u, spec in enumerate(ks):
        kind, k = spec if isinstance(spec, tuple) else ("live", spec)
        rng = _sample_rng(seed, u, bumps.get(u, 0))
        cnt = k - 1
        assert 0 <= cnt <= min(pool, slots - 1), (u, k, pool)
        scale = SCALES[(u + bumps.get(u, 0)) % len(SCALES)]
        perm = rng.permutation(pool)
        own = perm[:cnt]
        free = np.setdiff1d(np.arange(slots), own)
        active[u, :cnt] = own
        active[u, cnt:] = free[-1]
        G[u, own] = (scale * rng.randn(cnt, n)).astype(cut_dtype)
        ys[u, own] = rng.rand(cnt, n)
        h[u, own] = 0.3 * rng.randn(cnt)
        fvals[u, own] = rng.randn(cnt)
        y[u] = 0.05 + 0.9 * rng.rand(n)
        g[u] = (scale * rng.randn(n)).astype(cut_dtype)
        f[u] = f_dtype(rng.randn())
        if full is not None and kind == "live":
            pts, g_all, h_all, phi = full_bundle(rng, n, cnt, cut_dtype, *full)
            G[u, own], ys[u, own], h[u, own], fvals[u, own] = g_all[:cnt], pts[:cnt], h_all[:cnt], phi[:cnt]
            y[u], g[u], f[u] = pts[cnt], g_all[cnt], f_dtype(phi[cnt])
        if kind == "dup":
            assert cnt >= 1
            g[u] = G[u, own[rng.randint(cnt)]]
        elif kind == "zero":
            assert cnt == 0
            g[u] = 0
        elif kind == "fin":
            finished[u] = 1
        else:
            assert kind == "live"
        count[u] = cnt
        kinds.append(kind)
    full = iters if iters else slots
    return RoundState(B=B, n=n, slots=slots, cut_dtype=cut_dtype, variant=variant, t=t, iters=iters, kind=kinds,
                      y=y, G=G, h=h, ys=ys, lam=lam, active=active, fvals=fvals, f=f, g=g,
                      count=count, n_iters=np.full(B, full, dtype=np.int32), finished=finished,
                      status=np.zeros(B, dtype=np.int32), newton_iters=np.zeros(B, dtype=np.int32),
                      t_next=np.full(B, t, dtype=np.int32), phase=np.zeros(B, dtype=np.int32),
                      skip_fg=np.zeros(B, dtype=np.int32))


def new_slot(s, u):
    """slot the round's cut of sample u goes to: t, or with more iterations than slots the lowest slot not in the active list
    (be_dual_dev.h dual_step_body, 'Slot of the new cut')"""
    if s.iters <= s.slots:
        return s.t
    used = set(s.active[u, :s.count[u]].tolist())
    return min(i for i in range(s.slots) if i not in used)


def one_round(s, variant=None):
    """Round t of oracle.solve_batch's sample loop (:294-330) on the state s, slot-addressed like the device.  Returns a dict of
    per-sample lists / arrays: y [B, n], lam / active (the pruned bundle, bundle order), count, finished, n_iters, slot (of the
    new cut), G_new / h_new / ys_new (what the slot holds afterwards; None for a finished sample), newton (updates of the inner
    solve, None where none ran), lam_full / slots_full (multipliers of ALL k cuts before pruning; None where no solve ran)."""
    variant = variant or s.variant
    rules = oracle.VARIANTS[variant]
    y = s.y.copy()
    off = s.f - np.sum(s.g * s.y, axis=1)                    # dual :143 for the whole batch, as solve_batch forms it
    out = dict(y=y, lam=[], active=[], count=np.zeros(s.B, dtype=np.int32), finished=s.finished.copy(),
               n_iters=s.n_iters.copy(), slot=[], G_new=[], h_new=[], ys_new=[], newton=[], lam_full=[], slots_full=[])
    for u in range(s.B):
        cnt = int(s.count[u])
        old = [int(v) for v in s.active[u, :cnt]]
        if s.finished[u]:
            for key, val in (("lam", s.lam[u, :cnt].copy()), ("active", old), ("slot", None), ("G_new", None), ("h_new", None),
                             ("ys_new", None), ("newton", None), ("lam_full", None), ("slots_full", None)):
                out[key].append(val)
            out["count"][u] = cnt
            continue
        slot = new_slot(s, u)
        G_u, h_u = s.G[u].copy(), s.h[u].copy()
        G_u[slot] = s.g[u]
        h_u[slot] = off[u]
        out["slot"].append(slot)
        out["G_new"].append(s.g[u].copy())
        out["h_new"].append(off[u])
        out["ys_new"].append(s.y[u].copy())
        slots = old + [slot]
        stats = []

        def keep_old():
            out["lam"].append(s.lam[u, :cnt].copy())
            out["active"].append(old)
            out["count"][u] = cnt
            out["newton"].append(None)
            out["lam_full"].append(None)
            out["slots_full"].append(None)

        if rules.rank_test and np.linalg.matrix_rank(G_u[slots]) < len(slots):      # dual :155-161
            out["finished"][u] = 1
            out["n_iters"][u] = s.t - 1
            keep_old()
            continue
        Au = G_u[slots]
        hu = h_u[slots]
        if rules.ipm:
            y[u], lam_u = oracle.interior_point(Au, hu, stats)
            pos = lam_u > oracle._IPM_PRUNE
        else:
            before = y[u].copy()
            if len(slots) > 1:
                lam_u = oracle.simplex_newton(Au, hu, rules, stats)
                y[u] = 1 / (1 + np.exp(Au.T.dot(lam_u)))
            else:
                lam_u = np.array([1.0])
                y[u] = 1 / (1 + np.exp(Au[0]))
            if rules.clip is not None:
                y[u] = np.clip(y[u], rules.clip[0], rules.clip[1])
            if rules.stall_tol is not None and max(abs(before - y[u])) < rules.stall_tol:
                out["finished"][u] = 1
            pos = lam_u > 0
        out["lam"].append(np.asarray(lam_u, dtype=np.float64)[pos])
        out["active"].append([sl for sl, p in zip(slots, pos) if p])
        out["count"][u] = int(np.sum(pos))
        out["newton"].append(stats[0] if stats else None)
        out["lam_full"].append(np.asarray(lam_u, dtype=np.float64))
        out["slots_full"].append(slots)
    return out


def perturbed(s, seed):
    """s with every active h and the new cut's f multiplied by 1 + 1e-15 randn: one float64 rounding on the round's inputs"""
    rng = np.random.RandomState(seed)
    p = s.copy()
    p.h = s.h * (1.0 + 1e-15 * rng.randn(*s.h.shape))
    p.f = s.f.astype(np.float64) * (1.0 + 1e-15 * rng.randn(s.B))
    return p


def bundle_of(s, ref, u):
    """(A, h) of the k cuts sample u's round works on, in the order of ref['slots_full'][u]: the older active cuts, then the new"""
    slots = ref["slots_full"][u]
    A = np.concatenate([s.G[u, slots[:-1]], ref["G_new"][u][None]])
    return A, np.concatenate([s.h[u, slots[:-1]], [ref["h_new"][u]]])


def reduced_gradient(A, h, lam_full):
    """At the multipliers lam_full of ALL k cuts (zeros where pruned), in longdouble: c as the oracle forms it (row sums in the
    cut dtype, simplex_newton :97), grad = -c + A sigmoid(A^T lam) (:107), g0 = grad - grad[argmax lam] (:115).  Returns (norm of
    g0 over the surviving cuts, g0 of the pruned cuts)."""
    c = (np.sum(A, axis=1) + h).astype(LD)
    Al, lam = A.astype(LD), np.asarray(lam_full, dtype=LD)
    z = 1 / (1 + np.exp(-(Al.T.dot(lam))))
    grad = -c + Al.dot(z)
    g0 = grad - grad[int(np.argmax(lam_full))]
    alive = np.asarray(lam_full) > 0
    return float(np.sqrt(np.sum(g0[alive] ** 2))), np.asarray(g0[~alive], dtype=np.float64)


def newton_trace(A, b, rules):
    """oracle.simplex_newton once more, statement for statement, with one addition: the smallest distance from zero that a
    multiplier had BEFORE the clip at zero (:139) or the pivot's 1 - sum (:142) decided its value, over all accepted iterates.
    Where that distance is at the rounding level, whether the cut ends at exactly zero -- and is pruned -- or at 1e-17 depends on
    the order of a summation: the reference's outcome is then not a function of the bundle.  Returns (lam, margin);
    tests/test_dual_step_shapes.py checks lam against the oracle's bit for bit, so this is a trace of the oracle, not a second
    opinion."""
    k = A.shape[0]
    c = np.sum(A, axis=1) + b
    lam = np.ones(k) / k
    keep = np.ones(k)
    margin = np.inf
    for _ in range(rules.newton_cap):
        a = A.T.dot(lam)
        z = 1 / (1 + np.exp(-a))
        fval = -c.dot(lam) + np.sum(oracle.softplus_stable(a))
        grad = -c + A.dot(z)
        hess = (A * (z * (1 - z))).dot(A.T)
        piv = np.argmax(lam)
        red = lam.copy()
        red[piv] = 1
        keep[piv] = 0
        col = hess[:, piv]
        g0 = grad - keep * grad[piv]
        h0 = (hess - keep[:, None] * col[None, :] - col[:, None] * keep[None, :]
              + hess[piv, piv] * (keep[:, None] * keep[None, :]))
        bound = (red <= oracle._BOUND_EPS) & (g0 > 0)
        bound[piv] = True
        free = ~bound
        if np.linalg.norm(g0[free]) < oracle._GRAD_TOL:
            return lam, margin
        step = np.zeros(k)
        try:
            step[free] = np.linalg.solve(h0[free, :][:, free], -g0[free])
        except np.linalg.LinAlgError:
            if rules.singular_raises:
                raise
            break
        t = min(1. / np.max(abs(step)), 1.) if rules.scaled_first_step else 1.
        done = False
        for _ in range(rules.backoff_cap):
            raw = red + t * step
            trial = np.maximum(raw, 0)
            trial[piv] = 1
            lam_new = trial.copy()
            lam_new[piv] = 1. - keep.dot(trial)
            if lam_new[piv] >= 0:
                if rules.armijo:
                    if oracle._dual_objective(c, A, lam_new) < fval + t * oracle._ARMIJO_ALPHA * step.dot(g0):
                        break
                else:
                    break
            if rules.tiny_step_on_td:
                if max(t * abs(step)) < oracle._TINY:
                    done = True
                    break
            elif t < oracle._TINY:
                done = True
                break
            t *= oracle._SHRINK
        moved = free.copy()
        moved[piv] = False
        margin = min([margin, abs(lam_new[piv])] + list(np.abs(raw[moved])))
        if done:
            return lam_new, margin
        keep[piv] = 1.
        lam = lam_new.copy()
    return lam, margin


def objective_noise_runs(s):
    """one_round of s with every softplus term of the oracle's objective (the Armijo test of variant rl, :145-146) moved by a
    relative 1e-15: ramps of either sign and two random draws.  The Newton system is untouched, so only a line search decided
    at the rounding level of the objective changes the outcome."""
    orig = oracle.softplus_stable
    runs = []
    try:
        for d in range(4):
            rng = np.random.RandomState(900 + d)
            if d < 2:
                oracle.softplus_stable = lambda v, sign=1 - 2 * d: orig(v) * (1 + sign * 1e-15 * np.linspace(0, 1, v.size).reshape(v.shape))
            else:
                oracle.softplus_stable = lambda v, rng=rng: orig(v) * (1 + 1e-15 * rng.randn(*v.shape))
            with np.errstate(all="ignore"):
                runs.append(one_round(s))
    finally:
        oracle.softplus_stable = orig
    return runs


# ---- which routine forms H | A z (dual) or M | G Hinv ry (pdipm) for a sample: the kernels' own width conditions, restated ------
HV_K1MAX, HV_KMAX, IPM_KMAX, IPM_KMAX_WAVES, WIDE_LR = 8, 20, 12, 20, 12      # be_dual_valu_dev.h, be_ipm_dev.h, be_dual_dev.h


def hv_padded(k):
    return k if k <= 7 else (k + 1) & ~1


def hv_pitch(k):
    K = hv_padded(k)
    return (K * (K + 1) // 2 + K + 3) & ~3


def ipm_nv(K):
    return K * (K + 1) // 2 + 2 * K + 1


def sums_path(plan, n, k, flags, rows):
    """(routine, instance size) that sample of k cuts runs on the launch `plan` with `rows` staged rows: be_dual_dev.h `valu`
    (dual_step_body), be_ipm_dev.h ipm_solve (its conditions `hv_ok`, `fast`, the wide-one dispatch in front of the loop and the
    weighted-pass branch of the sums), be_dual_dev.h `waves_ok` (dual_step_body).  'mfma' is the general sweep."""
    cut, kt, nw, variant, staged, kernel = plan
    n_pad = (n + 15) & ~15
    f32 = cut == "float"
    if kernel == "small" or variant == "rl" or k < 2 and variant != "pdipm":
        return ("mfma", 0)
    if variant == "dual":
        lr = WIDE_LR if kernel == "wide" else 0
        mirror = lr > 0 and (min(rows, HV_KMAX) if k <= min(rows, HV_KMAX) else rows) <= HV_KMAX
        valu = (not flags & FLAG_MFMA_CONTRACTION and (nw > 1 or (n_pad <= 192 and f32 and k <= HV_K1MAX)) and 2 <= k <= HV_KMAX
                and (lr == 0 or mirror) and n_pad <= 256 * nw and nw * hv_pitch(k) <= n_pad)
        return ("valu", hv_padded(k)) if valu else ("mfma", 0)
    kp = 2 if k < 2 else hv_padded(k)
    if nw > 1 and f32 and k <= IPM_KMAX_WAVES and nw * ((ipm_nv(kp) + 3) & ~3) <= n_pad:
        return ("ipm_waves", kp)
    if f32 and n_pad > 192 and k <= IPM_KMAX_WAVES and ((ipm_nv(kp) + 3) & ~3) <= n_pad:
        return ("ipm_wide_one", kp)
    hv_ok = f32 and n_pad <= 192 and not staged
    if hv_ok and 2 <= k <= IPM_KMAX and ipm_nv(hv_padded(k)) <= n_pad:
        return ("ipm_unrolled", hv_padded(k))
    if hv_ok and 2 <= k <= HV_K1MAX and hv_pitch(k) <= n_pad:
        return ("ipm_weighted", hv_padded(k))
    return ("mfma", 0)


# ---- the table: (name, expected plan, cut dtype, slots, n, variant, flags, t, ks[, options]) -----------------------------------
# expected plan: (cut type, KT | KS, waves per workgroup, variant, staged, kernel) -- icnn_amd._lib.dual_plan()[:6]
def _plan(cut, kt, waves, variant, staged=False, kernel="body"):
    return (cut, kt, waves, variant, staged, kernel)


FIN, DUP, ZERO = ("fin", 4), ("dup", 5), ("zero", 1)
K15 = (1, 2, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15)
K31 = (1, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 31)
K10 = (1, 2, 5, 8, 9, 10)
GLB, WPS, MFMA, E64 = FLAG_GLOBAL_BUNDLE, FLAG_WAVE_PER_SAMPLE, FLAG_MFMA_CONTRACTION, FLAG_F64_ENERGY
FULL = (4.0, 0.05)                 # full_bundle's (c, sigma)

CASES = [
    # one wave, float32, LDS, dual
    ("f32_16_dual_n48", _plan("float", 16, 1, "dual"), F32, 15, 48, "dual", 0, 14, K15 + (FIN, DUP, ZERO)),
    ("f32_16_dual_n48_mfma", _plan("float", 16, 1, "dual"), F32, 15, 48, "dual", MFMA, 14, K15 + (FIN, DUP, ZERO),
     {"twin_of": "f32_16_dual_n48"}),
    ("f32_32_dual_n70", _plan("float", 32, 1, "dual"), F32, 31, 70, "dual", 0, 30, K31 + (FIN, DUP, ZERO)),
    ("f32_32_dual_n70_t12", _plan("float", 32, 1, "dual"), F32, 31, 70, "dual", 0, 12, (1, 2, 8, 9, 12, 13, DUP)),
] + [
    ("f32_16_dual_n%d" % n, _plan("float", 16, 1, "dual"), F32, 10, n, "dual", 0, 9, K10)
    for n in (1, 15, 16, 17, 63, 64, 65, 177, 192, 193, 255, 256, 257, 300, 1023)
] + [
    # rl
    ("f32_16_rl_n17", _plan("float", 16, 1, "rl"), F32, 15, 17, "rl", 0, 14, K15),
    ("f32_16_rl_n48", _plan("float", 16, 1, "rl"), F32, 15, 48, "rl", 0, 14, K15),
    ("f32_32_rl_n48", _plan("float", 32, 1, "rl"), F32, 31, 48, "rl", 0, 30, K31),
] + [
    ("%s_small%d_rl_n%d" % (cn, ks_, n), _plan(ct, ks_, 4, "rl", False, "small"), cd, slots, n, "rl", 0, slots - 1,
     tuple(k for k in (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 15) if k <= min(slots, max(n, 2))), {"twin": WPS})     # rl has no rank test: full-rank bundles only (k = 2 at n = 1: a 1 x 1 system)
    for cn, ct, cd in (("f32", "float", F32), ("f64", "double", F64))
    for slots, ks_ in ((5, 5), (7, 8), (15, 16)) for n in (1, 6, 16)
] + [
    # pdipm
    ("f32_16_pdipm_n48", _plan("float", 16, 1, "pdipm"), F32, 15, 48, "pdipm", 0, 14, (1, 2, 12, 13, 15, FIN, DUP, ZERO, 7, 8)),
    ("f32_32_pdipm_n70", _plan("float", 32, 1, "pdipm"), F32, 31, 70, "pdipm", 0, 30, (1, 2, 12, 13, 20, 21, 31, FIN, DUP, ZERO)),
    ("f32_32_pdipm_n208", _plan("float", 32, 1, "pdipm"), F32, 31, 208, "pdipm", 0, 30, (1, 2, 12, 13, 20, 21, 31, FIN, DUP, ZERO)),
    # widths at which the interior point's width-gated passes reach their largest instances (sums_path): the unrolled passes
    # need ipm_nv(12) = 103 <= n_pad <= 192, ipm_solve_wide_one_fn at 20 cuts ipm_nv(20) = 251 <= n_pad
    ("f32_32_pdipm_n177", _plan("float", 32, 1, "pdipm"), F32, 31, 177, "pdipm", 0, 30, (1, 2, 8, 9, 12, 13, 15)),
    ("f32_32_pdipm_n255", _plan("float", 32, 1, "pdipm"), F32, 31, 255, "pdipm", 0, 30, (2, 18, 19, 20, 21, 31)),
    # n_pad = 32: no room for the factor of spd_factor_size's 6, 10 and 16 (36, 100, 256 > 32), so these bundles solve twice with
    # the non-factor form of the elimination at KS = 6, 10, 16 (the rows above reach it at 8, 12, 16 only)
    ("f32_16_pdipm_n17", _plan("float", 16, 1, "pdipm"), F32, 15, 17, "pdipm", 0, 14, (5, 6, 9, 10, 13)),
    # float64 cuts
    ("f64_16_dual_n40", _plan("double", 16, 1, "dual"), F64, 15, 40, "dual", 0, 14, K15 + (FIN, DUP, ZERO)),
    ("f64_32_dual_n40", _plan("double", 32, 1, "dual"), F64, 31, 40, "dual", 0, 30, K31 + (FIN, DUP, ZERO)),
    ("f64_16_rl_n40", _plan("double", 16, 1, "rl"), F64, 15, 40, "rl", 0, 14, K15),
    ("f64_32_rl_n40", _plan("double", 32, 1, "rl"), F64, 31, 40, "rl", 0, 30, K31),
    ("f64_16_pdipm_n40", _plan("double", 16, 1, "pdipm"), F64, 15, 40, "pdipm", 0, 14, (1, 2, 12, 13, 15, FIN, DUP, ZERO)),
    ("f64_32_pdipm_n40", _plan("double", 32, 1, "pdipm"), F64, 31, 40, "pdipm", 0, 30, (1, 2, 12, 13, 20, 21, 31, FIN, DUP, ZERO)),
    # eight waves, float32
    ("f32_16_dual8_n1024", _plan("float", 16, 8, "dual"), F32, 15, 1024, "dual", 0, 14, K15),
    ("f32_16_dual8_n1040", _plan("float", 16, 8, "dual"), F32, 15, 1040, "dual", 0, 14, K15 + (FIN, DUP, ZERO)),
    ("f32_32_dual8_n1040_t20", _plan("float", 32, 8, "dual"), F32, 31, 1040, "dual", 0, 20, (1, 2, 8, 9, 20, 21, DUP)),   # 22 rows fit
    ("f32_16_pdipm8_n1040", _plan("float", 16, 8, "pdipm"), F32, 15, 1040, "pdipm", 0, 14, (1, 2, 12, 13, 15)),
    ("f32_32_pdipm8_n1040_t13", _plan("float", 32, 8, "pdipm"), F32, 31, 1040, "pdipm", 0, 13, (1, 2, 13, 14, DUP)),
    # staged bundles
    ("f32_32_pdipm8_glb_n1040", _plan("float", 32, 8, "pdipm", True), F32, 31, 1040, "pdipm", 0, 30, (1, 2, 13, 14, 20, 21, 31)),
    ("f32_wide_n1040", _plan("float", 32, 8, "dual", True, "wide"), F32, 31, 1040, "dual", 0, 30, (1, 2, 8, 9, 20, 21, 31)),
    ("f32_wide_n1536", _plan("float", 32, 8, "dual", True, "wide"), F32, 24, 1536, "dual", 0, 23, (2, 12, 13, 20, 21, 24)),
    ("f32_wide_n1536_t19", _plan("float", 32, 8, "dual", True, "wide"), F32, 24, 1536, "dual", 0, 19, (1, 2, 12, 13, 20, DUP)),
    # n = 2048: 8 hv_pitch(20) = 1856 and 8 (ipm_nv(20) + 3 & ~3) = 2016 fit the row, so the eight-wave passes reach 20 cuts
    ("f32_wide_n2048", _plan("float", 32, 8, "dual", True, "wide"), F32, 24, 2048, "dual", 0, 23, (2, 14, 15, 18, 19, 20, 21, 24)),
    ("f32_32_dual8_glb_n2048", _plan("float", 32, 8, "dual", True), F32, 24, 2048, "dual", GLB, 23, (2, 14, 15, 18, 19, 20, 21, 24),
     {"twin_of": "f32_wide_n2048"}),
    ("f32_32_pdipm8_glb_n2048", _plan("float", 32, 8, "pdipm", True), F32, 24, 2048, "pdipm", 0, 23, (1, 2, 12, 13, 20, 21, 24)),
    # (31 slots: the twins run the same tile KT = 32.  With up to 15 slots the LDS instance is KT = 16 and the staged one KT = 32,
    #  whose row reductions differ in order: measured on 13 cuts of variant pdipm, equal to rounding, not bit for bit)
    ("f32_32_pdipm_glb_n177", _plan("float", 32, 1, "pdipm", True), F32, 31, 177, "pdipm", GLB, 30, (1, 2, 8, 9, 12, 13, 15),
     {"twin_of": "f32_32_pdipm_n177"}),
    ("f32_32_dual_glb_n70", _plan("float", 32, 1, "dual", True), F32, 31, 70, "dual", GLB, 30, K31 + (FIN, DUP, ZERO), {"twin_of": "f32_32_dual_n70"}),
    ("f32_32_dual8_glb_n1040", _plan("float", 32, 8, "dual", True), F32, 31, 1040, "dual", GLB, 30, (1, 2, 8, 9, 20, 21, 31),
     {"twin_of": "f32_wide_n1040"}),
    ("f32_32_pdipm_glb_n70", _plan("float", 32, 1, "pdipm", True), F32, 31, 70, "pdipm", GLB, 30, (1, 2, 12, 13, 20, 21, 31, FIN, DUP, ZERO),
     {"twin_of": "f32_32_pdipm_n70"}),
    ("f32_32_pdipm8_glbflag_n1040_t13", _plan("float", 32, 8, "pdipm", True), F32, 31, 1040, "pdipm", GLB, 13, (1, 2, 13, 14, DUP),
     {"twin_of": "f32_32_pdipm8_n1040_t13"}),
    ("f32_32_pdipm1_glb_n2560", _plan("float", 32, 1, "pdipm", True), F32, 31, 2560, "pdipm", 0, 30, (2, 21, 29)),      # one wave from 29 rows on
    ("f64_32_dual_glb_n640", _plan("double", 32, 1, "dual", True), F64, 31, 640, "dual", 0, 30, (1, 8, 9, 16, 17, 24, 25, 31, DUP)),
    ("f64_32_pdipm_glb_n640", _plan("double", 32, 1, "pdipm", True), F64, 31, 640, "pdipm", 0, 30, (1, 2, 12, 13, 20, 21, 31, DUP)),
    # single rows
    ("f32_16_dual_recycled", _plan("float", 16, 1, "dual"), F32, 10, 48, "dual", 0, 17, K10 + (DUP,), {"iters": 24}),
    ("f32_16_dual_f64energy", _plan("float", 16, 1, "dual"), F32, 10, 48, "dual", E64, 9, K10, {"f64_energy": True}),
] + [
    # n = 159 (n_pad 160): the width of the persistent tile kernel's fixed-shape instances, whose dual bodies
    # tests/test_dual_body_probe.py runs on these same rows.  t <= 7: the rounds of the body capped at eight cuts.
    ("f32_16_dual_n159_%s" % tag, _plan("float", 16, 1, "dual"), F32, slots, 159, "dual", 0, t, ks)
    for tag, slots, t, ks in (("t7", 10, 7, (1, 2, 3, 4, 5, 6, 7, 8, FIN, DUP, ZERO)), ("t5", 10, 5, (1, 2, 3, 4, 5, 6, ("dup", 3))),
                              ("t3", 10, 3, (1, 2, 3, 4, ("dup", 2))), ("t0", 10, 0, (1, ZERO)), ("t9", 10, 9, (1, 2, 4, 5, 8, 9, 10, DUP)),
                              ("s5_t4", 5, 4, (1, 2, 3, 4, 5)))       # s5: rows_cap is held by the slots, not by t + 1
] + [
    ("f32_32_dual_n159", _plan("float", 32, 1, "dual"), F32, 31, 159, "dual", 0, 30, K31 + (FIN, DUP, ZERO)),
] + [
    # the same width on bundles that stay full (full_bundle): random cuts prune hard -- the k = 8 sample of the t7 row above ends
    # its round with 3 cuts
    ("f32_16_dual_n159_full_%s" % tag, _plan("float", 16, 1, "dual"), F32, slots, 159, "dual", 0, t, ks, {"full": FULL})
    for tag, slots, t, ks in (("t7", 10, 7, (2, 3, 4, 5, 6, 7, 8, 8)), ("t5", 10, 5, (2, 3, 4, 5, 6, 6)), ("t3", 10, 3, (2, 3, 4, 4)),
                              ("t1", 10, 1, (2, 2)), ("t9", 10, 9, (8, 9, 10, 10)), ("s8_t7", 8, 7, (7, 8, 8)))
] + [
    ("f32_32_dual_n159_full_t20", _plan("float", 32, 1, "dual"), F32, 31, 159, "dual", 0, 20, (8, 9, 12, 13, 16, 17, 20, 21), {"full": FULL}),
]
CASE_IDS = [c[0] for c in CASES]

# samples whose first draw misses a precondition of tests/test_dual_step_shapes.py (a multiplier on the pruning threshold, an
# oracle that needs nearly all its updates): (row, sample) -> bump of the sample's seed.  Found by tools of the test itself:
# test_preconditions names the sample and the condition.
RESEED = {
    ('f32_32_pdipm_n177', 2): 1,
    ('f32_32_pdipm_n177', 3): 24,
    ('f32_32_pdipm_n177', 4): 1,
    ('f32_32_pdipm_n177', 5): 1,
    ('f32_32_pdipm_n177', 6): 3,
    ('f32_16_pdipm_n48', 1): 2,
    ('f32_16_pdipm_n48', 3): 6,
    ('f32_16_pdipm_n48', 4): 2,
    ('f32_16_pdipm_n48', 8): 10,
    ('f32_16_pdipm_n48', 9): 1,
    ('f32_16_rl_n17', 3): 2,
    ('f32_16_rl_n48', 1): 2,
    ('f32_16_rl_n48', 4): 1,
    ('f32_16_rl_n48', 7): 1,
    ('f32_16_rl_n48', 10): 1,
    ('f32_16_rl_n48', 12): 1,
    ('f32_32_rl_n48', 1): 1,
    ('f32_32_rl_n48', 4): 1,
    ('f32_32_rl_n48', 5): 2,
    ('f32_32_rl_n48', 6): 2,
    ('f32_32_rl_n48', 7): 1,
    ('f32_32_rl_n48', 10): 1,
    ('f32_small5_rl_n1', 1): 1,
    ('f32_small5_rl_n6', 3): 1,
    ('f32_small8_rl_n1', 1): 3,
    ('f32_small8_rl_n6', 1): 2,
    ('f32_small8_rl_n6', 3): 1,
    ('f32_small8_rl_n16', 1): 2,
    ('f32_small16_rl_n16', 1): 1,
    ('f32_small16_rl_n16', 4): 1,
    ('f32_small16_rl_n16', 7): 1,
    ('f64_small5_rl_n6', 1): 2,
    ('f64_small8_rl_n16', 4): 1,
    ('f64_small16_rl_n1', 1): 1,
    ('f64_small16_rl_n16', 6): 1,
    ('f64_small16_rl_n16', 7): 1,
    ('f32_32_pdipm_n70', 1): 2,
    ('f32_32_pdipm_n70', 2): 1,
    ('f32_32_pdipm_n70', 5): 1,
    ('f32_32_pdipm_n70', 6): 5,
    ('f32_32_pdipm_n208', 2): 1,
    ('f32_32_pdipm_n208', 4): 3,
    ('f32_32_pdipm_n208', 6): 1,
    ('f64_16_rl_n40', 3): 2,
    ('f64_16_rl_n40', 6): 1,
    ('f64_16_rl_n40', 7): 1,
    ('f64_32_rl_n40', 1): 1,
    ('f64_32_rl_n40', 3): 2,
    ('f64_32_rl_n40', 9): 2,
    ('f64_16_pdipm_n40', 1): 2,
    ('f64_16_pdipm_n40', 3): 1,
    ('f64_16_pdipm_n40', 4): 2,
    ('f64_32_pdipm_n40', 2): 1,
    ('f64_32_pdipm_n40', 4): 4,
    ('f64_32_pdipm_n40', 5): 4,
    ('f64_32_pdipm_n40', 6): 7,
    ('f32_16_pdipm8_n1040', 3): 2,
    ('f32_16_pdipm8_n1040', 4): 2,
    ('f32_32_pdipm8_n1040_t13', 3): 6,
    ('f32_32_pdipm8_glb_n1040', 2): 1,
    ('f32_32_pdipm8_glb_n1040', 3): 1,
    ('f32_32_pdipm8_glb_n1040', 4): 2,
    ('f32_32_pdipm8_glb_n1040', 5): 1,
    ('f32_32_pdipm1_glb_n2560', 1): 1,
    ('f32_32_pdipm1_glb_n2560', 2): 1,
    ('f64_32_pdipm_glb_n640', 2): 1,
    ('f64_32_pdipm_glb_n640', 3): 1,
    ('f64_32_pdipm_glb_n640', 4): 1,
    ('f64_32_pdipm_glb_n640', 5): 2,
    ('f64_32_pdipm_glb_n640', 6): 1,
    ('f32_32_pdipm_n255', 1): 2,
    ('f32_32_pdipm_n255', 2): 7,
    ('f32_32_pdipm_n255', 4): 2,
    ('f32_32_pdipm_n255', 5): 1,
    ('f32_16_pdipm_n17', 0): 9,
    ('f32_16_pdipm_n17', 1): 9,
    ('f32_16_pdipm_n17', 2): 10,
    ('f32_16_pdipm_n17', 4): 1,
    ('f32_32_pdipm8_glb_n2048', 2): 1,
    ('f32_32_pdipm8_glb_n2048', 4): 1,
    ('f32_32_pdipm8_glb_n2048', 5): 2,
    ('f32_32_pdipm8_glb_n2048', 6): 1,
    # the full rows' own condition (test_full_rows_stay_full): a draw whose oracle round keeps 16 and more cuts
    ('f32_32_dual_n159_full_t20', 4): 11,
    ('f32_32_dual_n159_full_t20', 6): 13,
    ('f32_32_dual_n159_full_t20', 7): 5,
}


def case_options(case):
    return case[9] if len(case) > 9 else {}


@functools.lru_cache(maxsize=None)
def case_state(name):
    """the synthetic state of a table row; the seed is the CRC of the row's name, nothing else.  A twin row (options twin_of) has the
    state of the row it names."""
    i = CASE_IDS.index(name)
    case = CASES[i]
    opt = case_options(case)
    if "twin_of" in opt:
        base = case_state(opt["twin_of"])
        assert (base.n, base.slots, base.cut_dtype, base.variant, base.t) == (case[4], case[3], case[2], case[5], case[7])
        return base
    _, _, cut, slots, n, variant, flags, t, ks = case[:9]
    reseed = tuple((u, b) for (row, u), b in sorted(RESEED.items()) if row == name)
    return synth_round(zlib.crc32(name.encode()), n, slots, cut, variant, t, ks, opt.get("iters", 0), opt.get("f64_energy", False), reseed,
                       opt.get("full"))


PERTURB_DRAWS = 3
ZERO_MARGIN = 1e-12             # newton_trace: no multiplier this close to zero when a clip or the pivot's 1 - sum decides it
OBJECTIVE_NOISE_LAM = 1e-13     # objective_noise_runs: the multipliers move by no more than this
PRUNED_GRAD_MARGIN = 1e-8       # a pruned cut's reduced gradient must be above this: the sign the bound rule (:119) asks for is then
                                # not a matter of rounding


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """(one_round of the row's state, [one_round of PERTURB_DRAWS perturbed copies]): computed once, shared, never written to"""
    s = case_state(name)
    with np.errstate(all="ignore"):
        ref = one_round(s)
        pert = [one_round(perturbed(s, 500 + d)) for d in range(PERTURB_DRAWS)]
    return ref, pert


@functools.lru_cache(maxsize=None)
def precondition_failures(name):
    """[(sample, what)] for every live sample of the row that misses a precondition of the comparison (module docstring of
    tests/test_dual_step_shapes.py); also returns the per-sample spread of lam and y between the oracle and its perturbed runs"""
    s = case_state(name)
    ref, pert = case_reference(name)
    cap = NEWTON_CAP[s.variant]
    noise = objective_noise_runs(s) if s.variant == "rl" else []
    bad = []
    lam_spread, y_spread = np.zeros(s.B), np.zeros(s.B)
    for u in range(s.B):
        for p in pert:
            if p["active"][u] != ref["active"][u] or p["finished"][u] != ref["finished"][u] or p["n_iters"][u] != ref["n_iters"][u]:
                bad.append((u, "the perturbed oracle ends on another active set / finished / n_iters"))
                continue
            y_spread[u] = max(y_spread[u], float(np.max(np.abs(p["y"][u] - ref["y"][u]))))
            if len(ref["lam"][u]) and ref["lam_full"][u] is not None:
                lam_spread[u] = max(lam_spread[u], float(np.max(np.abs(p["lam"][u] - ref["lam"][u]))))
            if p["newton"][u] is not None and not p["newton"][u] < cap - 2:
                bad.append((u, "the perturbed oracle needs %d of %d updates" % (p["newton"][u], cap)))
        if y_spread[u] > 1e-11:
            bad.append((u, "y moves by %.2e under the perturbation" % y_spread[u]))
        if ref["lam_full"][u] is None:
            continue
        if not np.isfinite(ref["y"][u]).all() or not np.isfinite(ref["lam_full"][u]).all():
            bad.append((u, "non-finite oracle result"))
        if ref["newton"][u] is not None and not ref["newton"][u] < cap - 2:
            bad.append((u, "the oracle needs %d of %d updates" % (ref["newton"][u], cap)))
        if len(ref["lam"][u]) and ref["lam"][u].min() <= 1e-6:
            bad.append((u, "surviving multiplier %.2e" % ref["lam"][u].min()))
        if s.variant != "pdipm" and len(ref["lam_full"][u]) > 1:
            with np.errstate(all="ignore"):
                lam_t, margin = newton_trace(*bundle_of(s, ref, u), oracle.VARIANTS[s.variant])
            if not np.array_equal(lam_t, ref["lam_full"][u]):
                bad.append((u, "newton_trace is not the oracle's simplex_newton"))
            if margin < ZERO_MARGIN:
                bad.append((u, "a multiplier was %.1e from zero before the clip / the pivot's 1 - sum decided it" % margin))
            for r in noise:
                if r["active"][u] != ref["active"][u] or r["finished"][u] != ref["finished"][u]:
                    bad.append((u, "the line search is decided by the rounding of the objective: another active set"))
                elif np.max(np.abs(r["lam"][u] - ref["lam"][u])) > OBJECTIVE_NOISE_LAM:
                    bad.append((u, "the line search is decided by the rounding of the objective: lam moves by %.1e"
                                % np.max(np.abs(r["lam"][u] - ref["lam"][u]))))
            _, g0_pruned = reduced_gradient(*bundle_of(s, ref, u), ref["lam_full"][u])
            if len(g0_pruned) and g0_pruned.min() <= PRUNED_GRAD_MARGIN:
                bad.append((u, "reduced gradient %.2e of a pruned cut: on the bound rule's threshold" % g0_pruned.min()))
        if s.variant == "pdipm":
            gone = ref["lam_full"][u][ref["lam_full"][u] <= oracle._IPM_PRUNE]
            if len(gone) and gone.max() >= 1e-10:
                bad.append((u, "pruned multiplier %.2e" % gone.max()))
    return bad, lam_spread, y_spread
