"""Statements of the solver comparison for tests/test_pgd*.py (shares no code with the kernels): the entropy-scaled
objective E - H(y) with the scripts' entr() convention, projected gradient descent on it as icnn_amd/pgd.py defines it, and
the bundle's lower bound.  NumPy float64; the sums that the tests compare a device sum against are formed in extended
precision, so that a tolerance pays for the device's rounding alone."""
import numpy as np

LO, HI = 1e-6, 1.0 - 1e-6                 # the scripts' proj (multi-label-cls/ebundle-vs-gd.py:116-117)
F32 = np.float32
ULP = 2.0 ** -52


def log_up(x):
    """np.log moved one ulp up: the perturbed logarithm of the feed screen (screen_feeds)"""
    return np.nextafter(np.log(x), np.inf)


def entr_terms(y, log=np.log):
    """y log y + (1 - y) log(1 - y) per element, an element whose term is NaN counting 0 -- minus the z of the scripts' entr()
    (ebundle-vs-gd.py:38-41), which zeroes 0 log 0 at y = 0 and y = 1 and every y outside [0, 1]"""
    y = np.asarray(y, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = y * log(y) + (1.0 - y) * log(1.0 - y)
    return np.where(t != t, 0.0, t)


def _row_sum(t):
    return np.sum(np.asarray(t, np.longdouble), axis=1).astype(np.float64)


def objective(E, y, log=np.log):
    """float64(E) - H(y) per sample"""
    return np.asarray(E).astype(np.float64) + _row_sum(entr_terms(y, log))


def objective_scale(E, y):
    """|E| + sum_j |y log y| + |(1 - y) log(1 - y)| per sample: what the tolerance of an objective is relative to"""
    y = np.asarray(y, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        a, b = np.abs(y * np.log(y)), np.abs((1.0 - y) * np.log(1.0 - y))
    a, b = np.where(a != a, 0.0, a), np.where(b != b, 0.0, b)
    return np.abs(np.asarray(E).astype(np.float64)) + _row_sum(a + b)


def grad(g, yf, log=np.log):
    """G = (float64(g) + log yf) - log(1 - yf); 1 - yf is exact in float64 for a float32 yf"""
    yf = np.asarray(yf, np.float64)
    return (np.asarray(g).astype(np.float64) + log(yf)) - log(1.0 - yf)


def pgd(fg, y0, K, lr, lo=LO, hi=HI, final=False, log=np.log):
    """The iteration of icnn_amd/pgd.py.  fg(y float64) -> (E, dE/dy) is fed float64(float32(y_k)).  Returns a dict: y = y_K
    [B, n]; obj [K, B] = e_k; scale [K, B] = objective_scale at the points e_k was taken; feeds = the K float32 feeds;
    iterates = y_0 .. y_K; obj_final, scale_final = e_K and its scale when `final`."""
    y = np.clip(np.asarray(y0, np.float64), lo, hi)
    out = {"obj": [], "scale": [], "feeds": [], "iterates": [y.copy()]}
    for _ in range(K):
        y32 = y.astype(F32)
        yf = y32.astype(np.float64)
        E, g = fg(yf)
        out["feeds"].append(y32)
        out["obj"].append(objective(E, yf, log))
        out["scale"].append(objective_scale(E, yf))
        step = lr * grad(g, yf, log)
        y = np.minimum(np.maximum(y - step, lo), hi)
        out["iterates"].append(y.copy())
    out["y"] = y
    out["obj"], out["scale"] = np.stack(out["obj"]), np.stack(out["scale"])
    if final:
        yf = y.astype(F32).astype(np.float64)
        E, _ = fg(yf)
        out["obj_final"], out["scale_final"] = objective(E, yf, log), objective_scale(E, yf)
    return out


def screen_feeds(fg, y0, K, lr, lo=LO, hi=HI):
    """The restatement run with np.log and with a logarithm one ulp off: (run with np.log, True when both runs feed the
    float32 energy the same bits at every iteration and clip the same entries of every iterate).  Then a device logarithm
    that is a few ulp off np.log moves y by the rounding of the update alone."""
    a = pgd(fg, y0, K, lr, lo, hi, final=True)
    b = pgd(fg, y0, K, lr, lo, hi, log=log_up)
    same = all(np.array_equal(p, q) for p, q in zip(a["feeds"], b["feeds"]))
    same = same and all(np.array_equal(p == lo, q == lo) and np.array_equal(p == hi, q == hi)
                        for p, q in zip(a["iterates"], b["iterates"]))
    return a, same


def y_tolerance(K, lr, lo=LO):
    """A logarithm accurate to a few ulp enters y K times with weight lr: K lr 64 2^-52 |log lo|"""
    return K * lr * 64 * ULP * abs(np.log(lo))


def softplus(x):
    x = np.asarray(x, np.longdouble)
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def dual_bound(G_rows, h_rows, lam):
    """(d, scale) of one sample: d = lam . h - sum_j log(1 + exp(-a_j)) with a = G^T lam over the active cuts G_rows [k, n],
    h_rows [k], lam [k]; scale = |lam . h| + sum_j softplus(-a_j).  For lam on the simplex d <= min_y E(y) - H(y): every cut
    under-estimates the convex E, so E(y) >= sum_i lam_i (g_i . y + h_i), and min_y <a, y> - H(y) = -sum_j log(1 + exp(-a_j)).
    No cut or lam None: (-inf, 0)."""
    if lam is None or len(lam) == 0:
        return -np.inf, 0.0
    G = np.asarray(G_rows).astype(np.longdouble).reshape(len(lam), -1)
    lam = np.asarray(lam).astype(np.longdouble)
    lh = np.sum(lam * np.asarray(h_rows).astype(np.longdouble))
    sp = np.sum(softplus(-(G.T.dot(lam))))
    return float(lh - sp), float(abs(lh) + sp)


def dual_bounds(A, b, lam):
    """dual_bound per sample of the reference's ragged (A, b, lam) lists: (d [B], scale [B])"""
    pairs = [dual_bound(A[u], b[u], lam[u]) for u in range(len(lam))]
    return np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
