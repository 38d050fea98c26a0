"""Helpers of the implicit-feed shape tests (test infrastructure, no GPU needed to import):

  kkt_grad_ld / feed_rows_ld   oracle/implicit_feed_oracle.py restated in numpy.longdouble -- the truth the float64 oracle is
                               judged against, so that the oracle is never the weak side of a device comparison
  synth_state                  a solver result written by hand: exact bundle sizes, slots in random order, NaN in everything
                               the kernel must not read, saturated and clamped columns in y
  feed_instance                launch_implicit_feed's choice of kernel instance (be_dual.hip), restated
  CASES                        the instance / bundle-size table of tests/test_implicit_feed_shapes.py
"""
import numpy as np

LD = np.longdouble


# ---- extended-precision restatement -----------------------------------------------------------------------------------------
def solve_gepp_ld(H, rhs):
    """H x = rhs by Gaussian elimination with partial pivoting, every operation in longdouble."""
    H = np.array(H, dtype=LD, copy=True)
    x = np.array(rhs, dtype=LD, copy=True)
    m = H.shape[0]
    for p in range(m):
        q = p + int(np.argmax(np.abs(H[p:, p])))
        if q != p:
            H[[p, q]] = H[[q, p]]
            x[[p, q]] = x[[q, p]]
        for r in range(p + 1, m):
            f = H[r, p] / H[p, p]
            H[r, p:] -= f * H[p, p:]
            x[r] -= f * x[p]
    for p in range(m - 1, -1, -1):
        x[p] = (x[p] - H[p, p + 1:].dot(x[p + 1:])) / H[p, p]
    return x


def kkt_grad_ld(y, true_y, G, loss):
    """implicit_feed_oracle.kkt_grad in longdouble: same z, dl and clamp rules, the bordered (k+1) system, c_y zeroed where y is
    exactly 0 or 1."""
    y, true_y, G = np.asarray(y, dtype=LD), np.asarray(true_y, dtype=LD), np.asarray(G, dtype=LD)
    k, n = G.shape
    one = LD(1)
    if loss == "xent":
        yc = np.clip(y, LD(1e-8), one - LD(1e-8))       # the float64 constants 1e-8 and 1 - 1e-8, as the oracle's
        z = one / yc + one / (one - yc)
        dl = true_y / yc - (one - true_y) / (one - yc)
    elif loss == "mse":
        with np.errstate(divide="ignore"):
            z = one / y + one / (one - y)
        dl = -(y - true_y)
    else:
        raise ValueError(loss)
    zinv = one / z
    Gz = G * zinv
    H = np.zeros((k + 1, k + 1), dtype=LD)
    H[:k, :k] = Gz.dot(G.T)
    H[:k, k] = one
    H[k, :k] = one
    rhs = np.concatenate([Gz.dot(dl), np.zeros(1, dtype=LD)])
    sol = solve_gepp_ld(H, rhs)
    c_lam, c_t = sol[:k], sol[k:]
    c_y = zinv * dl - Gz.T.dot(c_lam)
    c_y[(y == 0) | (y == 1)] = 0
    return c_y, c_lam, c_t


def feed_rows_ld(y_n, true_y, G, ys, lam, loss):
    """implicit_feed_oracle.feed_rows in longdouble (v and c as longdouble arrays)."""
    idx, rows_y, rows_v, rows_c = [], [], [], []
    for j in range(len(G)):
        if len(G[j]) == 0:
            continue
        c_y, c_lam, _ = kkt_grad_ld(y_n[j], true_y[j], np.array(G[j]), loss)
        yj = np.asarray(y_n[j], dtype=LD)
        for i in range(len(G[j])):
            idx.append(j)
            rows_y.append(ys[j][i])
            rows_v.append(LD(lam[j][i]) * c_y + c_lam[i] * (yj - np.asarray(ys[j][i], dtype=LD)))
            rows_c.append(c_lam[i])
    n = y_n.shape[1]
    return (np.array(idx, dtype=np.int64), np.array(rows_y, dtype=np.float64).reshape(-1, n),
            np.array(rows_v, dtype=LD).reshape(-1, n), np.array(rows_c, dtype=LD))


# ---- synthetic solver result --------------------------------------------------------------------------------------------------
SATURATED = (0.0, 1.0, 3e-9, 1.0 - 2e-9)      # exactly 0, exactly 1 (rule :416), below / above the cross-entropy clamp at 1e-8


class SynthState:
    """What a BundleState holds after a solve, as host arrays: y [B, n], G [B, slots, n] in the cut dtype, ys [B, slots, n],
    lam / active [B, slots], count [B]; labels [B, n]; sat[i] = the column of y that was overwritten with SATURATED[i]."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def bundles(self):
        """(A, xs, lams): the active rows per sample in bundle order, as implicit_feed_oracle.feed_rows takes them"""
        A = [[self.G[u, s].astype(np.float64) for s in self.active[u, :self.count[u]]] for u in range(self.B)]
        xs = [[self.ys[u, s] for s in self.active[u, :self.count[u]]] for u in range(self.B)]
        lams = [self.lam[u, :self.count[u]] for u in range(self.B)]
        return A, xs, lams

    def to_device(self):
        """BundleResult over a BundleState whose tensors hold this state (needs the GPU)"""
        import torch
        from icnn_amd import bundle_entropy
        y = torch.from_numpy(self.y.copy()).cuda()
        st = bundle_entropy.BundleState(y, self.slots, self.variant,
                                        torch.float64 if self.cut_dtype == np.float64 else torch.float32)
        assert st.T == self.slots
        for name in ("G", "ys", "lam", "active"):
            getattr(st, name).copy_(torch.from_numpy(getattr(self, name)))
        st.count[:self.B].copy_(torch.from_numpy(self.count))
        return bundle_entropy.BundleResult(st)


def synth_state(seed, n, slots, cut_dtype, variant, ks, loss):
    """Sample u has count = ks[u]; active[u, :k] is a random subset of the slots in random order; G there standard normal in the
    cut dtype, lam on the simplex, ys uniform in (0,1); y = 1/(1+exp(G^T lam)) with up to four columns overwritten by SATURATED.
    Every inactive slot of G and ys and every lam[u, k:] is NaN (active[u, k:] repeats an inactive slot where there is one):
    the kernel must never read them.  Seeded by RandomState only."""
    rng = np.random.RandomState(seed)
    cut_dtype = np.dtype(cut_dtype).type
    B = len(ks)
    G = np.full((B, slots, n), np.nan, dtype=cut_dtype)
    ys = np.full((B, slots, n), np.nan)
    lam = np.full((B, slots), np.nan)
    active = np.zeros((B, slots), dtype=np.int32)
    y = np.empty((B, n))
    sat = rng.permutation(n)[:min(n, len(SATURATED))]
    for u, k in enumerate(ks):
        assert 0 <= k <= slots and (k <= n // 2 or n == 1)
        perm = rng.permutation(slots)
        active[u, :k] = perm[:k]
        active[u, k:] = perm[k] if k < slots else perm[0]
        G[u, perm[:k]] = rng.randn(k, n).astype(cut_dtype)
        ys[u, perm[:k]] = rng.rand(k, n)
        w = rng.rand(k) + 0.1
        lam[u, :k] = w / w.sum()
        y[u] = 1.0 / (1.0 + np.exp(lam[u, :k].dot(G[u, perm[:k]].astype(np.float64)))) if k else rng.rand(n)
        y[u, sat] = SATURATED[:len(sat)]
    labels = (rng.rand(B, n) < 0.3).astype(np.float64) if loss == "xent" else rng.rand(B, n)
    return SynthState(B=B, n=n, slots=slots, cut_dtype=cut_dtype, variant=variant, loss=loss, y=y, G=G, ys=ys, lam=lam,
                      active=active, count=np.array(ks, dtype=np.int32), labels=labels, sat=sat)


# ---- which instance the launcher picks (be_dual.hip launch_implicit_feed, be_dual_cut.h carve, be_common.h pw_build) ----------
LDS_LIMIT = 160 * 1024


def _a16(v):
    return (v + 15) & ~15


def pw_leaves(n):
    if n <= 128:
        return 1
    n2 = n // 2
    n2 -= n2 % 8
    return pw_leaves(n2) + pw_leaves(n - n2)


def dual_row_pitch(n_pad):
    while n_pad % 32 != 2:
        n_pad += 1
    return n_pad


def carve_total(KT, rows, ldA, n_pad, cut_bytes, n_leaves, glb=False):
    """carve(KT, rows, ldA, n_pad, cut_bytes, n_leaves, rl=false).total: one wave, its own constant rows, no extra column
    buffers; glb: the rows live in device memory"""
    o = _a16(0 if glb else (rows + 2) * ldA * cut_bytes)
    o += 2 * _a16(n_pad * 8)
    o += _a16(max(rows * ((rows + 1) | 1) * 8, (KT * n_leaves + 2 * KT) * 8))
    return o + _a16(KT * 4)


def feed_lds_bytes(n, slots, cut_dtype, rows=None, glb=False):
    KT = 32 if slots > 15 else 16
    n_pad = _a16(n)
    return carve_total(KT, slots if rows is None else rows, dual_row_pitch(n_pad), n_pad,
                       8 if np.dtype(cut_dtype) == np.float64 else 4, pw_leaves(n), glb)


def feed_instance(n, slots, cut_dtype):
    """('float' | 'double', KT, 'LDS' | 'GLB') of the implicit_feed_kernel instance launch_implicit_feed takes"""
    return ("double" if np.dtype(cut_dtype) == np.float64 else "float", 32 if slots > 15 else 16,
            "GLB" if feed_lds_bytes(n, slots, cut_dtype) > LDS_LIMIT else "LDS")


def rows_fit(n, slots, cut_dtype):
    """dual_rows_fit for one wave of variant dual (n < 1024): the same carve as the feed's"""
    rows = slots
    while rows > 0 and feed_lds_bytes(n, slots, cut_dtype, rows) > LDS_LIMIT:
        rows -= 1
    return rows


# ---- the table: (name, expected instance, cut dtype, slots, n, variant, count per sample) -------------------------------------
F32, F64 = np.float32, np.float64
CASES = [
    ("f32_16", ("float", 16, "LDS"), F32, 15, 48, "dual", (0, 1, 4, 5, 7, 8, 9, 15, 0)),
    ("f32_16_n1", ("float", 16, "LDS"), F32, 8, 1, "dual", (0, 1, 1)),
    ("f32_16_n16", ("float", 16, "LDS"), F32, 8, 16, "dual", (1, 4, 5, 7, 8)),
    ("f32_16_n17", ("float", 16, "LDS"), F32, 8, 17, "dual", (1, 4, 5, 7, 8)),
    ("f32_32", ("float", 32, "LDS"), F32, 31, 70, "dual", (0, 1, 4, 5, 7, 8, 9, 15, 16, 17, 20, 21, 31)),
    ("f32_32_pdipm_n1024", ("float", 32, "LDS"), F32, 31, 1024, "pdipm", (1, 8, 16, 17, 31)),
    ("f64_16", ("double", 16, "LDS"), F64, 15, 40, "dual", (0, 1, 4, 5, 7, 8, 9, 15)),
    ("f64_32", ("double", 32, "LDS"), F64, 20, 40, "dual", (1, 8, 9, 15, 16, 17, 20)),
    ("f32_16_glb", ("float", 16, "GLB"), F32, 15, 2048, "dual", (1, 7, 8, 15)),
    ("f32_32_glb", ("float", 32, "GLB"), F32, 31, 1104, "dual", (0, 4, 16, 17, 21, 31)),
    ("f64_16_glb", ("double", 16, "GLB"), F64, 15, 1200, "dual", (1, 8, 9, 15)),
    ("f64_32_glb", ("double", 32, "GLB"), F64, 31, 640, "dual", (1, 8, 16, 17, 20, 31)),
]
CASE_IDS = [c[0] for c in CASES]
ALL_K = (0, 1, 4, 5, 7, 8, 9, 15, 16, 17, 20, 21, 31)


def case_state(name, loss):
    """the synthetic state of a table row; the seed is the row's position and the loss, nothing else"""
    i = CASE_IDS.index(name)
    _, _, cut, slots, n, variant, ks = CASES[i]
    return synth_state(1000 + 2 * i + (loss == "mse"), n, slots, cut, variant, ks, loss)
