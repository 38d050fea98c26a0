"""A NumPy restatement of the feed-forward baseline's training step, written from its description, with the
error bound of every quantity.  Everything is float64; the float32 update is ddpg_ref.update32.

A model is a dict W1, b1, gamma1, beta1, ..., Wo, bo (W [in, out]);  L hidden layers, h_0 = x:
    z_i = h_{i-1} W_i + b_i,  a_i = relu(z_i),  mu_i = mean_b a_i,  var_i = mean_b (a_i - mu_i)^2   (or the moving pair)
    inv_i = 1 / sqrt(var_i + eps),  xh_i = (a_i - mu_i) inv_i,  h_i = xh_i gamma_i + beta_i
    logit = h_L Wo + bo,  yhat = 1 / (1 + exp(-logit)),  om = 1 - yhat
    loss = sum(-y log(yhat + 1e-10) - (1 - y) log(om + 1e-10))
    dy = -y / (yhat + 1e-10) + (1 - y) / (om + 1e-10),  dlogit = dy yhat om
    du_i = delta_{i+1} W_{i+1}^T,  S1 = sum_b du,  S2 = sum_b du xh,  da = gamma inv (du - (S1 + xh S2) / B),  dz = da [mask]
    dgamma = S2, dbeta = S1,  dW_i = h_{i-1}^T dz_i,  db_i = sum_b dz_i
The ReLU masks of the backward pass are an INPUT (the reference's own where none is given).

Bounds (u = 2^-24).  A product with an exact matrix over k terms follows §22's running bound, e = e_x |W| + (k + 1) u (m_x |W|
+ |b|) with m(x) = |x| + e(x); k counts the terms of a row that are not exact zeros (an exact 0 times a weight is an exact 0,
and adding it rounds nothing).  Everything behind it follows §23's first-order rules applied to the error itself with the
true magnitudes:
    a sum              e = e_x + e_y + u m(x + y)
    a product          e = e_x m_y + |x| e_y + u m_x m_y
    a sum over B rows  e = sum of the rows' e + B u (sum of the rows' m);  a mean adds one rounding for the division
    1 / sqrt(s)        e = e_s / (2 (s - e_s)^1.5) + FN u / sqrt(s)
    sigmoid(l)         e = e_l / 4 + FN u yhat                                  (its slope is at most 1/4)
    log(v)             e = e_v / (v - e_v) + FN u |log v|
    a quotient x / v   e = e_x / (v - e_v) + |x| e_v / (v (v - e_v)) + u m(x / v)
with FN = 8 roundings for 1 / sqrt, sigmoid and log, the allowance tanhf and expf got in §22 and §23.  relu passes e on, except
where z < -e: that unit is 0 exactly on both sides.

These are worst-case bounds, and BatchNorm makes them grow fast: one layer multiplies the error relative to a column's spread
by about 6 sqrt(fan-in) (the division by sigma, the variance's own error, and the next product's sum of |W|).  Behind three
layers they say little about a single element; the per-layer checks of tests/test_ff.py, which start every layer from the
device's own inputs, are the ones that stay sharp at any depth.
"""
import numpy as np

from ddpg_ref import U, adam_lr_t, update32  # noqa: F401

FN = 8
BN_EPS = float(np.float32(1e-5))
LOSS_EPS = float(np.float32(1e-10))


def names(L):
    out = []
    for i in range(1, L + 1):
        out += ["W%d" % i, "b%d" % i, "gamma%d" % i, "beta%d" % i]
    return out + ["Wo", "bo"]


def widths(shape):
    """(B, n_features, layer_sizes, n_labels) -> [w_0, .., w_L, n_labels]"""
    return [shape[1]] + list(shape[2]) + [shape[3]]


def uniform_params(shape, seed, density=1.0, logit_offset=0.0):
    """W uniform +-1/sqrt(fan-in), gamma uniform in [0.5, 1.5), beta uniform +-0.5: every unit's h is O(1), both signs.  The
    hidden biases are uniform in [0, 0.5): a unit is then on in most rows but not all, so no column's batch variance is tiny.
    (1 / sqrt(var + eps) multiplies every error below it by up to 316 where a unit is on in one row of the batch; that is the
    model's own conditioning, and a draw that has it at every layer leaves no bound that says anything.)
    density < 1: the inputs are batch(density=)'s sparse 0 / 1 rows, and W1 is widened by 1 / sqrt(density) to keep z_1 O(1).
    logit_offset > 0: |bo| uniform in [offset, offset + 1) with either sign, which keeps every logit away from 0."""
    rng = np.random.RandomState(seed)
    w = widths(shape)
    L = len(w) - 2
    P = {}
    for i in range(1, L + 2):
        r = 1.0 / np.sqrt(w[i - 1] * (density if i == 1 else 1.0))
        tag = "o" if i == L + 1 else str(i)
        P["W" + tag] = rng.uniform(-r, r, (w[i - 1], w[i])).astype(np.float32)
        if i <= L:
            P["b" + tag] = rng.uniform(0.0, 0.5, w[i]).astype(np.float32)
            P["gamma" + tag] = rng.uniform(0.5, 1.5, w[i]).astype(np.float32)
            P["beta" + tag] = rng.uniform(-0.5, 0.5, w[i]).astype(np.float32)
        elif logit_offset > 0:
            P["b" + tag] = (rng.choice([-1.0, 1.0], w[i]) * rng.uniform(logit_offset, logit_offset + 1.0, w[i])).astype(np.float32)
        else:
            P["b" + tag] = rng.uniform(-r, r, w[i]).astype(np.float32)
    return P


def batch(shape, seed, rows=None, density=1.0):
    """x uniform in [-1, 1) -- or, with density < 1, 0 / 1 with that share of ones, as Bibtex's bag of words --, y 0 / 1 with
    both values in every row where there are two labels; float32"""
    rng = np.random.RandomState(3000 + seed)
    B = shape[0] if rows is None else rows
    if density < 1.0:
        x = (rng.rand(B, shape[1]) < density).astype(np.float32)
    else:
        x = rng.uniform(-1, 1, (B, shape[1])).astype(np.float32)
    y = (rng.rand(B, shape[3]) < 0.4).astype(np.float32)
    if shape[3] > 1:
        y[:, 0], y[:, 1] = 1.0, 0.0
    return x, y


def moving_stats(shape, seed):
    """non-trivial moving pairs: means around 0.3, variances in [0.2, 1.7)"""
    rng = np.random.RandomState(4000 + seed)
    return [((0.3 + 0.2 * rng.randn(w)).astype(np.float32), rng.uniform(0.2, 1.7, w).astype(np.float32)) for w in shape[2]]


def flat(P, L):
    return np.concatenate([np.asarray(P[k]).reshape(-1) for k in names(L)])


def unflat(vec, like, L):
    out, at = {}, 0
    for k in names(L):
        n = like[k].size
        out[k] = np.asarray(vec[at:at + n]).reshape(like[k].shape)
        at += n
    return out


def _m(x, e):
    return np.abs(x) + e


def e_sum(ex, ey, s):
    return ex + ey + U * (np.abs(s) + ex + ey)


def e_prod(x, ex, y, ey):
    return ex * _m(y, ey) + np.abs(x) * ey + U * _m(x, ex) * _m(y, ey)


def e_matmul(x, ex, W, b):
    # a term whose x is an exact 0 is an exact 0, and adding it rounds nothing: the roundings of a row are its other terms'
    k = ((x != 0) | (ex != 0)).sum(1, keepdims=True)
    bias = 0.0 if b is None else np.abs(b)
    return ex @ np.abs(W) + (k + 1) * U * (_m(x, ex) @ np.abs(W) + bias)


def e_rowsum(x, ex):
    return ex.sum(0) + x.shape[0] * U * _m(x, ex).sum(0)


def forward(P, x, L, stats=None):
    """(values, bounds) of the forward pass; stats: [(mean, var)] per layer = inference mode with these moving pairs (exact)"""
    f = {k: np.asarray(v, np.float64) for k, v in P.items()}
    h, eh = np.asarray(x, np.float64), np.zeros(np.shape(x))
    B = h.shape[0]
    v, e = {}, {}
    for i in range(1, L + 1):
        W, b, ga, be = (f[k + str(i)] for k in ("W", "b", "gamma", "beta"))
        z = h @ W + b
        ez = e_matmul(h, eh, W, b)
        a, ea = np.maximum(z, 0.0), np.where(z < -ez, 0.0, ez)       # a unit that is off beyond its bound is exactly 0
        if stats is None:
            mu = a.mean(0)
            emu = e_rowsum(a, ea) / B
            emu = emu + U * _m(mu, emu)
            d = a - mu
            ed = e_sum(ea, emu, d)
            dd, edd = d * d, e_prod(d, ed, d, ed)
            var = dd.mean(0)
            evar = e_rowsum(dd, edd) / B
            evar = evar + U * _m(var, evar)
        else:
            mu, var = (np.asarray(s, np.float64) for s in stats[i - 1])
            emu, evar = np.zeros_like(mu), np.zeros_like(var)
            d = a - mu
            ed = e_sum(ea, emu, d)
        s = var + BN_EPS
        es = evar + U * _m(s, evar)
        assert np.all(es < 0.5 * s)
        inv = 1.0 / np.sqrt(s)
        einv = es / (2.0 * (s - es) ** 1.5) + FN * U * inv
        xh, exh = d * inv, e_prod(d, ed, inv, einv)
        p = xh * ga
        ep = exh * np.abs(ga) + U * _m(xh, exh) * np.abs(ga)
        hh = p + be
        ehh = ep + U * _m(hh, ep)
        for k, val, err in (("z", z, ez), ("a", a, ea), ("mu", mu, emu), ("var", var, evar), ("inv", inv, einv), ("xh", xh, exh),
                            ("h", hh, ehh)):
            v[k + str(i)], e[k + str(i)] = val, err
        h, eh = hh, ehh
    logit = h @ f["Wo"] + f["bo"]
    el = e_matmul(h, eh, f["Wo"], f["bo"])
    yhat = 1.0 / (1.0 + np.exp(-logit))
    ey = 0.25 * el + FN * U * yhat
    om = 1.0 - yhat
    eom = ey + U * _m(om, ey)
    v.update(logit=logit, yhat=yhat, om=om)
    e.update(logit=el, yhat=ey, om=eom)
    return v, e


def head(v, e, y):
    """the loss and d loss / d logits with their bounds, from forward()'s values"""
    y = np.asarray(y, np.float64)
    out, err = {}, {}
    terms, eterms = 0.0, 0.0
    quot, equot = [], []
    for w, val, ev, sign in ((y, v["yhat"], e["yhat"], -1.0), (1.0 - y, v["om"], e["om"], 1.0)):
        s = val + LOSS_EPS
        es = ev + U * _m(s, ev)
        assert np.all(es < 0.5 * s)
        lg = np.log(s)
        elg = es / (s - es) + FN * U * np.abs(lg)
        terms = terms - w * lg
        eterms = eterms + w * (elg + U * _m(lg, elg))
        q = w / s
        quot.append(sign * q)
        equot.append(w * es / (s * (s - es)) + U * q * (1.0 + es / (s - es)))
    eterms = eterms + U * (np.abs(terms) + eterms)
    out["loss"] = terms.sum()
    err["loss"] = eterms.sum() + 2 * U * np.abs(terms).sum()      # float64 partial sums, then one rounding to float32
    dy = quot[0] + quot[1]
    edy = e_sum(equot[0], equot[1], dy)
    t = dy * v["yhat"]
    et = e_prod(dy, edy, v["yhat"], e["yhat"])
    out["dlogit"] = t * v["om"]
    err["dlogit"] = e_prod(t, et, v["om"], e["om"])
    return out, err


def layer_backward(delta, edelta, Wup, xh, exh, inv, einv, ga, mask):
    """one hidden layer's backward from the delta above it [B, K] and that layer's weights Wup [N, K]: (values, bounds) of du,
    dz, dgamma, dbeta"""
    B = delta.shape[0]
    du = delta @ Wup.T
    edu = e_matmul(delta, edelta, Wup.T, None)
    t2, et2 = du * xh, e_prod(du, edu, xh, exh)
    S1, eS1 = du.sum(0), e_rowsum(du, edu)
    S2, eS2 = t2.sum(0), e_rowsum(t2, et2)
    scale = ga * inv
    escale = np.abs(ga) * einv + U * _m(scale, np.abs(ga) * einv)
    p, ep = xh * S2, e_prod(xh, exh, S2, eS2)
    sm = S1 + p
    esm = e_sum(eS1, ep, sm)
    q = sm / B
    eq = esm / B + U * _m(q, esm / B)
    r = du - q
    er = e_sum(edu, eq, r)
    da, eda = scale * r, e_prod(scale, escale, r, er)
    return ({"du": du, "dz": da * mask, "dgamma": S2, "dbeta": S1}, {"du": edu, "dz": eda * mask, "dgamma": eS2, "dbeta": eS1})


def xhat_of(a, mu, var):
    """(xh, e_xh, inv, e_inv) from a layer's stored a, mu, var taken as exact inputs: what a backward launch recomputes"""
    a, mu, var = (np.asarray(t, np.float64) for t in (a, mu, var))
    d = a - mu
    ed = U * np.abs(d)
    s = var + BN_EPS
    es = U * s
    inv = 1.0 / np.sqrt(s)
    einv = es / (2.0 * (s - es) ** 1.5) + FN * U * inv
    return d * inv, e_prod(d, ed, inv, einv), inv, einv


def stage_forward(h_in, W, b, ga, be, stats=None):
    """one hidden layer from an exact input: (values, bounds) of z, a, mu, var, h (keys without a layer number)"""
    P = {"W1": W, "b1": b, "gamma1": ga, "beta1": be, "Wo": np.zeros((np.shape(W)[1], 1)), "bo": np.zeros(1)}
    v, e = forward(P, h_in, 1, None if stats is None else [stats])
    return ({k[:-1]: t for k, t in v.items() if k.endswith("1")}, {k[:-1]: t for k, t in e.items() if k.endswith("1")})


def stage_head(h_in, Wo, bo, y):
    """the head from an exact input: (values, bounds) of logit, yhat, loss, dlogit"""
    h_in, Wo, bo = (np.asarray(t, np.float64) for t in (h_in, Wo, bo))
    logit = h_in @ Wo + bo
    el = e_matmul(h_in, np.zeros_like(h_in), Wo, bo)
    yhat = 1.0 / (1.0 + np.exp(-logit))
    ey = 0.25 * el + FN * U * yhat
    om = 1.0 - yhat
    v, e = {"logit": logit, "yhat": yhat, "om": om}, {"logit": el, "yhat": ey, "om": ey + U * _m(om, ey)}
    hv, he = head(v, e, y)
    v.update(hv)
    e.update(he)
    return v, e


def backward(P, x, v, e, dlogit, edlogit, L, masks=None):
    """(values, bounds) of dz_i, du_i, dgamma_i, dbeta_i and of the flat gradient "grad", from forward()'s and head()'s results.
    masks: {i: 0 / 1 array} the ReLU masks to use (the reference's own a_i > 0 where None)"""
    f = {k: np.asarray(val, np.float64) for k, val in P.items()}
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    d, ed = {}, {}
    delta, edelta = dlogit, edlogit
    Wup = f["Wo"]
    for i in range(L, 0, -1):
        s = str(i)
        mask = (v["a" + s] > 0).astype(np.float64) if masks is None else np.asarray(masks[i], np.float64)
        lv, le = layer_backward(delta, edelta, Wup, v["xh" + s], e["xh" + s], v["inv" + s], e["inv" + s], f["gamma" + s], mask)
        for k in lv:
            d[k + s], ed[k + s] = lv[k], le[k]
        delta, edelta, Wup = d["dz" + s], ed["dz" + s], f["W" + s]
    # the weight and bias gradients: [X, 1]^T Delta, one chain over the batch per element
    g, eg = {}, {}
    for i in range(1, L + 2):
        tag = "o" if i == L + 1 else str(i)
        X, eX = (x, np.zeros_like(x)) if i == 1 else (v["h%d" % (i - 1)], e["h%d" % (i - 1)])
        D, eD = (dlogit, edlogit) if i == L + 1 else (d["dz" + tag], ed["dz" + tag])
        X1, eX1 = np.hstack([X, np.ones((B, 1))]), np.hstack([eX, np.zeros((B, 1))])
        G = X1.T @ D
        eG = eX1.T @ _m(D, eD) + np.abs(X1).T @ eD + (B + 1) * U * (_m(X1, eX1).T @ _m(D, eD))
        g["W" + tag], g["b" + tag] = G[:-1], G[-1]
        eg["W" + tag], eg["b" + tag] = eG[:-1], eG[-1]
        if i <= L:
            g["gamma" + tag], g["beta" + tag] = d["dgamma" + tag], d["dbeta" + tag]
            eg["gamma" + tag], eg["beta" + tag] = ed["dgamma" + tag], ed["dbeta" + tag]
    d["grad"], ed["grad"] = flat(g, L), flat(eg, L)
    return d, ed


def reference_step(P, x, y, L, masks=None):
    """forward (batch statistics), head and backward: (values, bounds) with everything in one dict each"""
    v, e = forward(P, x, L)
    hv, he = head(v, e, y)
    d, ed = backward(P, x, v, e, hv["dlogit"], he["dlogit"], L, masks)
    v.update(hv)
    v.update(d)
    e.update(he)
    e.update(ed)
    return v, e


def tallies(yhat_ge_half, y):
    """[B, 3] (tp, fp, fn) per example from the decisions and int(y)"""
    pred, truth = np.asarray(yhat_ge_half, bool), np.asarray(y).astype(np.int64) != 0
    return np.stack([(pred & truth).sum(1), (pred & ~truth).sum(1), (~pred & truth).sum(1)], axis=1).astype(np.int32)


def macro_f1(t):
    """util.macroF1 from the tallies: the mean over the examples of 2 tp / (2 tp + fp + fn), 0 where the denominator is 0"""
    t = np.asarray(t, np.float64)
    den = 2 * t[:, 0] + t[:, 1] + t[:, 2]
    return float(np.mean(np.where(den > 0, 2 * t[:, 0] / np.maximum(den, 1), 0.0)))


def fold32(mean, var, mu, sigma2, decay=0.9):
    """one fold of (mu, sigma2) into the moving pair in float32, rounded after every operation"""
    f = np.float32
    d = f(1.0 - decay)
    mean, var, mu, sigma2 = (np.asarray(a, f) for a in (mean, var, mu, sigma2))
    return (mean - ((mean - mu) * d).astype(f)).astype(f), (var - ((var - sigma2) * d).astype(f)).astype(f)


def train64(P, x, y, L, steps, lr=1e-3):
    """`steps` Adam steps in float64 on one fixed batch (TF's form, eps 1e-8): the loss before each step, and the last"""
    theta = flat(P, L).astype(np.float64)
    m, vv = np.zeros_like(theta), np.zeros_like(theta)
    losses = []
    for t in range(1, steps + 1):
        val, _ = reference_step(unflat(theta, P, L), x, y, L)
        losses.append(val["loss"])
        g = val["grad"]
        m = 0.9 * m + 0.1 * g
        vv = 0.999 * vv + 0.001 * g * g
        theta = theta - adam_lr_t(lr, 0.9, 0.999, t) * m / (np.sqrt(vv) + 1e-8)
    val, _ = reference_step(unflat(theta, P, L), x, y, L)
    losses.append(val["loss"])
    return losses
