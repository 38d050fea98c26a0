"""A NumPy restatement of one NAF training step with BatchNorm, naf_bn True, written from its description:
the four forward passes, the head of naf_ref, the backward pass with the ReLU masks as an INPUT, the gradients of every W, b
and beta, the fold of the moving pairs, and the running error bound of each quantity.  Everything is float64; the float32
update is ddpg_ref.update32 and the float32 fold is fold32.

A net is a dict W1, b1, W2, b2, W3, b3, beta0, beta1, beta2 (W [in, out]).  One BatchNorm site on a column x over the batch:
    mu = mean_b x,  var = mean_b (x - mu)^2  (or the net's moving pair),  inv = 1 / sqrt(var + 1e-3),  xh = (x - mu) inv
    h0 = xh(obs) + beta0;  z1 = h0 W1 + b1,  h1 = relu(xh(z1) + beta1);  z2 = h1 W2 + b2,  h2 = relu(xh(z2) + beta2)
    out = h2 W3 + b3;  the head and q are naf_ref's;  y = term ? rew : rew + discount out_T(ob2)
where the target pass T reads the target's W and b with V's betas.  Backward through a site, dout the gradient at its
output (behind the ReLU mask):  dbeta = sum_b dout,  dz = inv (dout - mean_b dout - xh mean_b(dout xh)).

Bounds (u = 2^-24): ff_ref's first-order rules applied to the error itself, e_sum, e_prod, e_matmul (a product with an
exact matrix: k + 1 roundings on the magnitudes), e_rowsum (a sum over B rows: B roundings on the sum of magnitudes), one
more rounding for a division by B, FN = 8 roundings for 1 / sqrt.  The mean is formed as x_0 + mean(x - x_0) (include/
icnn_be.h), so its bound runs through the differences.  relu passes e on, except where the value is below -e: that unit is
0 exactly on both sides.  The head's rules are naf_ref.forward_errors', entered with the bounds of l, of tanh's argument,
of V's output and of y.  b1 and b2 stand in front of a BatchNorm, so their gradients are sums that cancel to zero: their
bound is the absolute bound of that sum, (B + 1) u sum |dz| plus the deltas' own errors, like every other gradient's.
"""
import numpy as np

import naf_ref
from ddpg_ref import U, f64, update32  # noqa: F401
from ff_ref import FN, _m, e_matmul, e_prod, e_rowsum, e_sum

BN_EPS = float(np.float32(1e-3))
BN_DECAY = 0.999
NETS = ("L", "U", "V")
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3", "beta0", "beta1", "beta2")
PLAIN = NAMES[:6]
MASKS = {"h1": "o1", "h2": "o2"}         # a mask and the BatchNorm output whose sign it is


def uniform_params(dimO, dimA, l1, l2, seed):
    """naf_ref.uniform_params with betas uniform in +-0.5: units on in about half of the rows"""
    out = naf_ref.uniform_params(dimO, dimA, l1, l2, seed)
    rng = np.random.RandomState(5000 + seed)
    for which in NETS:
        for i, w in enumerate((dimO, l1, l2)):
            out[which]["beta%d" % i] = rng.uniform(-0.5, 0.5, w).astype(np.float32)
    return out


def moving_stats(dimO, l1, l2, seed):
    """{"L", "U", "V"}: non-trivial moving pairs mean0, var0, ..: means around 0.1, variances in [0.2, 1.7)"""
    rng = np.random.RandomState(6000 + seed)
    out = {}
    for which in NETS:
        out[which] = {}
        for i, w in enumerate((dimO, l1, l2)):
            out[which]["mean%d" % i] = (0.1 + 0.2 * rng.randn(w)).astype(np.float32)
            out[which]["var%d" % i] = rng.uniform(0.2, 1.7, w).astype(np.float32)
    return out


def flat(net, names=NAMES):
    return np.concatenate([np.asarray(net[k]).reshape(-1) for k in names])


def unflat(vec, like, names=NAMES):
    out, at = {}, 0
    for k in names:
        n = like[k].size
        out[k] = np.asarray(vec[at:at + n]).reshape(like[k].shape)
        at += n
    return out


def flat_moving(mv):
    return np.concatenate([np.asarray(mv[k + str(i)]) for i in range(3) for k in ("mean", "var")])


def site(x, ex, beta, stats=None):
    """one BatchNorm site: (values, bounds) of mu, var, inv, xh and o = xh + beta; stats (mean, var): inference mode"""
    B = x.shape[0]
    if stats is None:
        s = x - x[0]                                            # the mean relative to the first row
        es = e_sum(ex, ex[0], s)
        sm = s.mean(0)
        esm = e_rowsum(s, es) / B
        esm = esm + U * _m(sm, esm)
        mu = x.mean(0)
        emu = e_sum(ex[0], esm, mu)
        d = x - mu
        ed = e_sum(ex, emu, d)
        dd, edd = d * d, e_prod(d, ed, d, ed)
        var = dd.mean(0)
        evar = e_rowsum(dd, edd) / B
        evar = evar + U * _m(var, evar)
    else:
        mu, var = (np.asarray(t, np.float64) for t in stats)
        emu, evar = np.zeros_like(mu), np.zeros_like(var)
        d = x - mu
        ed = e_sum(ex, emu, d)
    s = var + BN_EPS
    es = evar + U * _m(s, evar)
    assert np.all(es < 0.5 * s)
    inv = 1.0 / np.sqrt(s)
    einv = es / (2.0 * (s - es) ** 1.5) + FN * U * inv
    xh, exh = d * inv, e_prod(d, ed, inv, einv)
    o = xh + beta
    eo = e_sum(exh, 0.0, o)
    return ({"mu": mu, "var": var, "inv": inv, "xh": xh, "o": o}, {"mu": emu, "var": evar, "inv": einv, "xh": exh, "o": eo})


def net_forward(N, betas, x, stats=None):
    """(values, bounds) of one pass: W and b from N, the betas from `betas`; keys mu0, var0, inv0, xh0, h0, z1, mu1, .., o1, h1,
    .., h2, out.  stats: a dict mean0, var0, .. = inference mode"""
    N, betas = f64(N), f64(betas)
    x = np.asarray(x, np.float64)
    v, e = {}, {}
    h, eh = x, np.zeros_like(x)
    for i in range(3):
        if i:
            W, b = N["W%d" % i], N["b%d" % i]
            z, ez = h @ W + b, e_matmul(h, eh, W, b)
            v["z%d" % i], e["z%d" % i] = z, ez
        else:
            z, ez = h, eh
        sv, se = site(z, ez, betas["beta%d" % i], None if stats is None else (stats["mean%d" % i], stats["var%d" % i]))
        for k in sv:
            v[k + str(i)], e[k + str(i)] = sv[k], se[k]
        if i:
            h, eh = np.maximum(sv["o"], 0.0), np.where(sv["o"] < -se["o"], 0.0, se["o"])
        else:
            h, eh = sv["o"], se["o"]
        v["h%d" % i], e["h%d" % i] = h, eh
    v["out"], e["out"] = h @ N["W3"] + N["b3"], e_matmul(h, eh, N["W3"], N["b3"])
    return v, e


def head_forward(out_l, out_u, out_v, y, act, e_l, e_u, e_v, e_y):
    """naf_ref's head on the three outputs: (fw, bounds) with naf_ref's keys"""
    B, dimA = act.shape
    u = np.tanh(out_u)
    Lm = naf_ref.lm_of(out_l.reshape(B, dimA, dimA))
    delta = act - u
    h = np.einsum("bi,bij->bj", delta, Lm)
    adv = -0.5 * np.sum(h * h, axis=1)
    q = out_v + adv
    d = np.arange(dimA)
    fw = {"y": y, "l": out_l, "pre_u": out_u, "v": out_v, "u": u, "Lm": Lm, "ld": Lm[:, d, d], "delta": delta, "h": h, "adv": adv,
          "q": q, "td": q - y}
    # forward_errors forms n u M of its inputs; with n = 1 and M = e / u it starts from the bounds given here
    mg = {"l": e_l / U, "pre_u": e_u / U, "v": e_v / U, "y": e_y / U}
    n = {"out": 1, "y": 1}
    for k in ("z1", "h1", "z2", "h2"):
        n[k] = 0
        for w in "luv":
            mg[k + w] = 0.0
    e = naf_ref.forward_errors(fw, mg, n, dimA)
    return fw, e


def step_forward(nets, target, mb, discount, stats=None):
    """the four passes and the head: (passes {"L", "U", "V", "T": (values, bounds)}, fw, bounds of fw)"""
    obs, act, rew, ob2, term = mb
    act, rew = np.asarray(act, np.float64), np.asarray(rew, np.float64)
    p = {w: net_forward(nets[w], nets[w], obs, None if stats is None else stats[w]) for w in NETS}
    p["T"] = net_forward(target, nets["V"], ob2, None if stats is None else stats["V"])
    fw, e = head_from_outputs({w: p[w][0]["out"] for w in p}, {w: p[w][1]["out"] for w in p}, mb, discount)
    return p, fw, e


def head_from_outputs(out, eout, mb, discount):
    """y and the head from the outputs of the four passes {"L", "U", "V", "T"} and their bounds: (fw, bounds of fw)"""
    _, act, rew, _, term = mb
    act, rew = np.asarray(act, np.float64), np.asarray(rew, np.float64)
    ot, eot = out["T"][:, 0], eout["T"][:, 0]
    y = np.where(term != 0, rew, rew + discount * ot)
    ey = np.where(term != 0, 0.0, abs(discount) * eot + 2 * U * (np.abs(rew) + abs(discount) * (np.abs(ot) + eot)))
    return head_forward(out["L"], out["U"], out["V"][:, 0], y, act, eout["L"], eout["U"], eout["V"][:, 0], ey)


def stage_forward(h_in, W, b, beta):
    """one hidden layer and its site from an exact input (what a forward launch read): (values, bounds) with site()'s keys and
    z, h = relu(o)"""
    h_in, W, b, beta = (np.asarray(t, np.float64) for t in (h_in, W, b, beta))
    z, ez = h_in @ W + b, e_matmul(h_in, np.zeros_like(h_in), W, b)
    v, e = site(z, ez, beta)
    v["z"], e["z"] = z, ez
    v["h"], e["h"] = np.maximum(v["o"], 0.0), np.where(v["o"] < -e["o"], 0.0, e["o"])
    return v, e


def stage_output(h2, W3, b3):
    """layer 3 from an exact h2: (out, bound)"""
    h2, W3, b3 = (np.asarray(t, np.float64) for t in (h2, W3, b3))
    return h2 @ W3 + b3, e_matmul(h2, np.zeros_like(h2), W3, b3)


def stage_backward(delta, Wup, mask, xh, var):
    """site_backward from exact operands (what a backward launch read: the delta above, that layer's W [N, K], the stored
    activation's sign, the stored xhat and variance): (values, bounds) of dout, dbeta, dz"""
    delta, Wup, xh, var = (np.asarray(t, np.float64) for t in (delta, Wup, xh, var))
    s = var + BN_EPS
    es = U * s
    inv = 1.0 / np.sqrt(s)
    einv = es / (2.0 * (s - es) ** 1.5) + FN * U * inv
    return site_backward(delta, np.zeros_like(delta), Wup, np.asarray(mask, np.float64), {"xh0": xh, "inv0": inv},
                         {"xh0": np.zeros_like(xh), "inv0": einv}, 0)


def head_backward(nets, fw, e):
    """layer 3's deltas d3L, d3U, d3V and their bounds from head_forward's results (naf_ref.step_backward's head part)"""
    plain = {w: f64({k: nets[w][k] for k in PLAIN}) for w in NETS}
    B = fw["q"].shape[0]
    zero = {k + w: np.zeros((B, plain["L"]["W%s" % k[1]].shape[1])) for k in ("h1", "h2") for w in "luv"}
    d3, ed3 = naf_ref.step_backward(plain["L"], plain["U"], plain["V"], fw, e, zero)
    return {"d3" + w: d3["d3" + w.lower()] for w in NETS}, {"d3" + w: ed3["d3" + w.lower()] for w in NETS}


def site_backward(delta, edelta, Wup, mask, v, e, i):
    """through layer i's product and site: (values, bounds) of dout (masked), dbeta, dz"""
    B = delta.shape[0]
    du = (delta @ Wup.T) * mask
    edu = e_matmul(delta, edelta, Wup.T, None) * mask
    xh, exh, inv, einv = v["xh%d" % i], e["xh%d" % i], v["inv%d" % i], e["inv%d" % i]
    t2, et2 = du * xh, e_prod(du, edu, xh, exh)
    S1, eS1 = du.sum(0), e_rowsum(du, edu)
    S2, eS2 = t2.sum(0), e_rowsum(t2, et2)
    m1, m2 = S1 / B, S2 / B
    em1, em2 = eS1 / B + U * _m(m1, eS1 / B), eS2 / B + U * _m(m2, eS2 / B)
    r = du - m1
    er = e_sum(edu, em1, r)
    p, ep = xh * m2, e_prod(xh, exh, m2, em2)
    r2 = r - p
    er2 = e_sum(er, ep, r2)
    dz, edz = inv * r2, e_prod(inv, einv, r2, er2)
    return {"dout": du, "dbeta": S1, "dz": dz}, {"dout": edu, "dbeta": eS1, "dz": edz}


def step_backward(nets, p, fw, e, masks):
    """The deltas and the flat gradients (before the decay term) of the three nets.  masks {"h1L", "h2L", "h1U", ..}: 0 / 1
    arrays.  Returns (d, bounds): d3 / dz2 / dz1 / dbeta0..2 + the net's letter, and "g" + letter the flat gradient."""
    B, dimA = fw["u"].shape
    d3, ed3 = head_backward(nets, fw, e)
    d, ed = {}, {}
    for w in NETS:
        N = f64(nets[w])
        v, ev = p[w]
        delta, edelta = d3["d3" + w], ed3["d3" + w]
        d["d3" + w], ed["d3" + w] = delta, edelta
        g, eg = {}, {}
        deltas = {3: (delta, edelta)}
        for i in (2, 1):
            sv, se = site_backward(delta, edelta, N["W%d" % (i + 1)], masks["h%d" % i + w], v, ev, i)
            d["dz%d" % i + w], ed["dz%d" % i + w] = sv["dz"], se["dz"]
            g["beta%d" % i], eg["beta%d" % i] = sv["dbeta"], se["dbeta"]
            delta, edelta = sv["dz"], se["dz"]
            deltas[i] = (delta, edelta)
        dh0 = delta @ N["W1"].T
        edh0 = e_matmul(delta, edelta, N["W1"].T, None)
        g["beta0"], eg["beta0"] = dh0.sum(0), e_rowsum(dh0, edh0)
        for i in (1, 2, 3):                                     # [X, 1]^T Delta, one chain over the batch per element
            X, eX = v["h%d" % (i - 1)], ev["h%d" % (i - 1)]
            X1, eX1 = np.hstack([X, np.ones((B, 1))]), np.hstack([eX, np.zeros((B, 1))])
            D, eD = deltas[i]
            G = X1.T @ D
            eG = eX1.T @ _m(D, eD) + np.abs(X1).T @ eD + (B + 1) * U * (_m(X1, eX1).T @ _m(D, eD))
            g["W%d" % i], g["b%d" % i], eg["W%d" % i], eg["b%d" % i] = G[:-1], G[-1], eG[:-1], eG[-1]
        for k in g:
            d[k + w], ed[k + w] = g[k], eg[k]
        d["g" + w], ed["g" + w] = flat(g), flat(eg)
    return d, ed


def reference_step(nets, target, mb, discount, masks=None):
    """The float64 step and its bounds.  nets {"L", "U", "V"}, target: V's target (W and b).  masks None: the reference's own.
    Returns (p, fw, bound_fw, d, bound_d, own masks, ambiguous)."""
    p, fw, e = step_forward(nets, target, mb, discount)
    own = {k + w: (p[w][0][o] > 0).astype(np.float64) for k, o in MASKS.items() for w in NETS}
    ambiguous = {k + w: np.abs(p[w][0][o]) < p[w][1][o] for k, o in MASKS.items() for w in NETS}
    masks = own if masks is None else {k: np.asarray(m, np.float64) for k, m in masks.items()}
    d, ed = step_backward(nets, p, fw, e, masks)
    e["loss_td"] = np.mean(2 * np.abs(fw["td"]) * e["td"] + e["td"] ** 2)
    return p, fw, e, d, ed, own, ambiguous


def margin(p):
    """the smallest |o| / bound over the masked sites of the passes that have a backward"""
    return min((np.abs(p[w][0][o]) / p[w][1][o]).min() for o in MASKS.values() for w in NETS)


def loss_q(nets, fw, l2norm):
    """the betas are not in theta (naf.py:77): the sum of squares runs over W and b"""
    return np.mean(fw["td"] ** 2) + l2norm * 0.5 * sum(np.sum(flat(f64(nets[w]), PLAIN) ** 2) for w in NETS)


def fold32(mv, stat, decay=BN_DECAY):
    """m <- m - (m - stat) (1 - decay) in float32, rounded after every operation (flat vectors of one layout)"""
    f = np.float32
    d = f(1.0 - decay)
    mv, stat = np.asarray(mv, f), np.asarray(stat, f)
    return (mv - ((mv - stat).astype(f) * d).astype(f)).astype(f)
