"""A NumPy restatement of one DDPG training step, written from its description: the forward pass, the
backward pass with the ReLU masks as an INPUT, the weight gradients and the update; and the running error bound of each
quantity.  Everything is float64 except update32, which restates the update in float32 operation by operation.

A net is a dict W1, b1, W2, b2, W3, b3 (W [in, out]):
    policy  a = tanh(relu(relu(o W1 + b1) W2 + b2) W3 + b3)
    critic  q = relu([relu(o W1 + b1), a] W2 + b2) W3 + b3

The bound of a quantity is n u M (Higham's running bound, u = 2^-24): M is the same formula evaluated on the absolute values
of all operands (every subtraction an addition, relu and tanh the identity, a mask 0 / 1), n the number of roundings along
its longest chain: a product with an exact matrix adds its inner dimension, an elementwise operation one, tanh
TANH_ROUNDINGS, the product of two inexact factors the sum of theirs, a sum the larger of the two.  `Exact` and `Mag` are
the two readings of the elementwise operations; step_forward / step_backward run under either.
"""
import math

import numpy as np

U = 2.0 ** -24
TANH_ROUNDINGS = 8
NAMES = ("W1", "b1", "W2", "b2", "W3", "b3")


class Exact:
    mag = False
    sub = staticmethod(lambda a, b: a - b)
    neg = staticmethod(lambda a: -a)
    relu = staticmethod(lambda z: np.maximum(z, 0.0))
    tanh = staticmethod(np.tanh)
    one_minus_sq = staticmethod(lambda a: 1.0 - a * a)


class Mag:
    mag = True
    sub = staticmethod(lambda a, b: a + b)
    neg = staticmethod(lambda a: a)
    relu = staticmethod(lambda z: z)
    tanh = staticmethod(lambda z: z)
    one_minus_sq = staticmethod(lambda a: 1.0 + a * a)


def f64(net):
    return {k: np.asarray(v, np.float64) for k, v in net.items()}


def absnet(net):
    return {k: np.abs(np.asarray(v, np.float64)) for k, v in net.items()}


def flat(net):
    return np.concatenate([np.asarray(net[k]).reshape(-1) for k in NAMES])


def unflat(vec, like):
    out, at = {}, 0
    for k in NAMES:
        n = like[k].size
        out[k] = np.asarray(vec[at:at + n]).reshape(like[k].shape)
        at += n
    return out


def uniform_params(dimO, dimA, l1, l2, seed):
    """uniform +-1/sqrt(fan-in) in every layer, the last included, so that the deltas are O(1); float32"""
    rng = np.random.RandomState(seed)
    out = {}
    for which, shapes in (("p", ((dimO, l1), (l1, l2), (l2, dimA))), ("q", ((dimO, l1), (l1 + dimA, l2), (l2, 1)))):
        net = {}
        for i, (fan_in, fan_out) in enumerate(shapes, 1):
            b = 1.0 / math.sqrt(fan_in)
            net["W%d" % i] = rng.uniform(-b, b, (fan_in, fan_out)).astype(np.float32)
            net["b%d" % i] = rng.uniform(-b, b, (fan_out,)).astype(np.float32)
        out[which] = net
    return out


def batch(B, dimO, dimA, seed):
    """a minibatch: obs, act (float64 holding float32 values), rew, ob2 float32, term uint8 with both values where B > 1"""
    rng = np.random.RandomState(1000 + seed)
    obs = rng.uniform(-1, 1, (B, dimO)).astype(np.float32)
    act = rng.uniform(-1, 1, (B, dimA)).astype(np.float32).astype(np.float64)
    rew = rng.uniform(-1, 1, B).astype(np.float32)
    ob2 = rng.uniform(-1, 1, (B, dimO)).astype(np.float32)
    term = (rng.rand(B) < 0.25).astype(np.uint8)
    if B > 1:
        term[0], term[1] = 1, 0
    return obs, act, rew, ob2, term


def policy(ops, P, o):
    z1 = o @ P["W1"] + P["b1"]
    h1 = ops.relu(z1)
    z2 = h1 @ P["W2"] + P["b2"]
    h2 = ops.relu(z2)
    a = ops.tanh(h2 @ P["W3"] + P["b3"])
    return {"z1": z1, "h1": h1, "z2": z2, "h2": h2, "a": a}


def critic(ops, Q, o, a, h1=None):
    z1 = o @ Q["W1"] + Q["b1"]
    h1 = ops.relu(z1)
    z2 = np.concatenate([h1, a], axis=1) @ Q["W2"] + Q["b2"]
    h2 = ops.relu(z2)
    q = (h2 @ Q["W3"] + Q["b3"])[:, 0]
    return {"z1": z1, "h1": h1, "z2": z2, "h2": h2, "q": q}


def forward_counts(dimO, dimA, l1, l2):
    """n of every forward quantity"""
    n = {}
    n["z1"] = dimO + 1
    n["h1"] = n["z1"] + 1
    n["pz2"] = n["h1"] + l1 + 1
    n["ph2"] = n["pz2"] + 1
    n["a"] = n["ph2"] + l2 + 1 + TANH_ROUNDINGS
    n["qz2"] = n["h1"] + l1 + dimA + 1                       # the minibatch's action is exact
    n["qh2"] = n["qz2"] + 1
    n["q"] = n["qh2"] + l2 + 1
    n["cz2"] = max(n["h1"], n["a"]) + l1 + dimA + 1          # the critic at the policy's action
    n["ch2"] = n["cz2"] + 1
    n["qpi"] = n["ch2"] + l2 + 1
    n["y"] = n["qpi"] + 2                                    # q2 has qpi's chain, then discount q2 and + rew
    n["td"] = max(n["q"], n["y"]) + 1
    return n


def step_forward(ops, P, Q, PT, QT, obs, act, rew, ob2, term, discount):
    """steps 1-3 of the training step without the gradients"""
    t = policy(ops, PT, ob2)
    tq = critic(ops, QT, ob2, t["a"])
    y = np.where(term != 0, rew, rew + discount * tq["q"])
    c = critic(ops, Q, obs, act)
    td = ops.sub(c["q"], y)
    p = policy(ops, P, obs)
    cp = critic(ops, Q, obs, p["a"])
    return {"a2": t["a"], "q2": tq["q"], "y": y, "q": c["q"], "td": td, "a": p["a"], "qpi": cp["q"],
            "qz1": c["z1"], "qh1": c["h1"], "qz2": c["z2"], "qh2": c["h2"],
            "pz1": p["z1"], "ph1": p["h1"], "pz2": p["z2"], "ph2": p["h2"], "cz2": cp["z2"], "ch2": cp["h2"]}


def step_backward(ops, P, Q, fw, masks, B, dimO, dimA, l1, l2):
    """The pre-activation deltas of both losses from the forward quantities fw and the ReLU masks (0 / 1 arrays qh1, qh2,
    ph1, ph2, ch2).  Returns (deltas, n of each)."""
    nf = forward_counts(dimO, dimA, l1, l2)
    d, n = {}, {}
    d["d3q"] = (2.0 * fw["td"] / B)[:, None]
    n["d3q"] = nf["td"] + 2
    d["d2q"] = d["d3q"] * Q["W3"][:, 0][None, :] * masks["qh2"]
    n["d2q"] = n["d3q"] + 1
    d["d1q"] = (d["d2q"] @ Q["W2"][:l1].T) * masks["qh1"]
    n["d1q"] = n["d2q"] + l2
    d2c = ops.neg(np.ones((fw["a"].shape[0], 1)) / B) * Q["W3"][:, 0][None, :] * masks["ch2"]
    da = d2c @ Q["W2"][l1:].T
    d["d3p"] = da * ops.one_minus_sq(fw["a"])
    n["d3p"] = (2 + l2) + (nf["a"] + 2) + 1
    d["d2p"] = (d["d3p"] @ P["W3"].T) * masks["ph2"]
    n["d2p"] = n["d3p"] + dimA
    d["d1p"] = (d["d2p"] @ P["W2"].T) * masks["ph1"]
    n["d1p"] = n["d2p"] + l2
    return d, n


def weight_grads(obs, x_q2, h2q, h1p, h2p, d):
    """(g_q, g_p) flat from the layer inputs and the deltas: dW = X^T Delta, db the column sums, before the decay term"""
    gq = [obs.T @ d["d1q"], d["d1q"].sum(0), x_q2.T @ d["d2q"], d["d2q"].sum(0), h2q.T @ d["d3q"], d["d3q"].sum(0)]
    gp = [obs.T @ d["d1p"], d["d1p"].sum(0), h1p.T @ d["d2p"], d["d2p"].sum(0), h2p.T @ d["d3p"], d["d3p"].sum(0)]
    return np.concatenate([g.reshape(-1) for g in gq]), np.concatenate([g.reshape(-1) for g in gp])


def losses(P, Q, fw, l2norm, pl2norm):
    loss_q = np.mean(fw["td"] ** 2) + l2norm * 0.5 * np.sum(flat(Q) ** 2)
    loss_p = -np.mean(fw["qpi"]) + pl2norm * 0.5 * np.sum(flat(P) ** 2)
    return loss_q, loss_p


def reference_step(P, Q, PT, QT, mb, discount, masks=None):
    """The float64 step and its bounds for float32 nets and a minibatch (obs, act, rew, ob2, term).  masks None: the
    reference's own.  Returns (fw, bound_fw, deltas, bound_deltas, masks, ambiguous): ambiguous[k] marks the units of mask k
    whose pre-activation lies below its own bound."""
    obs, act, rew, ob2, term = (np.asarray(x, np.float64) if i != 4 else np.asarray(x) for i, x in enumerate(mb))
    B, dimO = obs.shape
    dimA, l1, l2 = act.shape[1], P["W1"].shape[1], P["W2"].shape[1]
    fw = step_forward(Exact, f64(P), f64(Q), f64(PT), f64(QT), obs, act, rew, ob2, term, discount)
    mg = step_forward(Mag, absnet(P), absnet(Q), absnet(PT), absnet(QT), np.abs(obs), np.abs(act), np.abs(rew), np.abs(ob2),
                      term, abs(discount))
    nf = forward_counts(dimO, dimA, l1, l2)
    count = {"a2": nf["a"], "q2": nf["qpi"], "y": nf["y"], "q": nf["q"], "td": nf["td"], "a": nf["a"], "qpi": nf["qpi"],
             "qz1": nf["z1"], "qh1": nf["h1"], "qz2": nf["qz2"], "qh2": nf["qh2"], "pz1": nf["z1"], "ph1": nf["h1"],
             "pz2": nf["pz2"], "ph2": nf["ph2"], "cz2": nf["cz2"], "ch2": nf["ch2"]}
    bound_fw = {k: count[k] * U * mg[k] for k in fw}
    pre = {"qh1": "qz1", "qh2": "qz2", "ph1": "pz1", "ph2": "pz2", "ch2": "cz2"}
    own = {k: (fw[z] > 0).astype(np.float64) for k, z in pre.items()}
    ambiguous = {k: np.abs(fw[z]) < bound_fw[z] for k, z in pre.items()}
    masks = own if masks is None else {k: np.asarray(v, np.float64) for k, v in masks.items()}
    d, nd = step_backward(Exact, f64(P), f64(Q), fw, masks, B, dimO, dimA, l1, l2)
    dm, _ = step_backward(Mag, absnet(P), absnet(Q), mg, masks, B, dimO, dimA, l1, l2)
    bound_d = {k: nd[k] * U * dm[k] for k in d}
    return fw, bound_fw, d, bound_d, own, ambiguous


def stage_linear(x, W, b=None):
    """x W + b from operands taken as exact (what one launch read) and its one-layer bound (K + 1) u (|x| |W| + |b|)"""
    x, W = np.asarray(x, np.float64), np.asarray(W, np.float64)
    z, m = x @ W, np.abs(x) @ np.abs(W)
    if b is not None:
        z, m = z + np.asarray(b, np.float64), m + np.abs(np.asarray(b, np.float64))
    return z, (x.shape[1] + 1) * U * m


class Stages:
    """What a stage-wise check collects: want / bound of every stored quantity recomputed from the stored quantities it was
    formed from, and pre[name] = (z, bound) of every ReLU layer, whose sign the stored mask must have wherever |z| > bound."""

    def __init__(self):
        self.want, self.bound, self.pre = {}, {}, {}

    def put(self, name, want, bound):
        self.want[name], self.bound[name] = want, bound

    def relu(self, name, x, W, b):
        z, e = stage_linear(x, W, b)
        self.pre[name] = (z, e)
        self.put(name, np.maximum(z, 0.0), np.where(z < -e, 0.0, e))         # a unit that is off beyond its bound is exactly 0

    def back(self, name, delta, W, h):
        """(delta W^T) [h > 0]: a delta through a layer's weights and the stored activation's sign"""
        z, e = stage_linear(delta, np.asarray(W, np.float64).T)
        mask = np.asarray(h) > 0
        self.put(name, z * mask, e * mask)

    def ambiguous(self):
        return {k: np.abs(z) < e for k, (z, e) in self.pre.items()}


def stage_step(P, Q, obs, dev, B):
    """Every stored layer output and delta of the chain at obs from the stored quantities `dev` it was formed from (xa, h2q, q,
    y, td, d3q, d2q, h1p, h2p, a, h2c, d3p, d2p: float64 arrays as the workspace holds them), each under one layer's rounding:
    a product (K + 1) u (|x| |W| + |b|), tanh TANH_ROUNDINGS more on its value, an elementwise operation u.  The target path
    keeps none of its layers, so a2 and y have no stage of their own."""
    P, Q, obs = f64(P), f64(Q), np.asarray(obs, np.float64)
    l1 = P["W1"].shape[1]
    s = Stages()
    qh1 = dev["xa"][:, :l1]
    s.relu("qh1", obs, Q["W1"], Q["b1"])
    s.relu("h2q", dev["xa"], Q["W2"], Q["b2"])
    z, e = stage_linear(dev["h2q"], Q["W3"], Q["b3"])
    s.put("q", z[:, 0], e[:, 0])
    td = dev["q"] - dev["y"]
    s.put("td", td, U * np.abs(td))
    d3 = 2.0 * dev["td"] / B
    s.put("d3q", d3[:, None], 2 * U * np.abs(d3)[:, None])                   # 1 / B rounded, then one product
    d2 = dev["d3q"] * Q["W3"][:, 0][None, :] * (dev["h2q"] > 0)
    s.put("d2q", d2, U * np.abs(d2))
    s.back("d1q", dev["d2q"], Q["W2"][:l1], qh1)
    s.relu("h1p", obs, P["W1"], P["b1"])
    s.relu("h2p", dev["h1p"], P["W2"], P["b2"])
    z, e = stage_linear(dev["h2p"], P["W3"], P["b3"])
    s.put("a", np.tanh(z), e + TANH_ROUNDINGS * U * np.abs(np.tanh(z)))      # tanh's slope is at most 1
    s.relu("h2c", np.concatenate([qh1, dev["a"]], axis=1), Q["W2"], Q["b2"])
    z, e = stage_linear(dev["h2c"], Q["W3"], Q["b3"])
    s.put("qpi", z[:, 0], e[:, 0])
    # d3p = (d2c W2[action rows]^T) (1 - a^2); d2c = -(1 / B) W3 [h2c > 0] is not stored: two roundings, then the product's
    c = -(1.0 / B) * Q["W3"][:, 0][None, :] * (dev["h2c"] > 0)
    ec = 2 * U * np.abs(c)
    Wa = np.abs(Q["W2"][l1:]).T
    da, eda = c @ Q["W2"][l1:].T, ec @ Wa + (c.shape[1] + 1) * U * ((np.abs(c) + ec) @ Wa)
    w = 1.0 - dev["a"] ** 2
    ew = 2 * U * (1.0 + dev["a"] ** 2)
    s.put("d3p", da * w, eda * (np.abs(w) + ew) + np.abs(da) * ew + U * (np.abs(da) + eda) * (np.abs(w) + ew))
    s.back("d2p", dev["d3p"], P["W3"], dev["h2p"])
    s.back("d1p", dev["d2p"], P["W2"], dev["h1p"])
    return s


def adam_lr_t(lr, beta1, beta2, t):
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def update32(theta, m, v, target, g, t, lr, k, tau, eps=1e-4, beta1=0.9, beta2=0.999):
    """The update of one net in float32, every operation rounded, no contraction: the decay term (k = 0 leaves g), TF-Adam at
    step count t (the count AFTER this update), then the target from the new theta.  Returns (theta, m, v, target)."""
    f = np.float32
    theta, m, v, target, g = (np.asarray(x, f).copy() for x in (theta, m, v, target, g))
    b1, c1, b2, c2 = f(beta1), f(1.0 - beta1), f(beta2), f(1.0 - beta2)
    lr_t = f(adam_lr_t(lr, beta1, beta2, t))
    if f(k) != 0:
        g = g + f(k) * theta
    m = b1 * m + c1 * g
    v = b2 * v + c2 * (g * g)
    theta = theta - (lr_t * m) / (np.sqrt(v) + f(eps))
    target = target - f(tau) * (target - theta)
    return theta, m, v, target
