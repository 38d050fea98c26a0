"""A NumPy restatement of one NAF training step, written from its description: the forward pass with the
lower-triangular advantage head, the backward pass with the ReLU masks as an INPUT, the weight gradients, and the running
error bound of each quantity.  Everything is float64; the float32 update is ddpg_ref.update32, once per net at one step count.

A net is a dict W1, b1, W2, b2, W3, b3 (W [in, out]);  mlp(o) = relu(relu(o W1 + b1) W2 + b2) W3 + b3:
    l = mlp_L(obs) as [dimA, dimA];  Lm = its strict lower triangle + diag(exp(diag l));  u = tanh(mlp_U(obs))
    delta = act - u;  h = delta Lm;  A = -1/2 sum h^2;  q = mlp_V(obs) + A;  y = term ? rew : rew + discount mlp_VT(ob2)

Bounds.  Inside the three nets (and y) the bound of a quantity is n u M as in ddpg_ref: u = 2^-24, M the same formula on the
absolute values of all operands, n the roundings along its longest chain (`counts`).  Behind the nets' outputs that form
stops saying anything: M of u is the M of tanh's argument (some 80 at the shipped shape where |u| <= 1), h multiplies it with
M of l, and A squares the product (9e8 for values of order 1).  There the same first-order rules are applied to the error e
itself with the true magnitudes, m(x) = |x| + e(x) -- which is n u M with every factor's M renormalised to its value and its
count scaled to keep n M, so never more than n u M allows:
    a sum              e = e_x + e_y + u m(x + y)
    a product          e = e_x m_y + |x| e_y + u m_x m_y
    an fma chain       of k terms: the terms' errors, plus k u times the sum of the terms' m
    tanh               e = e_arg + TANH_ROUNDINGS u |tanh|                      (its slope is at most 1)
    exp                e = exp(x) expm1(e_arg) + EXP_ROUNDINGS u exp(x + e_arg)  (the argument's error is exp's RELATIVE error)
    a product with an exact matrix over k terms     e = e_x |W| + k u (m_x |W|)
EXP_ROUNDINGS is tanh's allowance: the ROCm installation the project builds against ships no math-library document that
states a bound for expf.
"""
import numpy as np

from ddpg_ref import NAMES, TANH_ROUNDINGS, U, Exact, Mag, absnet, adam_lr_t, f64, flat, update32  # noqa: F401
from ddpg_ref import Stages, stage_linear

EXP_ROUNDINGS = TANH_ROUNDINGS
NETS = ("L", "U", "V")


def uniform_params(dimO, dimA, l1, l2, seed):
    """{"L", "U", "V"}: uniform +-1/sqrt(fan-in) in every layer, biases included, so that l, delta and the masks are O(1)"""
    rng = np.random.RandomState(seed)
    out = {}
    for which, width in (("L", dimA * dimA), ("U", dimA), ("V", 1)):
        net = {}
        for i, (fan_in, fan_out) in enumerate(((dimO, l1), (l1, l2), (l2, width)), 1):
            b = 1.0 / np.sqrt(fan_in)
            net["W%d" % i] = rng.uniform(-b, b, (fan_in, fan_out)).astype(np.float32)
            net["b%d" % i] = rng.uniform(-b, b, (fan_out,)).astype(np.float32)
        out[which] = net
    return out


def batch(B, dimO, dimA, seed):
    """a minibatch: obs, act (float64 holding float32 values), rew, ob2 float32, term uint8 with both values where B > 1"""
    rng = np.random.RandomState(2000 + seed)
    obs = rng.uniform(-1, 1, (B, dimO)).astype(np.float32)
    act = rng.uniform(-1, 1, (B, dimA)).astype(np.float32).astype(np.float64)
    rew = rng.uniform(-1, 1, B).astype(np.float32)
    ob2 = rng.uniform(-1, 1, (B, dimO)).astype(np.float32)
    term = (rng.rand(B) < 0.25).astype(np.uint8)
    if B > 1:
        term[0], term[1] = 1, 0
    return obs, act, rew, ob2, term


def mlp(ops, N, o):
    z1 = o @ N["W1"] + N["b1"]
    h1 = ops.relu(z1)
    z2 = h1 @ N["W2"] + N["b2"]
    h2 = ops.relu(z2)
    return {"z1": z1, "h1": h1, "z2": z2, "h2": h2, "out": h2 @ N["W3"] + N["b3"]}


def counts(dimO, l1, l2):
    """n of the quantities inside a net, and of y"""
    n = {}
    n["z1"] = dimO + 1
    n["h1"] = n["z1"] + 1
    n["z2"] = n["h1"] + l1 + 1
    n["h2"] = n["z2"] + 1
    n["out"] = n["h2"] + l2 + 1                                # l, the argument of u's tanh, V's output
    n["y"] = n["out"] + 2
    return n


def lm_of(l3):
    """the strict lower triangle of l3 [B, dimA, dimA] with exp(diagonal) on the diagonal"""
    d = np.arange(l3.shape[1])
    Lm = np.tril(l3, -1)
    Lm[:, d, d] = np.exp(l3[:, d, d])
    return Lm


def step_forward(L, Un, V, VT, obs, act, rew, ob2, term, discount, ops=Exact):
    """steps 1-2 of the training step without the gradients.  ops Mag: only the M of the quantities inside the nets and of y"""
    B, dimA = act.shape
    y = np.where(term != 0, rew, rew + discount * mlp(ops, VT, ob2)["out"][:, 0])
    fl, fu, fv = mlp(ops, L, obs), mlp(ops, Un, obs), mlp(ops, V, obs)
    out = {"y": y, "l": fl["out"], "pre_u": fu["out"], "v": fv["out"][:, 0]}
    for w, f in (("l", fl), ("u", fu), ("v", fv)):
        for k in ("z1", "h1", "z2", "h2"):
            out[k + w] = f[k]
    if ops.mag:
        return out
    u = np.tanh(fu["out"])
    Lm = lm_of(fl["out"].reshape(B, dimA, dimA))
    delta = act - u
    h = np.einsum("bi,bij->bj", delta, Lm)
    adv = -0.5 * np.sum(h * h, axis=1)
    q = fv["out"][:, 0] + adv
    out.update({"u": u, "Lm": Lm, "ld": Lm[:, np.arange(dimA), np.arange(dimA)], "delta": delta, "h": h, "adv": adv, "q": q,
                "td": q - y})
    return out


def forward_errors(fw, mg, n, dimA):
    """e of every forward quantity: n u M inside the nets, the rules of the docstring behind them"""
    a = np.abs
    e = {k + w: n[k] * U * mg[k + w] for k in ("z1", "h1", "z2", "h2") for w in "luv"}
    e["y"] = n["y"] * U * mg["y"]
    e["l"], e["pre_u"], e["v"] = (n["out"] * U * mg[k] for k in ("l", "pre_u", "v"))
    B = len(fw["q"])
    d = np.arange(dimA)
    e["u"] = e["pre_u"] + TANH_ROUNDINGS * U * a(fw["u"])
    e["delta"] = e["u"] + U * (a(fw["delta"]) + e["u"])
    el3 = e["l"].reshape(B, dimA, dimA)
    e["Lm"] = np.tril(el3, -1)
    e["ld"] = fw["ld"] * np.expm1(el3[:, d, d]) + EXP_ROUNDINGS * U * fw["ld"] * np.exp(el3[:, d, d])
    e["Lm"][:, d, d] = e["ld"]
    m_delta, m_Lm = a(fw["delta"]) + e["delta"], a(fw["Lm"]) + e["Lm"]
    e["h"] = (np.einsum("bi,bij->bj", e["delta"], m_Lm) + np.einsum("bi,bij->bj", a(fw["delta"]), e["Lm"])
              + dimA * U * np.einsum("bi,bij->bj", m_delta, m_Lm))
    m_h = a(fw["h"]) + e["h"]
    e["adv"] = 0.5 * np.sum(2 * a(fw["h"]) * e["h"] + e["h"] ** 2, axis=1) + (dimA + 1) * U * 0.5 * np.sum(m_h ** 2, axis=1)
    e["q"] = e["v"] + e["adv"] + U * (a(fw["q"]) + e["v"] + e["adv"])
    e["td"] = e["q"] + e["y"] + U * (a(fw["td"]) + e["q"] + e["y"])
    return e


def step_backward(L, Un, V, fw, e, masks):
    """The pre-activation deltas of loss_q from the forward quantities fw, their errors e and the ReLU masks (0 / 1 arrays
    h1l, h2l, h1u, h2u, h1v, h2v).  Returns (deltas, e of each)."""
    a = np.abs
    B, dimA = fw["u"].shape
    l2 = L["W2"].shape[1]
    d, ed = {}, {}
    d3 = 2.0 * fw["td"] / B
    e_d3 = 2.0 * e["td"] / B + 2 * U * (a(d3) + 2.0 * e["td"] / B)              # 1 / B rounded, then one product
    m_d3 = a(d3) + e_d3
    h, m_h = fw["h"], a(fw["h"]) + e["h"]
    gh = -d3[:, None] * h
    e_gh = e_d3[:, None] * m_h + a(d3)[:, None] * e["h"] + U * m_d3[:, None] * m_h
    m_gh = a(gh) + e_gh
    Lm, delta = fw["Lm"], fw["delta"]
    m_Lm, m_delta = a(Lm) + e["Lm"], a(delta) + e["delta"]
    lower = np.tril(np.ones((dimA, dimA)))
    diag = np.arange(dimA)
    g3 = delta[:, :, None] * gh[:, None, :] * lower[None]                       # [b, i, j] = delta[i] gh[j], i >= j
    e_g3 = (e["delta"][:, :, None] * m_gh[:, None, :] + a(delta)[:, :, None] * e_gh[:, None, :]
            + U * m_delta[:, :, None] * m_gh[:, None, :]) * lower[None]
    t, e_t = g3[:, diag, diag], e_g3[:, diag, diag]                             # the diagonal: times Lm[i][i]
    e_g3[:, diag, diag] = e_t * m_Lm[:, diag, diag] + a(t) * e["ld"] + U * (a(t) + e_t) * m_Lm[:, diag, diag]
    g3[:, diag, diag] = t * Lm[:, diag, diag]
    d["d3l"], ed["d3l"] = g3.reshape(B, dimA * dimA), e_g3.reshape(B, dimA * dimA)
    s = np.einsum("bj,bij->bi", gh, Lm)
    e_s = (np.einsum("bj,bij->bi", e_gh, m_Lm) + np.einsum("bj,bij->bi", a(gh), e["Lm"])
           + dimA * U * np.einsum("bj,bij->bi", m_gh, m_Lm))
    w = 1.0 - fw["u"] ** 2
    e_w = 2 * a(fw["u"]) * e["u"] + e["u"] ** 2 + 2 * U * (1.0 + (a(fw["u"]) + e["u"]) ** 2)
    d["d3u"] = -s * w
    ed["d3u"] = e_s * (a(w) + e_w) + a(s) * e_w + U * (a(s) + e_s) * (a(w) + e_w)
    d["d3v"], ed["d3v"] = d3[:, None], e_d3[:, None]
    for k, N, width in (("l", L, dimA * dimA), ("u", Un, dimA), ("v", V, 1)):
        W3, W2 = np.asarray(N["W3"], np.float64), np.asarray(N["W2"], np.float64)
        d["d2" + k] = (d["d3" + k] @ W3.T) * masks["h2" + k]
        ed["d2" + k] = (ed["d3" + k] @ a(W3).T + width * U * ((a(d["d3" + k]) + ed["d3" + k]) @ a(W3).T)) * masks["h2" + k]
        d["d1" + k] = (d["d2" + k] @ W2.T) * masks["h1" + k]
        ed["d1" + k] = (ed["d2" + k] @ a(W2).T + l2 * U * ((a(d["d2" + k]) + ed["d2" + k]) @ a(W2).T)) * masks["h1" + k]
    return d, ed


def weight_grads(obs, h, d):
    """{"l", "u", "v"}: the flat gradient of each net from the layer inputs (h[k + w]) and the deltas: dW = X^T Delta, db the
    column sums, before the decay term"""
    out = {}
    for w in "luv":
        parts = []
        for X, D in ((obs, d["d1" + w]), (h["h1" + w], d["d2" + w]), (h["h2" + w], d["d3" + w])):
            parts += [(X.T @ D).reshape(-1), D.sum(0)]
        out[w] = np.concatenate(parts)
    return out


def loss_q(nets, fw, l2norm):
    return np.mean(fw["td"] ** 2) + l2norm * 0.5 * sum(np.sum(flat(N) ** 2) for N in nets)


def stage_step(L, Un, V, obs, act, dev, B):
    """Every stored layer output and delta of the chain at obs from the stored quantities `dev` it was formed from (h1, h2,
    d3, d2 of the three nets, l, y: float64 arrays as the workspace holds them), each under its own stage's rounding
    (ddpg_ref.Stages): a layer's product (K + 1) u (|x| |W| + |b|); the head -- u, diag Lm, h, A, q, td and the three d3 -- by
    forward_errors and step_backward entered with the stored l and y as exact and with layer 3's bound for tanh's argument
    and for V's output, which are not stored.  The target pass keeps none of its layers, so y has no stage of its own."""
    nets = {"l": f64(L), "u": f64(Un), "v": f64(V)}
    obs, act = np.asarray(obs, np.float64), np.asarray(act, np.float64)
    dimA = act.shape[1]
    s = Stages()
    for w, N in nets.items():
        s.relu("h1" + w, obs, N["W1"], N["b1"])
        s.relu("h2" + w, dev["h1" + w], N["W2"], N["b2"])
    s.put("l", *stage_linear(dev["h2l"], nets["l"]["W3"], nets["l"]["b3"]))
    pre_u, e_pre_u = stage_linear(dev["h2u"], nets["u"]["W3"], nets["u"]["b3"])
    v, e_v = (t[:, 0] for t in stage_linear(dev["h2v"], nets["v"]["W3"], nets["v"]["b3"]))
    u = np.tanh(pre_u)
    Lm = lm_of(dev["l"].reshape(B, dimA, dimA))
    delta = act - u
    h = np.einsum("bi,bij->bj", delta, Lm)
    adv = -0.5 * np.sum(h * h, axis=1)
    q = v + adv
    d = np.arange(dimA)
    fw = {"y": dev["y"], "l": dev["l"], "pre_u": pre_u, "v": v, "u": u, "Lm": Lm, "ld": Lm[:, d, d], "delta": delta, "h": h,
          "adv": adv, "q": q, "td": q - dev["y"]}
    # forward_errors forms n u M of its inputs; with n = 1 and M = e / u it starts from the bounds given here
    mg = {"l": np.zeros_like(dev["l"]), "pre_u": e_pre_u / U, "v": e_v / U, "y": np.zeros_like(dev["y"])}
    n = {"out": 1, "y": 1}
    for k in ("z1", "h1", "z2", "h2"):
        n[k] = 0
        for w in "luv":
            mg[k + w] = 0.0
    e = forward_errors(fw, mg, n, dimA)
    for k in ("u", "ld", "h", "adv", "q", "td"):
        s.put(k, fw[k], e[k])
    zero = {k + w: np.zeros((B, nets["l"]["W%s" % k[1]].shape[1])) for k in ("h1", "h2") for w in "luv"}
    d3, ed3 = step_backward(nets["l"], nets["u"], nets["v"], fw, e, zero)
    for w, N in nets.items():
        s.put("d3" + w, d3["d3" + w], ed3["d3" + w])
        s.back("d2" + w, dev["d3" + w], N["W3"], dev["h2" + w])
        s.back("d1" + w, dev["d2" + w], N["W2"], dev["h1" + w])
    return s


MASKS = {"h1l": "z1l", "h2l": "z2l", "h1u": "z1u", "h2u": "z2u", "h1v": "z1v", "h2v": "z2v"}


def reference_step(L, Un, V, VT, mb, discount, masks=None):
    """The float64 step and its bounds for float32 nets and a minibatch (obs, act, rew, ob2, term).  masks None: the
    reference's own.  Returns (fw, bound_fw, deltas, bound_deltas, masks, ambiguous): ambiguous[k] marks the units of mask k
    whose pre-activation lies below its own bound.  bound_fw["loss_td"]: the bound of mean td^2."""
    obs, act, rew, ob2, term = (np.asarray(x, np.float64) if i != 4 else np.asarray(x) for i, x in enumerate(mb))
    dimO, dimA, l1, l2 = obs.shape[1], act.shape[1], L["W1"].shape[1], L["W2"].shape[1]
    fw = step_forward(f64(L), f64(Un), f64(V), f64(VT), obs, act, rew, ob2, term, discount)
    mg = step_forward(absnet(L), absnet(Un), absnet(V), absnet(VT), np.abs(obs), np.abs(act), np.abs(rew), np.abs(ob2), term,
                      abs(discount), ops=Mag)
    bound_fw = forward_errors(fw, mg, counts(dimO, l1, l2), dimA)
    own = {k: (fw[z] > 0).astype(np.float64) for k, z in MASKS.items()}
    ambiguous = {k: np.abs(fw[z]) < bound_fw[z] for k, z in MASKS.items()}
    masks = own if masks is None else {k: np.asarray(v, np.float64) for k, v in masks.items()}
    d, bound_d = step_backward(f64(L), f64(Un), f64(V), fw, bound_fw, masks)
    bound_fw["loss_td"] = np.mean(2 * np.abs(fw["td"]) * bound_fw["td"] + bound_fw["td"] ** 2)
    return fw, bound_fw, d, bound_d, own, ambiguous
