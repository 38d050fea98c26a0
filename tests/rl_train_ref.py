"""Host restatement of the RL agent's critic training step, `Agent.train()` of RL/src/icnn.py:304-323 with
FLAGS.icnn_opt == 'adam' (test helper; shares no code with the kernels):
    act2           oracle.adam_oracle.adam with entropy_fg around the float32 PICNN chain of oracle/picnn_oracle.py
    the gradient   tests/train_ref.energy in float64 autograd
    TD, decay, TF-Adam, proj, Polyak   NumPy float32 in the order of include/icnn_be.h (icnn_be_rl_td,
                   icnn_be_rl_critic_update)."""
import numpy as np
import torch

import train_ref
from oracle import adam_oracle

F32 = np.float32
B1, B2, EPS = 0.9, 0.999, 1e-8


def layout_names(spec):
    from icnn_amd import train
    return train.grad_layout(spec)


def decayed(name):
    """the variables of tflearn's fully_connected(weight_decay=...): every W, no bias, no BatchNorm gamma / beta"""
    return name.endswith("/W")


def entropy_sum(act):
    """sum_i pen(act_i) per sample, sequential float32 (adam_oracle.entropy_fg's order)"""
    pen, _ = adam_oracle.entropy_terms(np.asarray(act, np.float64).astype(F32))
    tot = np.zeros(pen.shape[0], F32)
    for j in range(pen.shape[1]):
        tot = tot + pen[:, j]
    return tot


def td(e_critic, act, rew, term, q2_src, act2, discount, B):
    """(q, y, td, c) float32 / float64 c: icnn_be_rl_td's per-sample part.  act2 None: q2_src is negQ_entr already."""
    e = np.asarray(e_critic, F32)
    q = -(e + entropy_sum(act))
    q2 = -np.asarray(q2_src, F32) if act2 is None else -(np.asarray(q2_src, F32) + entropy_sum(act2))
    rew = np.asarray(rew, F32)
    y = np.where(np.asarray(term, bool), rew, rew + F32(discount) * q2).astype(F32)
    y = np.maximum(q - F32(1), y)
    y = np.minimum(q + F32(1), y)
    t = (q - y).astype(F32)
    c = (-(F32(1.0 / B) * (F32(2) * t))).astype(F32).astype(np.float64)
    return q, y, t, c


def reg_sum(theta, mask):
    th = np.asarray(theta, np.float64)[np.asarray(mask, bool)]
    return float(np.dot(th, th))


def loss(td_vals, theta, mask, l2norm, wd):
    """icnn_be_rl_td's loss: double from float32 inputs, rounded once"""
    t = np.asarray(td_vals, F32).astype(np.float64)
    return F32(np.sum(t * t) / t.size + float(F32(l2norm)) * (float(F32(wd)) * reg_sum(theta, mask) * 0.5))


def critic_update(theta, theta_t, m, v, g, t, mask, proj, lr, tau, l2norm, wd):
    """icnn_be_rl_critic_update in NumPy float32: Polyak from the pre-update theta, decay, TF-Adam, proj."""
    theta, theta_t, m, v, g = (np.array(a, F32) for a in (theta, theta_t, m, v, g))
    old = theta.copy()
    theta_t = theta_t - F32(tau) * (theta_t - old)
    k = F32(F32(l2norm) * F32(wd))
    mk = np.asarray(mask, bool)
    g = np.where(mk, g + k * old, g).astype(F32)
    b1, c1, b2, c2 = F32(B1), F32(1.0 - B1), F32(B2), F32(1.0 - B2)
    lr_t = F32(lr * np.sqrt(1.0 - B2 ** t) / (1.0 - B1 ** t))
    m = b1 * m + c1 * g
    v = b2 * v + c2 * (g * g)
    theta = theta - (lr_t * m) / (np.sqrt(v) + F32(EPS))
    for b, e in proj:
        seg = theta[b:e]
        theta[b:e] = np.where(seg < 0, F32(0), seg)
    return theta, theta_t, m, v


def closed_form_grad(spec, params, obs, act, c, l2norm, wd):
    """sum_j c_j dE_j/dtheta + l2norm wd W on the decayed variables, float64 (dict)"""
    g, _, _ = train_ref.surrogate_grad64(spec, params, obs, act, None, c)
    return {k: g[k] + (l2norm * wd * np.asarray(params[k], np.float64) if decayed(k) else 0.0) for k in g}


def autograd_loss_grad(spec, params, obs, act, y, act_entropy, l2norm, wd):
    """float64 autograd of the full loss mean((q - y)^2) + l2norm sum_W wd |W|^2 / 2 with y held fixed
    (tf.stop_gradient), q = -(negQ(obs, act) + sum pen(act))"""
    theta = {k: torch.tensor(np.asarray(p, np.float64), requires_grad=True) for k, p in params.items()}
    x = torch.as_tensor(np.asarray(obs, np.float64))
    a = torch.as_tensor(np.asarray(act, np.float64))
    E, _ = train_ref.energy(spec, theta, x, a)
    q = -(E + torch.as_tensor(np.asarray(act_entropy, np.float64)))
    tdv = q - torch.as_tensor(np.asarray(y, np.float64))
    L = (tdv ** 2).mean()
    for k, p in theta.items():
        if decayed(k):
            L = L + l2norm * wd * (p ** 2).sum() / 2
    gs = torch.autograd.grad(L, list(theta.values()))
    return {k: g.numpy() for k, g in zip(theta.keys(), gs)}, tdv.detach().numpy()


def target_actions(spec, params_t, ctx2_host, max_iter=1000):
    """act2, iterations, f_best of the inner Adam on the target (the context rows given, as tests/test_adam.py does)"""
    from oracle import picnn_oracle
    chain = picnn_oracle.make_fg_chain(params_t, ctx2_host, list(spec.szs), spec.alpha, False)
    func = adam_oracle.entropy_fg(lambda obs, a: chain(a))
    return adam_oracle.adam(func, ctx2_host, spec.n_labels, max_iter)
