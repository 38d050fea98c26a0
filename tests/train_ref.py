"""Float64 torch-autograd statement of the reference's training surrogate (test helper; shares no code with the kernels).

The network is written from the layer algebra of multi-label-cls/icnn_ebundle.py:316-388 (RL/src/icnn.py:325-404 with
leaky ReLU z-layers and the action box of :148-158), evaluated on the R GATHERED feed rows with BatchNorm over those
rows, as TensorFlow does with x_ = fd_xs; F = c E + <dE/dy, v> is differentiated with create_graph=True."""
import numpy as np
import torch


def energy(spec, theta, x, y):
    """E[R] of the FC PICNN on rows (x[R], y[R]); theta: dict of float64 tensors."""
    L = len(spec.szs)
    if spec.action_box:
        y = 2.0 * y - 1.0
    us, prev = [], x
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                mean = u.mean(dim=0)
                var = ((u - mean) ** 2).mean(dim=0)
                u = (u - mean) / torch.sqrt(var + 1e-5) * theta["u%d/bn/gamma" % i] + theta["u%d/bn/beta" % i]
        us.append(u)
        prev = u
    prevU, prevZ = x, y
    pre_acts = []
    for i in range(L + 1):
        add = 0.0
        if i > 0:
            zu_u = torch.relu(prevU @ theta["z%d_zu_u/W" % i] + theta["z%d_zu_u/b" % i])
            add = add + (prevZ * zu_u) @ theta["z%d_zu_proj/W" % i]
        yu_u = prevU @ theta["z%d_yu_u/W" % i] + theta["z%d_yu_u/b" % i]
        add = add + (y * yu_u) @ theta["z%d_yu/W" % i]
        add = add + prevU @ theta["z%d_u/W" % i] + theta["z%d_u/b" % i]
        pre_acts.append(add)
        z = add
        if i < L:
            z = torch.where(add > 0, add, spec.alpha * add)
        prevU = us[i] if i < L else None
        prevZ = z
    return z.reshape(-1), pre_acts


def surrogate_grad64(spec, params, x_rows, y, v, c):
    """(grad dict float64 numpy, F_r float64 numpy, min |pre-activation| over the masked layers) -- x_rows [R][features]
    are the gathered samples (float32 values), y/v [R][n] and c [R] float64; v None: F = c E."""
    theta = {k: torch.tensor(np.asarray(p, np.float64), requires_grad=True) for k, p in params.items()}
    x = torch.as_tensor(np.asarray(x_rows, np.float64))
    yt = torch.tensor(np.asarray(y, np.float64).astype(np.float32).astype(np.float64), requires_grad=True)
    ct = torch.as_tensor(np.asarray(c, np.float64).astype(np.float32).astype(np.float64))
    E, pre = energy(spec, theta, x, yt)
    F = ct * E
    if v is not None:
        vt = torch.as_tensor(np.asarray(v, np.float64).astype(np.float32).astype(np.float64))
        dEdy, = torch.autograd.grad(E.sum(), yt, create_graph=True)
        F = F + (dEdy * vt).sum(dim=1)
    gs = torch.autograd.grad(F.sum(), list(theta.values()), allow_unused=True)
    grads = {k: (g.detach().numpy() if g is not None else np.zeros_like(params[k], dtype=np.float64))
             for k, g in zip(theta.keys(), gs)}
    margin = min(float(p.detach().abs().min()) for p in pre[:-1])
    return grads, F.detach().numpy(), margin


def u_margin(spec, params, x_rows):
    """min |pre-ReLU| of the u-path and the gate heads on the gathered rows (float64): the masks the kernels take in float32
    agree with these when it is not tiny."""
    theta = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    x = torch.as_tensor(np.asarray(x_rows, np.float64))
    L = len(spec.szs)
    m, prev, us = np.inf, x, []
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            m = min(m, float(u.abs().min()))
            u = torch.relu(u)
            if spec.batchnorm:
                mean = u.mean(dim=0)
                var = ((u - mean) ** 2).mean(dim=0)
                u = (u - mean) / torch.sqrt(var + 1e-5) * theta["u%d/bn/gamma" % i] + theta["u%d/bn/beta" % i]
        us.append(u)
        prev = u
    for i in range(1, L + 1):
        m = min(m, float((us[i - 1] @ theta["z%d_zu_u/W" % i] + theta["z%d_zu_u/b" % i]).abs().min()))
    return m


def last_u(spec, params, x_rows):
    """u_{L-1} (the linear last u layer, what the final layer's 'z{L}_u' reads) on the gathered rows, float64 [R][width]."""
    theta = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    prev = torch.as_tensor(np.asarray(x_rows, np.float64))
    L = len(spec.szs)
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                mean = u.mean(dim=0)
                var = ((u - mean) ** 2).mean(dim=0)
                u = (u - mean) / torch.sqrt(var + 1e-5) * theta["u%d/bn/gamma" % i] + theta["u%d/bn/beta" % i]
        prev = u
    return prev.numpy()
