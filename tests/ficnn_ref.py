"""Float64 torch restatement of the FICNN of synthetic-cls/icnn.py:213-234 for tests/test_ficnn*.py (shares no code with
the kernels): the reference loop as written, with its never-reassigned z, and the energy of both heads."""
import numpy as np
import torch


def reference_loop(spec, theta, x, y):
    """f_ficnn literally: the last layer (sz == 1) does not reassign z, so flatten(z) is the last hidden layer [B, s]"""
    xy = torch.cat([x, y], 1)
    prevZ, z = None, None
    for i, sz in enumerate(list(spec.szs) + [1]):
        z_add = [xy @ theta["z_x%d/W" % i] + theta["z_x%d/b" % i]]
        if prevZ is not None:
            z_add.append(prevZ @ theta["z_z%d_proj/W" % i])
        if sz != 1:
            z = torch.relu(sum(z_add))
        prevZ = z
    return z.reshape(z.shape[0], -1)


def energy(spec, theta, x, y):
    """(E [B], the hidden pre-activations): head 'sum' E = sum_k z_{L-1,k}, head 'linear' E = a_L"""
    xy = torch.cat([x, y], 1)
    L = len(spec.szs)
    z, pre = None, []
    for i in range(L + 1):
        a = xy @ theta["z_x%d/W" % i] + theta["z_x%d/b" % i]
        if i > 0:
            a = a + z @ theta["z_z%d_proj/W" % i]
        if i < L:
            pre.append(a)
            z = torch.relu(a)
        else:
            last = a
    E = z.sum(1) if spec.head == "sum" else last[:, 0]
    return E, pre


def fg64(spec, params, x, y):
    """(E, dE/dy, min |hidden pre-activation| per row, |E|-magnitude, |dE/dy|-magnitude) in float64.  The magnitudes are
    the same network with every weight, bias and input replaced by its absolute value: the sums float32 rounding scales
    with."""
    theta = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    X = torch.tensor(np.asarray(x, np.float64))
    Y = torch.tensor(np.asarray(y, np.float64), requires_grad=True)
    E, pre = energy(spec, theta, X, Y)
    g, = torch.autograd.grad(E.sum(), Y)
    margin = torch.stack([p.abs().min(1).values for p in pre], 1).min(1).values
    ta = {k: v.abs() for k, v in theta.items()}
    Ya = Y.detach().abs().requires_grad_(True)
    Ea, _ = energy(spec, ta, X.abs(), Ya)
    ga, = torch.autograd.grad(Ea.sum(), Ya)
    return (E.detach().numpy(), g.numpy(), margin.detach().numpy(), Ea.detach().numpy(), ga.numpy())


def wide_params(spec, seed, scale=1.0):
    """weights with O(1) pre-activations (std 1/sqrt(fan-in)), non-negative proj weights, non-zero biases"""
    rng = np.random.RandomState(seed)
    from icnn_amd import ficnn
    p = {}
    for name, shape in ficnn.grad_layout(spec):
        if name.endswith("/b"):
            p[name] = (0.3 * rng.randn(*shape)).astype(np.float32)
        elif "proj" in name:
            p[name] = np.abs(rng.randn(*shape) * scale / np.sqrt(shape[0])).astype(np.float32)
        else:
            p[name] = (rng.randn(*shape) * scale / np.sqrt(shape[0])).astype(np.float32)
    return p


def surrogate_grad64(spec, params, x, counts, y, v, c):
    """float64 autograd of F = sum_r c_r E_r + <dE/dy_r, v_r> over every variable, rows of sample j repeated counts[j]
    times (v None: no tangent term).  Returns (gradient {name: ndarray}, F_r [R])."""
    theta = {k: torch.tensor(np.asarray(p, np.float64), requires_grad=True) for k, p in params.items()}
    X = torch.tensor(np.repeat(np.asarray(x, np.float64), counts, axis=0))
    Y = torch.tensor(np.asarray(y, np.float64), requires_grad=True)
    E, _ = energy(spec, theta, X, Y)
    F = torch.tensor(np.asarray(c, np.float64)) * E
    if v is not None:
        g, = torch.autograd.grad(E.sum(), Y, create_graph=True)
        F = F + (g * torch.tensor(np.asarray(v, np.float64))).sum(1)
    names = list(theta)
    gs = torch.autograd.grad(F.sum(), [theta[k] for k in names], allow_unused=True)
    out = {k: (np.zeros(params[k].shape) if gg is None else gg.numpy()) for k, gg in zip(names, gs)}
    return out, F.detach().numpy()
