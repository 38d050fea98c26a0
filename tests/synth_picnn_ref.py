"""Statements of the FC PICNN whose last u-layer is ReLU'd (picnn.FCSpec.relu_last_u: the PICNN of synthetic-cls/icnn.py)
for tests/test_synth_picnn.py; shares no code with the kernels or with icnn_amd.picnn.

    energy               float64 torch layer algebra, BatchNorm over the rows it is given, the flag honoured
    surrogate_grad64     float64 double-backward of F = c E + <dE/dy, v> over every variable
    unrolled_autograd    float64 autograd through the momentum-GD recurrence with the z-path masks taken at GIVEN points (the
                         device trajectory), not at the float64 iterates
    f_picnn_literal      the synthetic script's loop as it is written (prevU / prevZ, a u-layer for every sz != 1, all ReLU'd)
    context_by_hand      the float32 torch chain (addmm, relu, ...) of the context row
    small_problem        screened seeds for the small specs
"""
import numpy as np
import torch

from icnn_amd import picnn

MARGIN = 1e-4           # tests/test_train_grad.py's screening margin


def _bn(u, theta, i):
    mean = u.mean(dim=0)
    var = ((u - mean) ** 2).mean(dim=0)
    return (u - mean) / torch.sqrt(var + 1e-5) * theta["u%d/bn/gamma" % i] + theta["u%d/bn/beta" % i]


def u_path(spec, theta, x):
    """([u_0 .. u_{L-1}] as the next stage reads them, [their pre-ReLU values; None for a linear last layer])"""
    L = len(spec.szs)
    us, pres, prev = [], [], x
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            pres.append(u)
            u = torch.relu(u)
            if spec.batchnorm:
                u = _bn(u, theta, i)
        elif spec.relu_last_u:
            pres.append(u)
            u = torch.relu(u)
        else:
            pres.append(None)
        us.append(u)
        prev = u
    return us, pres


def energy(spec, theta, x, y, mask_at=None):
    """(E [R], z-path pre-activations of the masked layers, gate pre-activations, u-path pre-ReLU values).  mask_at: evaluate
    the z-path ReLU masks at those y instead of at y (detached: E stays linear in y between the masks)."""
    L = len(spec.szs)
    us, u_pre = u_path(spec, theta, x)

    def z_path(yy, masks):
        prevU, prevZ, pre, gates, out = x, None, [], [], []
        for i in range(L + 1):
            add = (yy * (prevU @ theta["z%d_yu_u/W" % i] + theta["z%d_yu_u/b" % i])) @ theta["z%d_yu/W" % i]
            add = add + prevU @ theta["z%d_u/W" % i] + theta["z%d_u/b" % i]
            if i > 0:
                g = prevU @ theta["z%d_zu_u/W" % i] + theta["z%d_zu_u/b" % i]
                gates.append(g)
                add = add + (prevZ * torch.relu(g)) @ theta["z%d_zu_proj/W" % i]
            if i < L:
                pre.append(add)
                m = (add > 0) if masks is None else masks[i]
                out.append(m)
                prevZ = torch.where(m, add, spec.alpha * add)
                prevU = us[i]
            else:
                prevZ = add
        return prevZ.reshape(-1), pre, gates, out

    masks = None
    if mask_at is not None:
        with torch.no_grad():
            masks = z_path(mask_at, None)[3]
    E, pre, gates, _ = z_path(y, masks)
    return E, pre, gates, u_pre


def _theta(params, grad=True):
    return {k: torch.tensor(np.asarray(p, np.float64), requires_grad=grad) for k, p in params.items()}


def margins(spec, params, x_rows, y):
    """(min |pre-activation| over u-path, gates and masked z-layers, float64; the last u-layer's pre-ReLU values)"""
    with torch.no_grad():
        _, pre, gates, u_pre = energy(spec, _theta(params, False), torch.as_tensor(np.asarray(x_rows, np.float64)),
                                      torch.as_tensor(np.asarray(y, np.float64)))
    vals = [p for p in pre + gates + u_pre if p is not None]
    last = u_pre[-1].numpy() if u_pre[-1] is not None else None
    return min(float(p.abs().min()) for p in vals), last


def last_u_pre(spec, params, x):
    """u_{L-1} before its ReLU, float64 [B, width]"""
    L = len(spec.szs)
    theta = _theta(params, False)
    prev = torch.as_tensor(np.asarray(x, np.float64))
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                u = _bn(u, theta, i)
        prev = u
    return prev.numpy()


def flag_matters(last):
    """a quarter of the last u-layer's pre-activations negative and a quarter positive"""
    return (last < 0).mean() >= 0.25 and (last > 0).mean() >= 0.25


def surrogate_grad64(spec, params, x_rows, y, v, c):
    """(grad dict, F_r) float64: x_rows [R][features] the gathered samples, y / v [R][n] and c [R] rounded to float32 like a
    feed; v None: F = c E."""
    theta = _theta(params)
    x = torch.as_tensor(np.asarray(x_rows, np.float64))
    yt = torch.tensor(np.asarray(y, np.float64).astype(np.float32).astype(np.float64), requires_grad=True)
    ct = torch.as_tensor(np.asarray(c, np.float64).astype(np.float32).astype(np.float64))
    E = energy(spec, theta, x, yt)[0]
    F = ct * E
    if v is not None:
        vt = torch.as_tensor(np.asarray(v, np.float64).astype(np.float32).astype(np.float64))
        dEdy, = torch.autograd.grad(E.sum(), yt, create_graph=True)
        F = F + (dEdy * vt).sum(dim=1)
    gs = torch.autograd.grad(F.sum(), list(theta.values()), allow_unused=True)
    grads = {k: (g.detach().numpy() if g is not None else np.zeros(np.shape(params[k]))) for k, g in zip(theta, gs)}
    return grads, F.detach().numpy()


def perturbed_params(spec, seed, rng):
    params = picnn.init_params(spec, seed, "spread")
    for k in params:                         # non-trivial BatchNorm parameters and biases (tests/test_train_grad.py)
        if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    return params


def small_problem(spec, seed, with_v):
    """Seeded model and feed (6 samples with 1-4 rows each), screened: no float64 pre-activation of the u-path, the gates or
    the z-path within MARGIN of zero, and the last u-layer's pre-activations over the batch a quarter negative and a quarter
    positive at least."""
    for s in range(seed, seed + 2000):
        rng = np.random.RandomState(s)
        params = perturbed_params(spec, s, rng)
        B = 6
        counts = rng.randint(1, 5, size=B)
        x = rng.rand(B, spec.n_features).astype(np.float32)
        samp = np.repeat(np.arange(B), counts)
        R = len(samp)
        y = rng.rand(R, spec.n_labels)
        v = rng.randn(R, spec.n_labels) if with_v else None
        c = rng.randn(R)
        y32 = y.astype(np.float32).astype(np.float64)
        m_rows, last = margins(spec, params, x[samp], y32)
        m_batch, _ = margins(spec, params, x, y32[np.cumsum(counts) - 1])
        if min(m_rows, m_batch) < MARGIN or not flag_matters(last_u_pre(spec, params, x)) or not flag_matters(last):
            continue
        g64, F64 = surrogate_grad64(spec, params, x[samp], y, v, c)
        return dict(seed=s, params=params, x=x, samp=samp, counts=counts, y=y, v=v, c=c, g64=g64, F64=F64)
    raise AssertionError("no screened seed")


def batch_problem(spec, seed, B, margin=MARGIN):
    """Seeded model and minibatch x [B], screened on the x-only pre-activations (u-path, gates) and the flag conditions"""
    for s in range(seed, seed + 2000):
        rng = np.random.RandomState(s)
        params = perturbed_params(spec, s, rng)
        x = rng.rand(B, spec.n_features).astype(np.float32)
        with torch.no_grad():
            _, _, gates, u_pre = energy(spec, _theta(params, False), torch.as_tensor(x.astype(np.float64)),
                                        torch.full((B, spec.n_labels), 0.5, dtype=torch.float64))
        m = min(float(p.abs().min()) for p in gates + u_pre if p is not None)
        if m < margin or not flag_matters(u_pre[-1].numpy()):
            continue
        return s, params, x
    raise AssertionError("no screened seed")


def unrolled_autograd(spec, params, x, y0, target, K, lr, mu, mask_traj=None):
    """Float64 autograd through K steps of momentum GD (g_k = dE/dy by autograd, create_graph) and the loss mean((y_K -
    t)^2).  mask_traj [B, K, n] (the device trajectory): the z-path masks of step k are those of E at mask_traj[:, k], so the
    recurrence differentiated is the one the device ran.  Returns (grads, y_K, trajectory, min |z pre-activation| at the
    masking points)."""
    theta = _theta(params)
    xt = torch.as_tensor(np.asarray(x, np.float64))
    y = torch.tensor(np.asarray(y0, np.float64), requires_grad=True)
    t = torch.as_tensor(np.asarray(target, np.float64))
    v, traj, margin = 0, [], np.inf
    for k in range(K):
        traj.append(y.detach().clone())
        at = None if mask_traj is None else torch.as_tensor(np.asarray(mask_traj[:, k], np.float64))
        E, pre, _, _ = energy(spec, theta, xt, y, mask_at=at)
        if at is None:
            margin = min([margin] + [float(p.detach().abs().min()) for p in pre])
        else:
            with torch.no_grad():
                margin = min([margin] + [float(p.abs().min()) for p in energy(spec, theta, xt, at)[1]])
        g, = torch.autograd.grad(E.sum(), y, create_graph=True)
        prev = v
        v = mu * prev - lr * g
        y = y - mu * prev + (1.0 + mu) * v
    loss = torch.mean(torch.square(y - t))
    names = list(theta)
    gs = torch.autograd.grad(loss, [theta[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(np.shape(params[k])) if g is None else g.detach().numpy()) for k, g in zip(names, gs)}
    return grads, y.detach().numpy(), torch.stack(traj, 1).numpy(), margin


def f_picnn_literal(params, x, y, sizes=(200, 200, 1)):
    """The synthetic script's f_picnn read literally, float64: for every size, a ReLU'd u-layer from prevU unless the size is
    1; the z terms from prevU (gate and proj from the second layer on), summed, ReLU'd unless the size is 1; then prevU = u,
    prevZ = z.  Returns E [B] as a tensor connected to y."""
    th = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    prevZ, prevU, u = None, x, None
    for layer, sz in enumerate(sizes):
        if sz != 1:
            u = torch.relu(prevU @ th["u%d/W" % layer] + th["u%d/b" % layer])
        terms = []
        if prevZ is not None:
            gate = torch.relu(prevU @ th["z%d_zu_u/W" % layer] + th["z%d_zu_u/b" % layer])
            terms.append((prevZ * gate) @ th["z%d_zu_proj/W" % layer])
        yu = prevU @ th["z%d_yu_u/W" % layer] + th["z%d_yu_u/b" % layer]
        terms.append((y * yu) @ th["z%d_yu/W" % layer])
        terms.append(prevU @ th["z%d_u/W" % layer] + th["z%d_u/b" % layer])
        z = sum(terms)
        if sz != 1:
            z = torch.relu(z)
        prevU, prevZ = u, z
    return z.reshape(z.shape[0], -1)[:, 0]


def context_y_path64(spec, params, ctx, y):
    """E [B] float64 from a context row (float64 tensor [B, C], picnn's layout) and the y-path weights: what fg evaluates"""
    th = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    L = len(spec.szs)
    z = None
    for i, (yu, zu, gate) in enumerate(spec.ctx_offsets):
        w = spec.widths[i]
        add = (y * ctx[:, yu:yu + spec.n_labels]) @ th["z%d_yu/W" % i] + ctx[:, zu:zu + w]
        if i > 0:
            add = add + (z * ctx[:, gate:gate + spec.widths[i - 1]]) @ th["z%d_zu_proj/W" % i]
        z = torch.where(add > 0, add, spec.alpha * add) if i < L else add
    return z.reshape(-1)


def context64(spec, params, x):
    """the context row in float64 (no BatchNorm), picnn's layout, the flag honoured"""
    assert not spec.batchnorm
    th = _theta(params, False)
    us, _ = u_path(spec, th, x)
    parts = []
    for i in range(len(spec.szs) + 1):
        prev = x if i == 0 else us[i - 1]
        parts.append(prev @ th["z%d_yu_u/W" % i] + th["z%d_yu_u/b" % i])
        parts.append(prev @ th["z%d_u/W" % i] + th["z%d_u/b" % i])
        if i > 0:
            parts.append(torch.relu(prev @ th["z%d_zu_u/W" % i] + th["z%d_zu_u/b" % i]))
    return torch.cat(parts, dim=1)


def context_by_hand(spec, params, x, relu_last):
    """The context row as a float32 torch chain written out by hand (addmm, relu, addmm ...), batch-statistics BatchNorm on
    the hidden u-layers when the spec has it; relu_last: ReLU the last u-layer."""
    t = {k: torch.as_tensor(np.asarray(v, np.float32)) for k, v in params.items()}
    L = len(spec.szs)
    x = x.to(torch.float32)
    us, prev = [], x
    for i in range(L):
        u = torch.addmm(t["u%d/b" % i], prev, t["u%d/W" % i])
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                mean = u.mean(dim=0)
                var = ((u - mean) ** 2).mean(dim=0)
                u = (u - mean) / torch.sqrt(var + 1e-5) * t["u%d/bn/gamma" % i] + t["u%d/bn/beta" % i]
        elif relu_last:
            u = torch.relu(u)
        us.append(u)
        prev = u
    cols = []
    for i in range(L + 1):
        prev = x if i == 0 else us[i - 1]
        cols.append(torch.addmm(t["z%d_yu_u/b" % i], prev, t["z%d_yu_u/W" % i]))
        cols.append(torch.addmm(t["z%d_u/b" % i], prev, t["z%d_u/W" % i]))
        if i > 0:
            cols.append(torch.relu(torch.addmm(t["z%d_zu_u/b" % i], prev, t["z%d_zu_u/W" % i])))
    return torch.cat(cols, dim=1).contiguous()


def moons(B, seed):
    """two interleaved half circles with noise (the data of tests/test_ficnn_train.py::test_loss_decreases_on_moons)"""
    rng = np.random.RandomState(seed)
    h = B // 2
    a = np.linspace(0, np.pi, h)
    b = np.linspace(0, np.pi, B - h)
    X = np.r_[np.c_[np.cos(a), np.sin(a)], np.c_[1 - np.cos(b), 1 - np.sin(b) - 0.5]] + 0.1 * rng.randn(B, 2)
    Y = np.r_[np.zeros(h), np.ones(B - h)].reshape(B, 1)
    return X.astype(np.float32), Y.astype(np.float32)
