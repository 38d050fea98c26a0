"""Statements of the back-optimisation inference for tests/test_gd*.py (shares no code with the kernels): the float32 NumPy
recurrence of multi-label-cls/icnn-back.py:120-133 around an energy/gradient oracle, and the float64 autograd unroll of the
reference graph next to the one-pass surrogate form that train.unrolled_grad evaluates."""
import numpy as np
import torch


def unroll_f32(fg, y0, K, lr, mu):
    """(y_K float32 [B, n], trajectory float64 [B, K, n], E(y_K) float32 [B]) of the float32 recurrence; fg(y float64) ->
    (E, dE/dy) float32.  The constants are float32(lr), float32(mu), float32(1.0 + mu) -- the sum formed in double."""
    f32 = np.float32
    lr32, mu32, c1 = f32(lr), f32(mu), f32(1.0 + mu)
    y = np.asarray(y0, np.float64).astype(f32)
    v = np.zeros_like(y)
    traj = []
    for _ in range(K):
        traj.append(y.astype(np.float64))
        _, g = fg(y.astype(np.float64))
        g = np.asarray(g, f32)
        mv = mu32 * v
        vn = mv - lr32 * g
        y = (y - mv) + c1 * vn
        v = vn
    E, _ = fg(y.astype(np.float64))
    return y, np.stack(traj, 1), np.asarray(E, f32)


def unrolled_autograd(energy, params, x, y0, target, K, lr, mu, scale=1.0):
    """Side one: the reference graph in float64 -- K steps of momentum GD with g_k = dE/dy by autograd (create_graph), loss
    mean((scale (y_K - target))^2), its gradient over every variable by autograd through the whole unroll.
    energy(theta, x, y) -> (E [B], list of pre-activation tensors).  Returns (grads {name: ndarray}, y_K, trajectory
    [B, K, ...], ybar = dL/dy_K, min |pre-activation| over every step)."""
    theta = {k: torch.tensor(np.asarray(p, np.float64), requires_grad=True) for k, p in params.items()}
    x = torch.as_tensor(np.asarray(x, np.float64))
    y = torch.tensor(np.asarray(y0, np.float64), requires_grad=True)
    t = torch.as_tensor(np.asarray(target, np.float64))
    v = 0
    traj, margin = [], np.inf
    for _ in range(K):
        traj.append(y.detach().clone())
        E, pre = energy(theta, x, y)
        margin = min([margin] + [float(p.detach().abs().min()) for p in pre])
        g, = torch.autograd.grad(E.sum(), y, create_graph=True)
        prev = v
        v = mu * prev - lr * g
        y = y - mu * prev + (1.0 + mu) * v
    yK = y
    loss = torch.mean(torch.square(scale * (yK - t)))
    ybar, = torch.autograd.grad(loss, yK, retain_graph=True)
    names = list(theta)
    gs = torch.autograd.grad(loss, [theta[k] for k in names], allow_unused=True)
    grads = {k: (np.zeros(params[k].shape) if g is None else g.detach().numpy()) for k, g in zip(names, gs)}
    return grads, yK.detach().numpy(), torch.stack(traj, 1).numpy(), ybar.detach().numpy(), margin


def surrogate_form(energy, params, x, traj, ybar, coef):
    """Side two: grad_theta sum_{j,k} <dE/dy(x_j, y_{j,k}), coef_k ybar_j> on the B K rows (x repeated K times, sample-major,
    BatchNorm over the repeated rows), float64 autograd.  traj [B, K, ...] detached, ybar [B, ...]."""
    theta = {k: torch.tensor(np.asarray(p, np.float64), requires_grad=True) for k, p in params.items()}
    B, K = traj.shape[:2]
    X = torch.as_tensor(np.repeat(np.asarray(x, np.float64), K, axis=0))
    Y = torch.tensor(np.asarray(traj, np.float64).reshape((B * K,) + traj.shape[2:]), requires_grad=True)
    V = torch.as_tensor((np.asarray(coef)[None, :, None] * np.asarray(ybar).reshape(B, 1, -1)).reshape(Y.shape))
    E, _ = energy(theta, X, Y)
    g, = torch.autograd.grad(E.sum(), Y, create_graph=True)
    F = (g * V).sum()
    names = list(theta)
    gs = torch.autograd.grad(F, [theta[k] for k in names], allow_unused=True)
    return {k: (np.zeros(params[k].shape) if g is None else g.detach().numpy()) for k, g in zip(names, gs)}
