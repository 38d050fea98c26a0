"""Float64 statement of the completion model's training surrogate (completion/icnn_ebundle.py:129-140, network :337-452) on
the gathered feed rows, for tests/test_train_grad_conv.py: BatchNorm over the rows (x_ = fd_xs), 'SAME' padding as
picnn.conv_context, F = c E + <dE/dy, v> differentiated with create_graph=True.  Shares no code with the kernels."""
import numpy as np
import torch
import torch.nn.functional as Fn

CONVS = [(32, 8, 4), (64, 4, 2), (64, 3, 1)]
PAD = {8: 2, 4: 1, 3: 1}


def _conv(inp, W, b, stride):
    out = Fn.conv2d(inp.permute(0, 3, 1, 2).contiguous(), W.permute(3, 2, 0, 1).contiguous(), b, stride=stride,
                    padding=PAD[W.shape[0]])
    return out.permute(0, 2, 3, 1)


def _bn(v, g, b, dims):
    mean = v.mean(dim=dims, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=dims, keepdim=True)
    return (v - mean) / torch.sqrt(var + 1e-5) * g + b


def _forward(t, x, y):
    """E [R] and the pre-activations whose sign sets a mask: z-path (y-dependent) and u-path / gates (x only)."""
    zpre, upre = [], []
    us, prev = [], x
    for l, (nf, k, s) in enumerate(CONVS):
        h = _conv(prev, t["u%d/W" % l], t["u%d/b" % l], s)
        upre.append(h)
        u = _bn(torch.relu(h), t["u%d/bn/gamma" % l], t["u%d/bn/beta" % l], (0, 1, 2))
        us.append(u)
        prev = u
    flat = prev.reshape(prev.shape[0], -1)
    h3 = flat @ t["u3/W"] + t["u3/b"]
    upre.append(h3)
    u3 = _bn(torch.relu(h3), t["u3/bn/gamma"], t["u3/bn/beta"], (0,))
    prevU, prevZ, y_red = x, None, y
    for l, (nf, k, s) in enumerate(CONVS):
        acc = _conv(prevU, t["z%d_u/W" % l], t["z%d_u/b" % l], s)
        if l > 0:
            gh = _conv(prevU, t["z%d_zu_u/W" % l], t["z%d_zu_u/b" % l], 1)
            upre.append(gh)
            acc = acc + _conv(prevZ * torch.relu(gh), t["z%d_zu_proj/W" % l], None, s)
        yu = _conv(prevU, t["z%d_yu_u/W" % l], t["z%d_yu_u/b" % l], 1)
        acc = acc + _conv(y_red * yu, t["z%d_yu/W" % l], None, s)
        y_red = _conv(y_red, t["z%d_y_red/W" % l], t["z%d_y_red/b" % l], s)
        zpre.append(acc)
        prevZ = torch.relu(acc)
        prevU = us[l]
    prevZ = prevZ.reshape(prevZ.shape[0], -1)
    prevU = prevU.reshape(prevU.shape[0], -1)
    for l in (3, 4):
        gh = prevU @ t["z%d_zu_u/W" % l] + t["z%d_zu_u/b" % l]
        upre.append(gh)
        z = (prevZ * torch.relu(gh)) @ t["z%d_zu_proj/W" % l] + prevU @ t["z%d_u/W" % l] + t["z%d_u/b" % l]
        if l == 3:
            zpre.append(z)
            z = torch.relu(z)
        prevZ, prevU = z, u3
    return prevZ.reshape(-1), zpre, upre


def surrogate_grad64(spec, params, x_rows, y, v, c):
    """(grads {name: float64 ndarray}, F [R], margin): F = c E + <dE/dy, v> per row and d(sum F)/dtheta for every variable
    (zeros where F does not depend on it); margin = min |z-path pre-activation| (the masks the kernels' float32 must
    reproduce)."""
    t = {k: torch.tensor(np.asarray(p, np.float64), requires_grad=True) for k, p in params.items()}
    R = y.shape[0]
    x = torch.as_tensor(np.asarray(x_rows, np.float64)).reshape(R, spec.H, spec.W, 1)
    y32 = np.asarray(y, np.float64).astype(np.float32).astype(np.float64)     # the feed is float32
    yt = torch.tensor(y32.reshape(R, spec.H, spec.W, 1), requires_grad=True)
    E, zpre, _ = _forward(t, x, yt)
    ct = torch.as_tensor(np.asarray(c, np.float64))
    F = ct * E
    if v is not None:
        g, = torch.autograd.grad(E.sum(), yt, create_graph=True)
        F = F + (g.reshape(R, -1) * torch.as_tensor(np.asarray(v, np.float64).reshape(R, -1))).sum(1)
    names = list(t.keys())
    grads = torch.autograd.grad(F.sum(), [t[k] for k in names], allow_unused=True)
    out = {k: (np.zeros(params[k].shape) if gk is None else gk.detach().numpy()) for k, gk in zip(names, grads)}
    margin = min(float(z.detach().abs().min()) for z in zpre)
    return out, F.detach().numpy(), margin


def u_margin(spec, params, x_rows):
    """min |pre-ReLU| of the u-path and the gates over the rows (x only)."""
    t = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    R = x_rows.shape[0]
    x = torch.as_tensor(np.asarray(x_rows, np.float64)).reshape(R, spec.H, spec.W, 1)
    y = torch.zeros(R, spec.H, spec.W, 1, dtype=torch.float64)
    _, _, upre = _forward(t, x, y)
    return min(float(h.abs().min()) for h in upre)


def energy_and_grad64(spec, params, x_rows, y):
    """E [R] and dE/dy [R, H*W] (float64) with BatchNorm over the rows: the check against the oracle."""
    t = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    R = y.shape[0]
    x = torch.as_tensor(np.asarray(x_rows, np.float64)).reshape(R, spec.H, spec.W, 1)
    yt = torch.tensor(np.asarray(y, np.float64).reshape(R, spec.H, spec.W, 1), requires_grad=True)
    E, _, _ = _forward(t, x, yt)
    g, = torch.autograd.grad(E.sum(), yt)
    return E.detach().numpy(), g.reshape(R, -1).numpy()
