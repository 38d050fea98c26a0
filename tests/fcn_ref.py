"""The FCN baseline of the completion experiment restated in float64, written from the layer table on
torch.nn.functional.conv2d / conv_transpose2d -- the arithmetic is the library's, the parameters are the table's -- with
worst-case float32 error bounds in §22 / §24's form and torch.optim.Adam's update.

    conv1..3  conv2d, 3x3, stride 2, dilation 2, padding 2        up1..3  conv_transpose2d, 3x3, stride 2, padding 1, output_padding 1
    up4       conv_transpose2d, 1x1                               ReLU behind every layer but up4
    loss = mean((scale (yhat - t))^2)

Bounds, u = 2^-24.  A layer's pre-activation from an input with error e:
    e_z = op(e, |W|) + (K + 1) u (op(|h| + e, |W|) + |b|),  K the terms per output: 9 Cin (conv), 4 Cin (transposed), Cin (up4)
ReLU does not grow an error; a unit with |z| < e_z is AMBIGUOUS: the two sides may disagree about its mask, and its delta's
bound is then the whole |dh| + e_dh.  A product X^T Delta over T terms gets (T + 1) u sum |x| |delta| on top of the
propagated errors.  Everything is NCHW here; the device keeps channels last."""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
LAYERS = ("conv1", "conv2", "conv3", "up1", "up2", "up3", "up4")
CONV = dict(stride=2, dilation=2, padding=2)
UP = dict(stride=2, padding=1, output_padding=1)


def op(name, h, W):
    """the layer's own product, without the bias"""
    if name.startswith("conv"):
        return F.conv2d(h, W, **CONV)
    if name == "up4":
        return F.conv_transpose2d(h, W)
    return F.conv_transpose2d(h, W, **UP)


def terms(name, cin):
    """products added per output element, at most"""
    return 9 * cin if name.startswith("conv") else cin if name == "up4" else 4 * cin


def terms_T(name, cout):
    """products added per element of the data gradient, at most"""
    return cout if name == "up4" else 9 * cout


def op_T(name, d, W, h_like):
    """the adjoint in h: d (sum op(h, W) d) / dh; op is linear in h, so any h serves"""
    h = torch.zeros_like(h_like, requires_grad=True)
    (op(name, h, W) * d).sum().backward()
    return h.grad


def op_W(name, h, d, W_like):
    """X^T Delta: d (sum op(h, W) d) / dW"""
    W = torch.zeros_like(W_like, requires_grad=True)
    (op(name, h, W) * d).sum().backward()
    return W.grad


def contraction(name, h, d):
    """T of the weight gradient: the positions its sum runs over -- the outputs of a conv, the inputs of a transposed conv"""
    return (d if name.startswith("conv") else h)[:, 0].numel()


def t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def params64(params):
    return {n: t64(a) for n, a in params.items()}


def flat(named):
    out = []
    for name in LAYERS:
        out += [np.asarray(named[name + ".weight"]).reshape(-1), np.asarray(named[name + ".bias"]).reshape(-1)]
    return np.concatenate(out)


def reference(params, x, t=None, scale=255.0, masks=None):
    """One forward (and with t the loss and the whole gradient) in float64 with end-to-end bounds.  x, t: [B, H, W].
    masks: six boolean arrays [B, k, h, w] to use instead of z > 0 (the device's), in which case no unit is ambiguous.
    Returns a dict of NumPy arrays: z[i], h[i], e_h[i] (i < 6), yhat, e_yhat, and with t: loss, e_loss, dy, e_dy, dz[i], e_dz[i],
    grad, e_grad (flat), ambiguous[i]."""
    P = params64(params)
    x = t64(x)
    B, H, W_ = x.shape
    x = x.reshape(B, 1, H, W_)
    h, e = x, torch.zeros_like(x)
    hs, es, zs, ezs, ms = [x], [e], [], [], []
    for i, name in enumerate(LAYERS):
        W, b = P[name + ".weight"], P[name + ".bias"].view(1, -1, 1, 1)
        K = terms(name, h.shape[1])
        z = op(name, h, W) + b
        e = op(name, e, W.abs()) + (K + 1) * U * (op(name, h.abs() + e, W.abs()) + b.abs())
        if name == "up4":
            yhat, e_y = z, e
            break
        m = (z > 0) if masks is None else torch.as_tensor(masks[i])
        h = z * m
        zs.append(z), ezs.append(e), ms.append(m), hs.append(h), es.append(e)
    out = {"z": [a.numpy() for a in zs], "e_z": [a.numpy() for a in ezs], "h": [a.numpy() for a in hs[1:]],
           "e_h": [a.numpy() for a in es[1:]], "yhat": yhat.numpy()[:, 0], "e_yhat": e_y.numpy()[:, 0]}
    if t is None:
        return out
    t = t64(t).reshape(B, 1, H, W_)
    N = B * H * W_
    diff = yhat - t
    loss = ((scale * diff) ** 2).mean()
    e_loss = (scale * scale * (2 * diff.abs() * e_y + e_y * e_y)).mean() + 7 * U * loss
    d = 2 * scale * scale * diff / N
    e_d = 2 * scale * scale * e_y / N + 5 * U * d.abs()
    out.update(loss=float(loss), e_loss=float(e_loss), dy=d.numpy()[:, 0], e_dy=e_d.numpy()[:, 0])
    grad, e_grad, dz, e_dz, amb = {}, {}, [None] * 6, [None] * 6, [None] * 6
    for i in range(6, -1, -1):
        name = LAYERS[i]
        W, hin, ein = P[name + ".weight"], hs[i], es[i]
        T, Tb = contraction(name, hin, d), d[:, 0].numel()
        grad[name + ".weight"] = op_W(name, hin, d, W).numpy()
        e_grad[name + ".weight"] = (op_W(name, hin.abs() + ein, e_d, W) + op_W(name, ein, d.abs(), W)
                                    + (T + 1) * U * op_W(name, hin.abs() + ein, d.abs() + e_d, W)).numpy()
        grad[name + ".bias"] = d.sum((0, 2, 3)).numpy()
        e_grad[name + ".bias"] = (e_d.sum((0, 2, 3)) + (Tb + 1) * U * (d.abs() + e_d).sum((0, 2, 3))).numpy()
        if i == 0:
            break
        Kt = terms_T(name, d.shape[1])
        dh = op_T(name, d, W, hin)
        e_dh = op_T(name, e_d, W.abs(), hin) + (Kt + 1) * U * op_T(name, d.abs() + e_d, W.abs(), hin)
        a = (zs[i - 1].abs() < ezs[i - 1]) if masks is None else torch.zeros_like(ms[i - 1], dtype=torch.bool)
        d = dh * ms[i - 1]
        e_d = torch.where(a, dh.abs() + e_dh, e_dh)
        dz[i - 1], e_dz[i - 1], amb[i - 1] = d.numpy(), e_d.numpy(), a.numpy()
    out.update(dz=dz, e_dz=e_dz, ambiguous=amb, grad=flat(grad), e_grad=flat(e_grad))
    return out


def grad_x(params, x, t, scale=255.0):
    """d loss / d x in float64 by torch.autograd, [B, H, W]"""
    P = params64(params)
    x = t64(x).unsqueeze(1).requires_grad_(True)
    h = x
    for name in LAYERS:
        h = op(name, h, P[name + ".weight"]) + P[name + ".bias"].view(1, -1, 1, 1)
        if name != "up4":
            h = F.relu(h)
    ((scale * (h - t64(t).unsqueeze(1))) ** 2).mean().backward()
    return x.grad.numpy()[:, 0]


def autograd_grad(params, x, t, scale=255.0):
    """the flat gradient in float64 by torch.autograd"""
    P = {n: a.requires_grad_(True) for n, a in params64(params).items()}
    h = t64(x).unsqueeze(1)
    for name in LAYERS:
        h = op(name, h, P[name + ".weight"]) + P[name + ".bias"].view(1, -1, 1, 1)
        if name != "up4":
            h = F.relu(h)
    ((scale * (h - t64(t).unsqueeze(1))) ** 2).mean().backward()
    return flat({n: a.grad.numpy() for n, a in P.items()})


def adam64(theta, m, v, g, t, lr=1e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's step number t (1-based) in float64: eps OUTSIDE the bias correction.  Returns (theta, m, v)."""
    theta, m, v, g = (np.asarray(a, np.float64) for a in (theta, m, v, g))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    theta = theta - (lr / (1 - beta1 ** t)) * m / (np.sqrt(v) / np.sqrt(1 - beta2 ** t) + eps)
    return theta, m, v


def adam_tol(theta_before, theta_after):
    """per step: 2 u |theta| + 16 u |delta theta|"""
    return 2 * U * np.abs(theta_after) + 16 * U * np.abs(np.asarray(theta_after, np.float64) - np.asarray(theta_before, np.float64))


def draw(k, B, H, W, seed):
    """(params, x, t): torch's init bounds with NumPy's stream (icnn_amd.fcn.init_params), uniform images and targets"""
    from icnn_amd import fcn
    params = fcn.init_params(fcn.FCNSpec(H, W, k), seed)
    rng = np.random.RandomState(seed + 1000)
    return params, rng.uniform(0, 1, (B, H, W)).astype(np.float32), rng.uniform(0, 1, (B, H, W)).astype(np.float32)


def nchw(a):
    """a device piece [B, h, w, k] as float64 [B, k, h, w]"""
    return np.ascontiguousarray(np.transpose(np.asarray(a, np.float64), (0, 3, 1, 2)))
