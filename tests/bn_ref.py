"""Float64 torch statement of the x-only context with tflearn's BatchNorm in either mode, and the float32 fold of the
moving statistics (test helper; shares no code with the kernels).

Training mode normalises with the batch mean and the biased batch variance (tf.nn.moments) and returns them; inference
mode normalises with the moving statistics.  fold32 is assign_moving_average without zero-debias (TF r0.10) in float32:
m <- m - (m - mu) d, v <- v - (v - sigma^2) d, d = float32(1 - decay), rounded after every operation."""
import numpy as np
import torch
import torch.nn.functional as F

from icnn_amd.picnn import CONV_FCS, CONV_LAYERS

EPS = 1e-5


def _bn(u, theta, i, dims, bn_stats, stats_out):
    g, b = theta["u%d/bn/gamma" % i], theta["u%d/bn/beta" % i]
    if bn_stats is not None:
        m = torch.as_tensor(np.asarray(bn_stats["u%d/bn/moving_mean" % i], np.float64))
        v = torch.as_tensor(np.asarray(bn_stats["u%d/bn/moving_variance" % i], np.float64))
    else:
        m = u.mean(dim=dims)
        v = ((u - m) ** 2).mean(dim=dims)
        stats_out[i] = (m.numpy().copy(), v.numpy().copy())
    return (u - m) / torch.sqrt(v + EPS) * g + b


def fc_context64(spec, params, x, bn_stats=None):
    """(ctx [B, ctx_width] float64, {layer: (batch mean, batch variance)}) of the FC PICNN; bn_stats: inference mode."""
    theta = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    x = torch.as_tensor(np.asarray(x, np.float64))
    L, stats, us, prev = len(spec.szs), {}, [], x
    for i in range(L):
        u = prev @ theta["u%d/W" % i] + theta["u%d/b" % i]
        if i < L - 1:
            u = torch.relu(u)
            if spec.batchnorm:
                u = _bn(u, theta, i, 0, bn_stats, stats)
        us.append(u)
        prev = u
    parts = []
    for i in range(L + 1):
        prev = x if i == 0 else us[i - 1]
        parts.append(prev @ theta["z%d_yu_u/W" % i] + theta["z%d_yu_u/b" % i])
        parts.append(prev @ theta["z%d_u/W" % i] + theta["z%d_u/b" % i])
        if i > 0:
            parts.append(torch.relu(prev @ theta["z%d_zu_u/W" % i] + theta["z%d_zu_u/b" % i]))
    return torch.cat(parts, dim=1).numpy(), stats


def conv_heads(spec):
    """(name, width) of the heads of a conv context row, in row order"""
    m, n = spec.maps, spec.n_labels
    return [("yu0", n), ("zu0", m[0][0] * m[0][1] * m[0][2]), ("gate1", m[0][0] * m[0][1] * m[0][2]),
            ("yu1", m[0][0] * m[0][1]), ("zu1", m[1][0] * m[1][1] * m[1][2]), ("gate2", m[1][0] * m[1][1] * m[1][2]),
            ("yu2", m[1][0] * m[1][1]), ("zu2", m[2][0] * m[2][1] * m[2][2]), ("gate3", spec.flat_dim),
            ("zu3", CONV_FCS[0]), ("gate4", CONV_FCS[0]), ("zu4", 1)]


def conv_context64(spec, params, x, bn_stats=None):
    """The same for the conv PICNN of the completion experiment, x [B, H, W, 1] (already h-flipped); the statistics of
    u0..u2 are over samples x positions, per channel."""
    theta = {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    pad_of = {8: 2, 4: 1, 3: 1}

    def conv(inp, W, b, stride):
        out = F.conv2d(inp.permute(0, 3, 1, 2), W.permute(3, 2, 0, 1), b, stride=stride, padding=pad_of[W.shape[0]])
        return out.permute(0, 2, 3, 1)

    x = torch.as_tensor(np.asarray(x, np.float64))
    B, stats, us, prev = x.shape[0], {}, [], x
    for l, (nf, k, s) in enumerate(CONV_LAYERS):
        u = _bn(torch.relu(conv(prev, theta["u%d/W" % l], theta["u%d/b" % l], s)), theta, l, (0, 1, 2), bn_stats, stats)
        us.append(u)
        prev = u
    u3 = _bn(torch.relu(prev.reshape(B, -1) @ theta["u3/W"] + theta["u3/b"]), theta, 3, 0, bn_stats, stats)
    parts, prevU = [], x
    for l, (nf, k, s) in enumerate(CONV_LAYERS):
        if l > 0:
            parts.append(torch.relu(conv(prevU, theta["z%d_zu_u/W" % l], theta["z%d_zu_u/b" % l], 1)).reshape(B, -1))
        parts.append(conv(prevU, theta["z%d_yu_u/W" % l], theta["z%d_yu_u/b" % l], 1).reshape(B, -1))
        parts.append(conv(prevU, theta["z%d_u/W" % l], theta["z%d_u/b" % l], s).reshape(B, -1))
        prevU = us[l]
    prevU = prevU.reshape(B, -1)
    for l in (3, 4):
        parts.append(torch.relu(prevU @ theta["z%d_zu_u/W" % l] + theta["z%d_zu_u/b" % l]))
        parts.append(prevU @ theta["z%d_u/W" % l] + theta["z%d_u/b" % l])
        prevU = u3
    ctx = torch.cat(parts, dim=1).numpy()
    assert ctx.shape[1] == spec.ctx_width
    return ctx, stats


def fold32(bn_stats, batch_stats, k, decay=0.9):
    """bn_stats after k folds of batch_stats ({layer: (mean, variance)}, any float dtype: rounded to float32 first)"""
    d = np.float32(1.0 - decay)
    out = {key: np.asarray(v, np.float32).copy() for key, v in bn_stats.items()}
    for i, (mu, var) in batch_stats.items():
        mu, var = np.asarray(mu, np.float32), np.asarray(var, np.float32)
        m, v = out["u%d/bn/moving_mean" % i], out["u%d/bn/moving_variance" % i]
        for _ in range(k):
            m = np.float32(m - np.float32((m - mu) * d))
            v = np.float32(v - np.float32((v - var) * d))
            m, v = m.astype(np.float32), v.astype(np.float32)
        out["u%d/bn/moving_mean" % i], out["u%d/bn/moving_variance" % i] = m, v
    return out


def random_bn_stats(stats, seed):
    """non-trivial moving statistics keyed like `stats` (picnn.init_bn_stats): means around 0.3, variances in [0.2, 1.7)"""
    rng = np.random.RandomState(seed)
    out = {}
    for k, v in stats.items():
        if k.endswith("moving_mean"):
            out[k] = (0.3 + 0.2 * rng.randn(*v.shape)).astype(np.float32)
        else:
            out[k] = (0.2 + 1.5 * rng.rand(*v.shape)).astype(np.float32)
    return out
