"""NumPy restatement of icnn_be_gd_feed_px (include/icnn_be.h): the feed of the completion model's
back-optimisation step with the loss mean((px (y_K - t))^2).  Every float32 operation is one NumPy float32 operation (rounded,
never fused), in the header's order."""
import math

import numpy as np


def ybar32(yK, t, scale, px):
    """(u, ybar), float32 [B, n]: d = (float)yK - t, u = px d, ybar = ((u 2) scale) px"""
    px, scale = np.float32(px), np.float32(scale)
    d = np.asarray(yK, np.float64).astype(np.float32) - np.asarray(t, np.float32)
    u = px * d
    ybar = ((u * np.float32(2.0)) * scale) * px
    assert u.dtype == np.float32 and ybar.dtype == np.float32
    return u, ybar


def feed(yK, t, coef, scale, px):
    """v_rows [B K, n] (float64), c_rows [B K], row_offset [B + 1] (int32) and the float64 loss mean(u^2) by math.fsum (every
    square exact in float64)"""
    B, n = np.shape(yK)
    coef = np.asarray(coef, np.float64).reshape(-1)
    K = coef.shape[0]
    u, ybar = ybar32(yK, t, scale, px)
    v = (coef[None, :, None] * ybar.astype(np.float64)[:, None, :]).reshape(B * K, n)
    c = np.zeros(B * K, np.float64)
    off = np.arange(0, (B + 1) * K, K, dtype=np.int32)
    return v, c, off, loss64(u)


def loss64(u):
    u = np.asarray(u, np.float32).astype(np.float64).reshape(-1)
    return math.fsum(u * u) / u.size
