"""Back-optimisation inference of the conv PICNN of the completion experiment (completion/icnn.back.py:136-147): the reduction
of the unrolled gradient on a small image (float64, CPU), the C entry's argument checks, and on the device the trajectory
against the kernel-order oracle and the loop of ConvModel.fg bit for bit, and the gradient at the reference's batch."""
import ctypes as C

import numpy as np
import pytest
import torch

import gd_ref
import train_conv_ref
from icnn_amd import picnn

LR, MU = 0.01, 0.9                       # completion defaults (icnn.back.py)
SPEC = picnn.ConvSpec()


def _conv_energy(spec):
    def energy(theta, x, y):
        R = y.shape[0]
        E, zpre, _ = train_conv_ref._forward(theta, x.reshape(R, spec.H, spec.W, 1), y.reshape(R, spec.H, spec.W, 1))
        return E, zpre
    return energy


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("K", [3, 5])
def test_conv_unrolled_gradient_is_one_surrogate_over_the_trajectory(K):
    from icnn_amd import gd
    spec = picnn.ConvSpec(16, 16)
    rng = np.random.RandomState(K)
    params = picnn.init_conv_params(spec, K, "spread")
    for k in params:
        if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    B = 3
    x = rng.rand(B, spec.n_labels).astype(np.float32)
    y0 = np.repeat((0.2 + 0.6 * rng.rand(spec.n_labels))[None], B, axis=0)
    t = rng.rand(B, spec.n_labels)
    lr, mu = 0.05, 0.9
    g1, yK, traj, ybar, _ = gd_ref.unrolled_autograd(_conv_energy(spec), params, x, y0, t, K, lr, mu, scale=255.0)
    assert np.abs(yK - y0).max() > 1e-4
    g2 = gd_ref.surrogate_form(_conv_energy(spec), params, x, traj, ybar, gd.coefficients(K, lr, mu))
    nonzero = 0
    for k in params:
        scale = float(np.abs(g1[k]).max())
        assert float(np.abs(g2[k] - g1[k]).max()) <= 1e-10 * scale, (k, scale)
        nonzero += scale > 0
    assert nonzero > len(params) // 2


def _conv_struct():
    from icnn_amd import _lib
    m = _lib.ConvModel()
    m.H, m.W = SPEC.H, SPEC.W
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        m.filters[l], m.ksize[l], m.stride[l] = nf, k, s
    m.fc_hidden, m.ctx_width = picnn.CONV_FCS[0], SPEC.ctx_width
    m.wpack, m.work, m.work_batch = 64, 64, 8
    return m


def test_conv_entry_rejects_bad_arguments_before_launch():
    from icnn_amd import _lib
    lib = _lib.load()
    m = _conv_struct()
    fake = C.c_void_p(64)

    def call(mm=m, batch=4, K=3, lr=LR, mu=MU, ctx=fake, y0=fake, y=fake, ws=fake):
        return lib.icnn_be_conv_gd(None if mm is None else C.byref(mm), ctx, y0, batch, K, lr, mu, y, None, None, ws, None)
    assert call(K=0) == -1
    assert call(batch=-1) == -1
    assert call(lr=float("nan")) == -1
    assert call(mu=float("inf")) == -1
    assert call(mm=None) == -1
    assert call(ctx=None) == -1
    assert call(y0=None) == -1
    assert call(y=None) == -1
    assert call(ws=None) == -1
    assert call(batch=9) == -1                        # beyond the model's work_batch
    m2 = _conv_struct()
    m2.work = None
    assert call(mm=m2) == -1
    m3 = _conv_struct()
    m3.ctx_width += 1
    assert call(mm=m3) == -1
    m4 = _conv_struct()
    m4.wpack = None
    assert call(mm=m4) == -1
    assert call(batch=0) == 0


# ------------------------------------------------------------------------------------------------ GPU


def _conv_problem(B, seed):
    rng = np.random.RandomState(seed)
    params = picnn.init_conv_params(SPEC, seed, "spread")
    x = rng.rand(B, SPEC.H, SPEC.W, 1).astype(np.float32)
    y0 = np.repeat((0.2 + 0.6 * rng.rand(SPEC.n_labels))[None], B, axis=0)       # meanY-like start
    return params, x, y0, rng


@pytest.mark.gpu
def test_conv_trajectory_bit_exact_against_oracle():
    from icnn_amd import gd
    from oracle import picnn_conv_oracle
    B, K = 8, 10
    params, x, y0, _ = _conv_problem(B, 8)
    model = picnn.ConvModel(SPEC, params)
    ctx = model.context(torch.from_numpy(x).cuda())
    y, traj, E = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, LR, MU, trajectory=True, energy=True)
    torch.cuda.synchronize()
    flat = ctx.cpu().numpy()

    def fg(yy):
        return picnn_conv_oracle.energy_and_grad_chain(params, flat, yy, SPEC.H, SPEC.W)
    y_ref, traj_ref, E_ref = gd_ref.unroll_f32(fg, y0, K, LR, MU)
    assert np.array_equal(traj.cpu().numpy(), traj_ref)
    assert np.array_equal(y.cpu().numpy(), y_ref.astype(np.float64))
    assert np.array_equal(E.cpu().numpy(), E_ref)
    assert np.abs(y_ref - y0.astype(np.float32)).max() > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("B", [70, 256])
def test_conv_equals_loop_of_fg(B):
    from icnn_amd import gd
    K = 30
    params, x, y0, _ = _conv_problem(B, B)
    model = picnn.ConvModel(SPEC, params)
    ctx = model.context(torch.from_numpy(x).cuda())
    y0d = torch.from_numpy(y0).cuda()
    y, traj, E = gd.solve(model, ctx, y0d, K, LR, MU, trajectory=True, energy=True)
    yy = y0d.float()
    v = torch.zeros_like(yy)
    lr32, mu32, c1 = (torch.tensor(c, dtype=torch.float32, device="cuda") for c in (LR, MU, 1.0 + MU))
    steps = []
    for _ in range(K):
        steps.append(yy.double())
        _, g = model.fg(ctx, yy.double().contiguous())
        mv = mu32 * v
        vn = mv - lr32 * g
        yy = (yy - mv) + c1 * vn
        v = vn
    E_ref, _ = model.fg(ctx, yy.double().contiguous())
    torch.cuda.synchronize()
    assert torch.equal(traj, torch.stack(steps, 1))
    assert torch.equal(y, yy.double()) and torch.equal(E, E_ref)


@pytest.mark.gpu
def test_completion_gradient_against_float64_surrogate_on_the_device_trajectory():
    """Reference batch 70, nGdIter 30, loss mean((255 (y_K - t))^2): relative Frobenius error <= 1e-4 per variable against
    surrogate_grad64 on the device's trajectory and ybar; z4_u/* exactly zero (c = 0: nothing reaches them)."""
    from icnn_amd import gd, train
    B, K = 70, 30
    params, x, y0, rng = _conv_problem(B, 0)
    t = rng.rand(B, SPEC.n_labels)
    model = picnn.ConvModel(SPEC, params)
    xd = torch.from_numpy(x).cuda()
    ctx = model.context(xd)
    y, traj, _ = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, LR, MU, trajectory=True)
    ybar = 2.0 * 255.0 ** 2 * (y - torch.from_numpy(t).cuda()) / y.numel()
    g = train.unrolled_grad(model, xd, traj, ybar, LR, MU)
    g2 = train.unrolled_grad(model, xd, traj, ybar, LR, MU, flat=True)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat([v.reshape(-1) for v in g.values()]), g2)
    trajh, ybarh = traj.cpu().numpy(), ybar.cpu().numpy()
    v = (gd.coefficients(K, LR, MU)[None, :, None] * ybarh[:, None, :]).reshape(B * K, -1)
    g64, _, margin = train_conv_ref.surrogate_grad64(SPEC, params, np.repeat(x, K, axis=0), trajh.reshape(B * K, -1), v,
                                                     np.zeros(B * K))
    top = max(float(np.linalg.norm(r)) for r in g64.values())
    print("completion %dx%d: min |z pre-activation| %.2e" % (B, K, margin))
    for k, ref in g64.items():
        got = g[k].double().cpu().numpy().reshape(ref.shape)
        if k.startswith("z4_u/"):
            assert np.all(got == 0), k
            continue
        err, size = float(np.linalg.norm(got - ref)), float(np.linalg.norm(ref))
        print("  %-16s |g - g64|_F = %.2e  |g64|_F = %.2e" % (k, err, size))
        if size == 0:
            assert err <= 1e-6 * top, (k, err)
            continue
        assert err <= 1e-4 * size, (k, err, size)
