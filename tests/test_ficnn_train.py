"""Training of the FICNN (be_train_ficnn.hip, ficnn.GDTrainer): the reduction of the unrolled gradient to one surrogate
over the trajectory (float64, CPU), the surrogate gradient against float64 autograd on the device, and the trainer's step
against a host restatement, its graph capture and its convergence on the moons data."""
import numpy as np
import pytest
import torch

import ficnn_ref
import gd_ref
from icnn_amd import ficnn, gd, train


def _energy(spec):
    def energy(theta, x, y):
        return ficnn_ref.energy(spec, theta, x, y)
    return energy


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("head", ["sum", "linear"])
@pytest.mark.parametrize("K", [5, 30])
def test_unrolled_gradient_is_one_surrogate_over_the_trajectory(head, K):
    """DESIGN.md §12's derivation holds for the FICNN (E piecewise linear in y): autograd through the unroll equals the
    gradient of sum_k <dE/dy(x, y_k), coef_k ybar> over the B K rows, c = 0."""
    spec = ficnn.FICNNSpec(2, 3, (12, 9), head)
    params = ficnn_ref.wide_params(spec, K)
    rng = np.random.RandomState(K)
    B = 7
    x = rng.randn(B, 2)
    y0 = np.full((B, 3), 0.5)
    t = rng.rand(B, 3)
    lr, mu = 0.05, 0.9
    g1, yK, traj, ybar, margin = gd_ref.unrolled_autograd(_energy(spec), params, x, y0, t, K, lr, mu)
    assert np.abs(yK - y0).max() > 1e-3 and margin > 1e-9
    g2 = gd_ref.surrogate_form(_energy(spec), params, x, traj, ybar, gd.coefficients(K, lr, mu))
    L = len(spec.szs)
    for k in params:
        scale = float(np.abs(g1[k]).max())
        assert float(np.abs(g2[k] - g1[k]).max()) <= 1e-10 * max(scale, 1e-300), (k, scale)
        # (biases and x rows move dE/dy only through the masks: their gradient through the unroll is 0 as well)
        unused = head == "sum" and (k.startswith("z_x%d/" % L) or k.startswith("z_z%d_" % L))
        assert scale == 0 if unused else (scale > 0 or not k.endswith("/W")), k


# ------------------------------------------------------------------------------------------------ GPU

F32 = 2.0 ** -24


@pytest.mark.gpu
@pytest.mark.parametrize("head", ["sum", "linear"])
@pytest.mark.parametrize("with_v", [False, True])
def test_surrogate_grad_against_float64(head, with_v):
    spec = ficnn.FICNNSpec(3, 4, (40, 33, 17), head)
    params = ficnn_ref.wide_params(spec, 3)
    rng = np.random.RandomState(1)
    counts = np.array([3, 0, 1, 5, 0, 2, 4])                   # samples without rows included
    B, R = len(counts), int(counts.sum())
    x = rng.randn(B, 3).astype(np.float32)
    y = rng.rand(R, 4).astype(np.float32).astype(np.float64)
    v = rng.randn(R, 4) if with_v else None
    c = rng.randn(R)
    ref, _ = ficnn_ref.surrogate_grad64(spec, params, x, counts, y, v, c)
    model = ficnn.FICNNModel(spec, params)
    off = torch.tensor(np.r_[0, np.cumsum(counts)], dtype=torch.int32, device="cuda")
    rows = (torch.from_numpy(y).cuda(), None if v is None else torch.from_numpy(v).cuda(), torch.from_numpy(c).cuda())
    g = train.surrogate_grad(model, torch.from_numpy(x).cuda(), rows if with_v else (rows[0], rows[2]), row_offset=off,
                             flat=True)
    if with_v:
        g = train.surrogate_grad(model, torch.from_numpy(x).cuda(), rows, row_offset=off, flat=True)
    g2 = train.surrogate_grad(model, torch.from_numpy(x).cuda(), rows if with_v else (rows[0], rows[2]), row_offset=off,
                              flat=True)
    assert torch.equal(g, g2)
    got = {k: t.cpu().numpy() for k, t in train.unpack_grad(spec, g).items()}
    L = len(spec.szs)
    for k in params:
        scale = float(np.abs(ref[k]).max())
        if head == "sum" and (k.startswith("z_x%d/" % L) or k.startswith("z_z%d_" % L)):
            assert scale == 0 and not got[k].any(), k
            continue
        assert float(np.abs(got[k] - ref[k]).max()) <= 1e-4 * scale + 1e-6, (k, float(np.abs(got[k] - ref[k]).max()), scale)


def _host_step(spec, params, x, t, K, lr, mu, adam_state):
    """context, GD, loss, unrolled gradient in float64 autograd, TFAdam and project, on the host"""
    g, yK, _, _, _ = gd_ref.unrolled_autograd(_energy(spec), params, x, np.full(t.shape, 0.5), t, K, lr, mu)
    loss = float(np.mean((yK - t) ** 2))
    tp = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
    if adam_state[0] is None:
        adam_state[0] = train.TFAdam(tp, lr=1e-3)
    opt = adam_state[0]
    opt.params = tp
    for k in list(opt.m):
        opt.m[k] = opt.m[k].to(torch.float64)
        opt.v[k] = opt.v[k].to(torch.float64)
    opt.step({k: torch.tensor(v) for k, v in g.items()})
    new = ficnn.project({k: v.numpy().astype(np.float32) for k, v in tp.items()})
    return new, loss


def _moons(B, seed):
    rng = np.random.RandomState(seed)
    h = B // 2
    a = np.linspace(0, np.pi, h)
    b = np.linspace(0, np.pi, B - h)
    X = np.r_[np.c_[np.cos(a), np.sin(a)], np.c_[1 - np.cos(b), 1 - np.sin(b) - 0.5]] + 0.1 * rng.randn(B, 2)
    Y = np.r_[np.zeros(h), np.ones(B - h)].reshape(B, 1)
    return X.astype(np.float32), Y.astype(np.float32)


@pytest.mark.gpu
def test_trainer_step_against_host_restatement():
    spec = ficnn.synthetic_spec()
    params = ficnn.make_convex(ficnn.init_params(spec, 0))
    x, t = _moons(100, 0)
    model = ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()})
    tr = ficnn.GDTrainer(model, 100)
    head0 = {k: v.copy() for k, v in params.items() if k.startswith("z_x2/") or k.startswith("z_z2_")}
    state = [None]
    host = {k: v.copy() for k, v in params.items()}
    for s in range(3):
        loss = float(tr.step(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()).item())
        host, hloss = _host_step(spec, host, x, t, 30, 0.01, 0.9, state)
        assert abs(loss - hloss) <= 1e-4 * hloss, (s, loss, hloss)
        dev = tr.host_params()
        for k in host:
            diff = np.abs(dev[k] - host[k]).max()
            assert diff <= 2e-5 + 1e-3 * np.abs(host[k]).max(), (s, k, diff)
    dev = tr.host_params()
    for k, v in head0.items():
        assert np.array_equal(dev[k], v), k


@pytest.mark.gpu
def test_captured_step_replays_as_eager_steps():
    spec = ficnn.synthetic_spec()
    params = ficnn.make_convex(ficnn.init_params(spec, 1))
    x, t = _moons(100, 1)
    xs, ts = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    a = ficnn.GDTrainer(ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()}), 100)
    b = ficnn.GDTrainer(ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()}), 100)
    k = 4
    la = [float(a.step(xs, ts).item()) for _ in range(k + 1)]
    b.step(xs, ts)                                         # warm-up (allocator, cached coefficients) outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loss = b.step()
    torch.cuda.current_stream().wait_stream(s)
    lb = []
    for _ in range(k):
        graph.replay()
        lb.append(float(loss.item()))
    torch.cuda.synchronize()
    assert la[1:] == lb
    assert torch.equal(a.opt.theta, b.opt.theta)
    assert a.t_steps == b.t_steps == k + 1


@pytest.mark.gpu
def test_loss_decreases_on_moons():
    spec = ficnn.synthetic_spec()
    params = ficnn.make_convex(ficnn.init_params(spec, 2))
    x, t = _moons(100, 2)
    tr = ficnn.GDTrainer(ficnn.FICNNModel(spec, params), 100)
    xs, ts = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    first = float(tr.step(xs, ts).item())
    for _ in range(99):
        last = tr.step()
    last = float(last.item())
    assert last < first, (first, last)
