"""Back-optimisation inference of the FC PICNN (icnn_amd.gd, be_gd.hip) and its training gradient (train.unrolled_grad):
the step coefficients and the reduction of the unrolled gradient to one surrogate over the trajectory (float64, CPU), the C
entries' argument checks, and on the device the trajectory bit for bit against the float32 recurrence around the MFMA-order
oracle, the gradient against float64 autograd through the unroll, and one captured training step."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import gd_ref
import train_ref
from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_gd_workspace_bytes", "icnn_be_fc_gd", "icnn_be_conv_gd"]
LR, MU = 0.01, 0.3                       # multi-label defaults (icnn-back.py)


def _small_spec():
    return picnn.FCSpec(20, 12, (24, 12), batchnorm=True)          # the small spec of test_train_grad.py, BN on


def _fc_energy(spec):
    def energy(theta, x, y):                         # E and the masked pre-activations (not the final scalar layer's)
        E, pre = train_ref.energy(spec, theta, x, y)
        return E, pre[:-1]
    return energy


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("K,lr,mu", [(1, 0.01, 0.3), (5, 0.01, 0.3), (30, 0.01, 0.9), (7, 0.5, -0.2)])
def test_coefficients_are_the_jacobian_of_the_recurrence(K, lr, mu):
    from icnn_amd import gd
    gs = [torch.zeros(1, dtype=torch.float64, requires_grad=True) for _ in range(K)]
    y, v = torch.zeros(1, dtype=torch.float64), 0
    for g in gs:
        prev = v
        v = mu * prev - lr * g
        y = y - mu * prev + (1.0 + mu) * v
    jac = torch.autograd.grad(y.sum(), gs)
    ref = np.array([float(j) for j in jac])
    got = gd.coefficients(K, lr, mu)
    assert got.dtype == np.float64 and got.shape == (K,)
    assert np.allclose(got, ref, rtol=1e-14, atol=0), (got, ref)
    with pytest.raises(ValueError):
        gd.coefficients(0, lr, mu)


@pytest.mark.parametrize("K", [5, 10])
def test_unrolled_gradient_is_one_surrogate_over_the_trajectory(K):
    """The derivation of DESIGN.md §12 on the small spec in float64: autograd through the unrolled loop equals the gradient
    of sum_k <dE/dy(x, y_k), coef_k ybar> over the B K rows with BatchNorm over the repeated rows."""
    from icnn_amd import gd
    spec = _small_spec()
    rng = np.random.RandomState(K)
    params = picnn.init_params(spec, K, "spread")
    for k in params:
        if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    B = 6
    x = rng.rand(B, spec.n_features).astype(np.float32)
    y0 = rng.rand(B, spec.n_labels)
    t = (rng.rand(B, spec.n_labels) < 0.3).astype(np.float64)
    lr, mu = 0.1, 0.3
    g1, yK, traj, ybar, _ = gd_ref.unrolled_autograd(_fc_energy(spec), params, x, y0, t, K, lr, mu)
    assert traj.shape == (B, K, spec.n_labels)
    assert np.abs(yK - y0).max() > 1e-3                                          # y did move
    g2 = gd_ref.surrogate_form(_fc_energy(spec), params, x, traj, ybar, gd.coefficients(K, lr, mu))
    nonzero = 0
    for k in params:
        scale = float(np.abs(g1[k]).max())
        assert float(np.abs(g2[k] - g1[k]).max()) <= 1e-10 * scale, (k, scale)
        nonzero += scale > 0
    assert nonzero > len(params) // 2


def test_new_exports_in_header_and_library():
    from icnn_amd import _lib
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()


def test_workspace_query():
    from icnn_amd import _lib
    lib = _lib.load()
    a = lib.icnn_be_gd_workspace_bytes(128, 159)
    assert a >= 2 * 128 * 159 * 4 + 128 * 4
    assert lib.icnn_be_gd_workspace_bytes(1024, 159) > a
    assert lib.icnn_be_gd_workspace_bytes(0, 159) > 0
    assert lib.icnn_be_gd_workspace_bytes(-1, 159) == 0
    assert lib.icnn_be_gd_workspace_bytes(4, 0) == 0


def _fc_struct(spec):
    from icnn_amd import _lib
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = spec.alpha, int(spec.action_box), spec.ctx_width
    m.wpack = 64
    return m


def test_fc_entry_rejects_bad_arguments_before_launch():
    """Placeholder pointers everywhere: every call below must be refused on the host (nothing would survive a launch)."""
    from icnn_amd import _lib
    lib = _lib.load()
    spec = picnn.bibtex_spec()
    m = _fc_struct(spec)
    fake = C.c_void_p(64)

    def call(mm=m, batch=4, K=3, lr=LR, mu=MU, ctx=fake, y0=fake, y=fake, ws=fake):
        return lib.icnn_be_fc_gd(None if mm is None else C.byref(mm), ctx, y0, batch, K, lr, mu, y, None, None, ws, None)
    assert call(K=0) == -1
    assert call(K=-5) == -1
    assert call(batch=-1) == -1
    for bad in (float("nan"), float("inf"), -float("inf"), 1e300):                # 1e300: float32(lr) overflows
        assert call(lr=bad) == -1, bad
        assert call(mu=bad) == -1, bad
    assert call(mm=None) == -1
    assert call(ctx=None) == -1
    assert call(y0=None) == -1
    assert call(y=None) == -1
    assert call(ws=None) == -1
    m2 = _fc_struct(spec)
    m2.wpack = None
    assert call(mm=m2) == -1
    m3 = _fc_struct(spec)
    m3.width[spec.n_layers - 1] = 2                   # last layer not scalar
    assert call(mm=m3) == -1
    m4 = _fc_struct(spec)
    m4.ctx_width += 1
    assert call(mm=m4) == -1
    m5 = _fc_struct(picnn.halfcheetah_spec())
    m5.action_box = 1                                 # the RL wrapper's box: not a back-optimisation model
    assert call(mm=m5) == -1
    assert call(batch=0) == 0                         # nothing to do, nothing launched


def test_python_solve_refuses_bad_context():
    from icnn_amd import gd
    spec = _small_spec()

    class _M:                                          # solve checks the context before touching the library
        pass
    m = _M()
    m.spec, m.device = spec, torch.device("cpu")
    with pytest.raises(AssertionError):
        gd.solve(m, torch.zeros(3, spec.ctx_width + 1), 0.5, 3, LR, MU)
    with pytest.raises(AssertionError):
        gd.solve(m, torch.zeros(3, spec.ctx_width, dtype=torch.float64), 0.5, 3, LR, MU)


# ------------------------------------------------------------------------------------------------ GPU


def _fc_problem(spec, B, seed):
    params = picnn.init_params(spec, seed, "spread")
    rng = np.random.RandomState(seed)
    x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32) if spec.n_features > 100 else \
        rng.rand(B, spec.n_features).astype(np.float32)
    y0 = rng.rand(B, spec.n_labels)                  # float64: rounded on entry
    return params, x, y0


@pytest.mark.gpu
@pytest.mark.parametrize("which,B,K", [("bibtex", 100, 30), ("bibtex", 300, 30), ("bibtex", 1000, 12), ("deep3", 37, 10),
                                       ("deep3", 700, 10)])
def test_fc_trajectory_bit_exact_against_oracle(which, B, K):
    """B = 100, 300: the per-sample rows path (<= 2 samples per CU); 1000 (partial last tile) and 700: the persistent tiles."""
    from icnn_amd import gd
    from oracle import picnn_oracle
    spec = picnn.bibtex_spec() if which == "bibtex" else picnn.FCSpec(40, 24, (64, 48, 32))
    params, x, y0 = _fc_problem(spec, B, B)
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(x))
    y, traj, E = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, LR, MU, trajectory=True, energy=True)
    torch.cuda.synchronize()
    flat = ctx.cpu().numpy()

    def fg(yy):
        return picnn_oracle.energy_and_grad_chain(params, flat, yy, list(spec.szs), spec.alpha)
    y_ref, traj_ref, E_ref = gd_ref.unroll_f32(fg, y0, K, LR, MU)
    assert traj.shape == (B, K, spec.n_labels) and y.dtype == torch.float64
    assert np.array_equal(traj.cpu().numpy(), traj_ref)
    assert np.array_equal(y.cpu().numpy(), y_ref.astype(np.float64))
    assert np.array_equal(E.cpu().numpy(), E_ref)
    assert np.abs(y_ref - y0.astype(np.float32)).max() > 1e-4                   # y did move
    # without the optional outputs: the same y_K
    y2, t2, E2 = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, LR, MU)
    torch.cuda.synchronize()
    assert t2 is None and E2 is None and torch.equal(y2, y)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 1000])
def test_fc_equals_loop_of_fg(B):
    """gd.solve against K calls of model.fg plus the float32 update in torch (what a caller can write without it)."""
    from icnn_amd import gd
    spec = picnn.bibtex_spec()
    params, x, y0 = _fc_problem(spec, B, 3)
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(x))
    K, lr, mu = 8, 0.05, 0.9
    y, _, E = gd.solve(model, ctx, 0.5, K, lr, mu, energy=True)
    yy = torch.full((B, spec.n_labels), 0.5, dtype=torch.float32, device="cuda")
    v = torch.zeros_like(yy)
    lr32, mu32, c1 = (torch.tensor(c, dtype=torch.float32, device="cuda") for c in (lr, mu, 1.0 + mu))
    for _ in range(K):
        _, g = model.fg(ctx, yy.double().contiguous())
        mv = mu32 * v
        vn = mv - lr32 * g
        yy = (yy - mv) + c1 * vn
        v = vn
    E_ref, _ = model.fg(ctx, yy.double().contiguous())
    torch.cuda.synchronize()
    assert torch.equal(y, yy.double()) and torch.equal(E, E_ref)


@pytest.mark.gpu
def test_optional_outputs_do_not_change_y():
    """The loop decides by null pointers what it records: all four combinations of trajectory and energy, on the rows path
    (B = 17) and on the tiles with a partial last tile (530), leave y_K and every output that is present unchanged."""
    from icnn_amd import gd
    spec = _small_spec()
    for B in (17, 530):
        params, x, y0 = _fc_problem(spec, B, 0)
        model = picnn.FCModel(spec, params, "cuda")
        ctx = model.context(torch.from_numpy(x))
        y0 = torch.from_numpy(y0).cuda()
        yf, trajf, Ef = gd.solve(model, ctx, y0, 3, LR, MU, trajectory=True, energy=True)
        for trajectory in (True, False):
            for energy in (True, False):
                y, traj, E = gd.solve(model, ctx, y0, 3, LR, MU, trajectory=trajectory, energy=energy)
                torch.cuda.synchronize()
                assert (traj is not None) == trajectory and (E is not None) == energy
                assert torch.equal(y, yf), (B, trajectory, energy)
                assert traj is None or torch.equal(traj, trajf), (B, trajectory, energy)
                assert E is None or torch.equal(E, Ef), (B, trajectory, energy)


def _small_gd_problem(K, lr, mu):
    """Small spec, screened so that no float64 pre-activation along the whole trajectory (and no u-path / gate
    pre-activation) is within 1e-4 of zero: the float32 masks of the device then agree with the float64 ones."""
    spec = _small_spec()
    for s in range(0, 300):
        rng = np.random.RandomState(s)
        params = picnn.init_params(spec, s, "spread")
        for k in params:
            if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
                params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
        B = 6
        x = rng.rand(B, spec.n_features).astype(np.float32)
        y0 = rng.rand(B, spec.n_labels).astype(np.float32).astype(np.float64)
        t = (rng.rand(B, spec.n_labels) < 0.3).astype(np.float64)
        if train_ref.u_margin(spec, params, x) < 1e-4:
            continue
        g64, yK, traj, ybar, margin = gd_ref.unrolled_autograd(_fc_energy(spec), params, x, y0, t, K, lr, mu)
        if margin < 1e-4:
            continue
        return spec, params, x, y0, t, g64
    raise AssertionError("no screened seed")


@pytest.mark.gpu
def test_small_gradient_against_float64_autograd_through_the_unroll():
    from icnn_amd import gd, train
    K, lr, mu = 5, 0.1, 0.3
    spec, params, x, y0, t, g64 = _small_gd_problem(K, lr, mu)
    model = picnn.FCModel(spec, params, "cuda")
    xd = torch.from_numpy(x).cuda()
    ctx = model.context(xd)
    y, traj, _ = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True)
    ybar = 2.0 * (y - torch.from_numpy(t).cuda()) / y.numel()
    g = train.unrolled_grad(model, xd, traj, ybar, lr, mu)
    torch.cuda.synchronize()
    assert list(g.keys()) == list(params.keys())
    for k, ref in g64.items():
        got = g[k].double().cpu().numpy()
        err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
        assert err <= 1e-4 * scale + 1e-12, (k, err, scale)


def _bibtex_run(B=128, K=30):
    from icnn_amd import gd
    spec = picnn.bibtex_spec()
    params = picnn.init_params(spec, 0, "spread")
    rng = np.random.RandomState(0)
    x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32)
    t = (rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)
    model = picnn.FCModel(spec, params, "cuda")
    xd = torch.from_numpy(x).cuda()
    ctx = model.context(xd)
    y, traj, _ = gd.solve(model, ctx, 0.5, K, LR, MU, trajectory=True)
    ybar = 2.0 * (y - torch.from_numpy(t).cuda()) / y.numel()
    return spec, params, model, x, xd, t, traj, ybar


@pytest.mark.gpu
def test_bibtex_gradient_against_float64_surrogate_on_the_device_trajectory():
    from icnn_amd import gd, train
    B, K = 128, 30
    spec, params, model, x, xd, t, traj, ybar = _bibtex_run(B, K)
    g = train.unrolled_grad(model, xd, traj, ybar, LR, MU)
    torch.cuda.synchronize()
    trajh, ybarh = traj.cpu().numpy(), ybar.cpu().numpy()
    v = (gd.coefficients(K, LR, MU)[None, :, None] * ybarh[:, None, :]).reshape(B * K, -1)
    g64, _, margin = train_ref.surrogate_grad64(spec, params, np.repeat(x, K, axis=0), trajh.reshape(B * K, -1), v,
                                                np.zeros(B * K))
    L = len(spec.szs)
    top = max(float(np.linalg.norm(r)) for r in g64.values())
    print("bibtex %dx%d: min |pre-activation| %.2e" % (B, K, margin))
    for k, ref in g64.items():
        got = g[k].double().cpu().numpy()
        if k.startswith("z%d_u/" % L):                   # the final layer's x-only term: c = 0, nothing reaches it
            assert np.all(got == 0), k
            continue
        err, size = float(np.linalg.norm(got - ref)), float(np.linalg.norm(ref))
        print("  %-16s |g - g64|_F = %.2e  |g64|_F = %.2e" % (k, err, size))
        if size == 0:                                    # no path from <dE/dy, v> to it (x-only additive terms)
            assert err <= 1e-6 * top, (k, err)
            continue
        assert err <= 1e-4 * size, (k, err, size)


@pytest.mark.gpu
def test_whole_training_step_captured_equals_eager():
    """context -> gd.solve -> ybar -> unrolled_grad(flat=True) -> DeviceAdam.step: three replays of one captured step give
    the bits of three eager steps; two eager evaluations of the same step agree."""
    from icnn_amd import gd, train
    spec = picnn.bibtex_spec()
    params = picnn.init_params(spec, 1, "spread")
    B, K = 64, 10
    rng = np.random.RandomState(1)
    xd = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
    td = torch.from_numpy((rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)).cuda()

    def step(model, opt):
        ctx = model.context(xd)
        y, traj, _ = gd.solve(model, ctx, 0.5, K, LR, MU, trajectory=True)
        ybar = 2.0 * (y - td) / y.numel()
        g = train.unrolled_grad(model, xd, traj, ybar, LR, MU, flat=True)
        opt.step(g)
        return y, g

    eager = picnn.FCModel(spec, params, "cuda")
    opt_e = train.DeviceAdam(eager)
    y_a, g_a = (t.clone() for t in step(eager, opt_e))
    check = picnn.FCModel(spec, params, "cuda")
    opt_c = train.DeviceAdam(check)
    y_b, g_b = step(check, opt_c)
    torch.cuda.synchronize()
    assert torch.equal(y_a, y_b) and torch.equal(g_a, g_b)
    for _ in range(2):
        step(eager, opt_e)
    captured = picnn.FCModel(spec, params, "cuda")
    opt_g = train.DeviceAdam(captured)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(captured, opt_g)
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    assert opt_g.t == opt_e.t == 3
    for a, b in ((opt_g.theta, opt_e.theta), (opt_g.m, opt_e.m), (opt_g.v, opt_e.v), (opt_g.arena, opt_e.arena)):
        assert torch.equal(a, b)
    assert not torch.equal(opt_e.theta, opt_c.theta)            # three steps are not one
