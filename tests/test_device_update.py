"""Parameter update on the device (train.DeviceAdam, icnn_be_param_update, be_train_update.hip): the map from the flat theta
into the weight arena against the host packers (CPU), one launch against its NumPy float32 restatement bit for bit, several
steps against TFAdam + picnn.project, graph capture, and one whole training step against the documented host path."""
import ctypes as C

import numpy as np
import pytest
import torch

from icnn_amd import _lib, bundle_entropy, picnn, train

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
ULPS_PER_STEP = 4          # DeviceAdam vs TFAdam + project: |theta difference| <= steps * 4 ulp(max(|theta|, lr))


def _problem(which, seed=0):
    if which == "bibtex":
        spec = picnn.bibtex_spec()
        return spec, picnn.init_params(spec, seed, "spread"), picnn.FCModel
    if which == "rl":
        spec = picnn.halfcheetah_spec()
        return spec, picnn.init_params(spec, seed, "init", yu_bias=1.0, gate_bias=1.0), picnn.FCModel
    if which == "deep":        # 8 z-layers, six batch-normalised u-layers (tests/test_architectures.py)
        from test_architectures import DEEP
        return DEEP, picnn.init_params(DEEP, seed, "spread"), picnn.FCModel
    spec = picnn.ConvSpec()
    return spec, picnn.init_conv_params(spec, seed, "spread"), picnn.ConvModel


def _flat(spec, params):
    return np.concatenate([np.asarray(params[k], np.float32).reshape(-1) for k, _ in train.grad_layout(spec)])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ------------------------------------------------------------------------------------------------ CPU: the map


@pytest.mark.parametrize("which", ["bibtex", "rl", "deep", "conv"])
def test_map_scatter_equals_host_packers(which):
    """The map applied as a NumPy scatter to random parameters = icnn_be_*_pack + the stage / gamma / beta buffers that
    repack / repack_context upload, bit for bit, at the arena's offsets; padding stays zero."""
    spec, _, Model = _problem(which)
    rng = np.random.RandomState(5)
    params = {k: rng.randn(*shape).astype(np.float32) for k, shape in train.grad_layout(spec)}
    model = Model(spec, params, "cpu")
    pm = train.ParamMap(model)
    img = pm.scatter(_flat(spec, params))
    offs = pm.offsets
    uploaded = [model.wpack] + list(model._ctx_keep)
    assert len(uploaded) == len(offs)
    covered = np.zeros(pm.arena_floats, bool)
    for t, off in zip(uploaded, offs):
        a = t.numpy().reshape(-1)
        assert np.array_equal(_bits(img[off:off + a.size]), _bits(a))
        covered[off:off + a.size] = True
    assert not img[~covered].any()
    assert np.array_equal(_bits(img), _bits(train.arena_image(model, params)[0]))
    print("%s: %d parameters, arena %d floats, %d copies, max fan-out %d"
          % (which, pm.n, pm.arena_floats, pm.dest.size, pm.max_fanout))


@pytest.mark.parametrize("which", ["bibtex", "rl", "deep", "conv"])
def test_every_arena_float_has_one_source(which):
    spec, params, Model = _problem(which)
    model = Model(spec, params, "cpu")
    pm = train.ParamMap(model)
    assert pm.dest.size == np.unique(pm.dest).size               # no arena float is written from two parameters
    idx = train.arena_image(model, train.index_params(train.grad_layout(spec)))[0]
    nz = np.nonzero(idx)[0]
    assert np.array_equal(np.sort(pm.dest), nz)                  # every non-padding float is written, padding never
    src = np.repeat(np.arange(pm.n), np.diff(pm.dest_off))
    assert np.array_equal(idx[pm.dest].astype(np.int64) - 1, src)
    assert pm.dest_off[0] == 0 and pm.dest_off[-1] == pm.dest.size and (np.diff(pm.dest_off) >= 0).all()
    expect = {"bibtex": 2, "rl": 2, "deep": 2, "conv": 3}[which]
    assert pm.max_fanout == expect


@pytest.mark.parametrize("which", ["bibtex", "rl", "deep", "conv"])
def test_arena_offsets_are_256_byte_aligned(which):
    spec, params, Model = _problem(which)
    model = Model(spec, params, "cpu")
    offs, total = train.arena_offsets(model.arena_parts(params))
    assert all((4 * o) % 256 == 0 for o in offs) and (4 * total) % 256 == 0
    assert offs == sorted(offs) and len(set(offs)) == len(offs)


def test_index_image_guard():
    """float(j + 1) is exact only up to 2^24: a larger layout is refused instead of silently aliasing indices."""
    with pytest.raises(ValueError, match="2\\^24"):
        train.index_params([("a/W", (4096, 4096)), ("a/b", (1,))])
    small = train.index_params([("a/W", (2, 3)), ("a/b", (3,))])
    assert small["a/W"].reshape(-1).tolist() == [1, 2, 3, 4, 5, 6] and small["a/b"].tolist() == [7, 8, 9]


def test_attached_model_refuses_repack_and_keeps_params_live():
    spec, params, _ = _problem("rl")
    model = picnn.FCModel(spec, params, "cpu")
    ref_pack, ref_keep = model.wpack.clone(), [t.clone() for t in model._ctx_keep]
    opt = train.DeviceAdam(model)
    for call in (lambda: model.repack(params), lambda: model.repack_context(params), lambda: model.clamp("proj")):
        with pytest.raises(RuntimeError, match="DeviceAdam"):
            call()
    assert torch.equal(model.wpack, ref_pack)                         # the same bits, now inside the arena
    for t, off in zip(ref_keep, opt.map.offsets[1:]):
        assert torch.equal(opt.arena[off:off + t.numel()], t.reshape(-1))
    assert model.c_model.wpack == opt.arena.data_ptr() + 4 * opt.map.offsets[0]
    assert model.c_ctx.w_stage[0] == opt.arena.data_ptr() + 4 * opt.map.offsets[1]
    hp = opt.host_params()
    assert set(hp) == set(params) and all(np.array_equal(hp[k], params[k]) for k in params)
    opt.theta[0] = 7.0                                                 # model.params are views of theta
    assert float(model.params["u0/W"].reshape(-1)[0]) == 7.0
    new = {k: v + np.float32(1) for k, v in params.items()}
    opt.load(new)
    assert np.array_equal(_bits(opt.arena.numpy()), _bits(train.arena_image(model, new)[0]))
    with pytest.raises(RuntimeError, match="already attached"):
        train.DeviceAdam(model)


def test_param_update_abi():
    lib = _lib.load()
    assert lib.icnn_be_struct_size(6) == C.sizeof(_lib.ParamUpdateArgs)
    assert lib.icnn_be_abi_version() == 12
    a = _lib.ParamUpdateArgs()
    assert lib.icnn_be_param_update(None, None) == -1
    assert lib.icnn_be_param_update(C.byref(a), None) == -1            # n = 0, NULL buffers: refused, nothing launched
    a.n, a.theta, a.m, a.v, a.grad, a.dest_off, a.dest, a.arena, a.step = 4, 16, 32, 48, 66, 80, 96, 112, 128
    a.beta1, a.beta2, a.eps = B1, B2, EPS
    assert lib.icnn_be_param_update(C.byref(a), None) == -1            # misaligned gradient
    a.grad, a.n_proj = 64, _lib.MAX_PROJ_RANGES + 1
    assert lib.icnn_be_param_update(C.byref(a), None) == -1
    a.n_proj, a.proj_begin[0], a.proj_end[0] = 1, 2, 5
    assert lib.icnn_be_param_update(C.byref(a), None) == -1            # range beyond n
    a.proj_end[0], a.beta2 = 4, 1.0
    assert lib.icnn_be_param_update(C.byref(a), None) == -1


# ------------------------------------------------------------------------------------------------ GPU


def _restated_step(theta, m, v, g, t, proj):
    """The kernel's arithmetic in NumPy float32 (be_train_update.hip): every operation rounded, no contraction."""
    b1, c1, b2, c2 = np.float32(B1), np.float32(1.0 - B1), np.float32(B2), np.float32(1.0 - B2)
    lr_t = np.float32(train.adam_lr_t(LR, B1, B2, t))
    m = b1 * m + c1 * g
    v = b2 * v + c2 * (g * g)
    theta = theta - (lr_t * m) / (np.sqrt(v) + np.float32(EPS))
    for b, e in proj:
        seg = theta[b:e]
        theta[b:e] = np.where(seg < 0, np.float32(0), seg)
    return theta, m, v


def _random_grad(n, rng, scale=1e-2):
    g = (scale * rng.randn(n)).astype(np.float32)
    g[rng.rand(n) < 0.05] = 0                  # some entries without a gradient at all
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bibtex", "rl", "deep", "conv"])
@pytest.mark.parametrize("t", [1, 7])
def test_one_step_matches_numpy_restatement(which, t):
    spec, params, Model = _problem(which, 3)
    model = Model(spec, params, "cuda")
    opt = train.DeviceAdam(model, LR, B1, B2, EPS)
    n, rng = opt.n, np.random.RandomState(t)
    theta = _flat(spec, params)
    m = (1e-3 * rng.randn(n)).astype(np.float32)
    v = (1e-6 * rng.rand(n)).astype(np.float32)
    g = _random_grad(n, rng)
    zero = g == 0
    m[zero], v[zero] = 0, 0                    # never-touched entries: theta must stay exactly
    opt.m.copy_(torch.from_numpy(m))
    opt.v.copy_(torch.from_numpy(v))
    opt.step_count.copy_(torch.tensor([t - 1, 0], dtype=torch.int32))
    opt.step(torch.from_numpy(g).cuda())
    torch.cuda.synchronize()
    th_r, m_r, v_r = _restated_step(theta.copy(), m, v, g, t, opt.map.proj)
    assert np.array_equal(_bits(opt.theta.cpu().numpy()), _bits(th_r))
    assert np.array_equal(_bits(opt.m.cpu().numpy()), _bits(m_r))
    assert np.array_equal(_bits(opt.v.cpu().numpy()), _bits(v_r))
    assert np.array_equal(_bits(th_r[zero]), _bits(theta[zero]))
    assert opt.step_count.cpu().tolist() == [t, 0]
    restated = {k: a.numpy() for k, a in train.unpack_grad(spec, torch.from_numpy(th_r)).items()}
    ref_arena = train.arena_image(model, restated)[0]
    assert np.array_equal(_bits(opt.arena.cpu().numpy()), _bits(ref_arena))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bibtex", "rl", "deep", "conv"])
def test_five_steps_against_tfadam_and_project(which):
    spec, params, Model = _problem(which, 4)
    model = Model(spec, params, "cuda")
    opt = train.DeviceAdam(model, LR, B1, B2, EPS)
    theta = {k: torch.from_numpy(v).cuda() for k, v in params.items()}
    ref = train.TFAdam(theta, LR, B1, B2, EPS)
    rng = np.random.RandomState(11)
    worst, steps = 0.0, 5
    for k in range(1, steps + 1):
        g = torch.from_numpy(_random_grad(opt.n, rng)).cuda()
        opt.step(g)
        ref.step(train.unpack_grad(spec, g))
        proj = picnn.project({name: t.cpu().numpy() for name, t in theta.items()})
        theta.update({name: torch.from_numpy(a).cuda() for name, a in proj.items()})
        ref.params = theta
        want = _flat(spec, proj)
        got = opt.theta.cpu().numpy()
        ulp = np.spacing(np.maximum(np.abs(want), np.float32(LR)))
        err = float(np.max(np.abs(got.astype(np.float64) - want) / ulp))
        worst = max(worst, err)
        assert err <= ULPS_PER_STEP * k, (k, err)
    hp = opt.host_params()
    for b, e in opt.map.proj:
        assert (opt.theta[b:e] >= 0).all()
    assert all(np.array_equal(hp[name], a) for name, a in train.unpack_grad(spec, opt.theta.cpu()).items())
    assert opt.t == steps
    print("%s: %d steps, bound %d ulp per step (of max(|theta|, lr)), observed max %.2f ulp"
          % (which, steps, ULPS_PER_STEP, worst))


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["bibtex", "conv"])
def test_captured_step_replays_and_captured_kernels_read_new_weights(which):
    spec, params, Model = _problem(which, 6)
    B, n_iter = (32, 6) if which == "bibtex" else (8, 4)
    rng = np.random.RandomState(2)
    if which == "bibtex":
        x = torch.from_numpy((rng.rand(B, spec.n_features) < 0.04).astype(np.float32)).cuda()
    else:
        x = torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda()
    y = torch.from_numpy(0.2 + 0.6 * rng.rand(B, spec.n_labels)).cuda()
    eager_model, model = Model(spec, params, "cuda"), Model(spec, params, "cuda")
    eager, opt = train.DeviceAdam(eager_model), train.DeviceAdam(model)
    g = torch.from_numpy((1e-2 * rng.randn(opt.n)).astype(np.float32)).cuda()
    solver = bundle_entropy.FusedSolver(model, B, n_iter)
    torch.cuda.synchronize()
    # captured before any update: the context, an energy evaluation, a fused solve, and the update itself
    g_ctx, g_fg, g_solve, g_step = (torch.cuda.CUDAGraph() for _ in range(4))
    with torch.cuda.graph(g_ctx):
        ctx = model.context(x)
    with torch.cuda.graph(g_fg):
        f, dy = model.fg(ctx, y)
    with torch.cuda.graph(g_solve):
        res = solver.solve(ctx, 0.5)
    with torch.cuda.graph(g_step):
        opt.step(g)
    for _ in range(4):
        g_step.replay()
        eager.step(g)
    g_ctx.replay()
    g_fg.replay()
    g_solve.replay()
    torch.cuda.synchronize()
    for a, b in ((opt.theta, eager.theta), (opt.m, eager.m), (opt.v, eager.v), (opt.arena, eager.arena),
                 (opt.step_count, eager.step_count)):
        assert torch.equal(a, b)
    assert opt.t == 4
    fresh = Model(spec, opt.host_params(), "cuda")
    ctx_f = fresh.context(x)
    f_f, dy_f = fresh.fg(ctx_f, y)
    res_f = bundle_entropy.FusedSolver(fresh, B, n_iter).solve(ctx_f, 0.5)
    torch.cuda.synchronize()
    assert torch.equal(ctx, ctx_f)
    assert torch.equal(f, f_f) and torch.equal(dy, dy_f)
    assert torch.equal(res.y, res_f.y) and torch.equal(res.count[:B], res_f.count[:B])
    assert not torch.equal(ctx_f, Model(spec, params, "cuda").context(x))     # the weights did change


def _train_data(which, B, rng):
    spec = picnn.bibtex_spec() if which == "bibtex" else picnn.ConvSpec()
    if which == "bibtex":
        x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32)
        y = (rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)
    else:
        x = rng.rand(B, spec.H, spec.W, 1).astype(np.float32)
        y = rng.rand(B, spec.n_labels)
    return torch.from_numpy(x).cuda(), y


def _train_step(model, x, y, n_iter, loss, conv):
    """solve -> implicit_feed -> surrogate_grad(flat=True); returns the flat gradient"""
    B = x.shape[0]
    if conv:
        y0 = torch.full((B, model.spec.n_labels), 0.5, dtype=torch.float64, device="cuda")
        res = bundle_entropy.FusedSolver(model, B, n_iter).solve(model.context(x), y0)
        model.context(x, bn_updates=res.fg_evaluations())
        feed = bundle_entropy.implicit_feed(res, y, loss)
        return train.surrogate_grad(model, x, feed, bn_updates=1, flat=True)
    res = bundle_entropy.FusedSolver(model, B, n_iter).solve(model.context(x), 0.5)
    feed = bundle_entropy.implicit_feed(res, y, loss)
    return train.surrogate_grad(model, x, feed, flat=True)


@pytest.mark.gpu
@pytest.mark.parametrize("which,B,n_iter,loss", [("bibtex", 128, 10, "xent"), ("conv", 70, 5, "mse")])
def test_training_step_device_update_matches_host_path(which, B, n_iter, loss):
    conv = which == "conv"
    spec, params, Model = _problem(which, 8)
    x, y = _train_data(which, B, np.random.RandomState(9))
    # the documented host path: TFAdam -> picnn.project -> repack
    host_model = Model(spec, params, "cuda")
    theta = {k: torch.from_numpy(v).cuda() for k, v in params.items()}
    ref = train.TFAdam(theta, LR, B1, B2, EPS)
    g_host = _train_step(host_model, x, y, n_iter, loss, conv)
    ref.step(train.unpack_grad(spec, g_host))
    new = picnn.project({k: t.cpu().numpy() for k, t in theta.items()})
    host_model.repack(new)
    # the device path
    model = Model(spec, params, "cuda")
    opt = train.DeviceAdam(model, LR, B1, B2, EPS)
    g_dev = _train_step(model, x, y, n_iter, loss, conv)
    opt.step(g_dev)
    torch.cuda.synchronize()
    assert torch.equal(g_host, g_dev)
    want, got = _flat(spec, new), opt.theta.cpu().numpy()
    ulp = np.spacing(np.maximum(np.abs(want), np.float32(LR)))
    err = float(np.max(np.abs(got.astype(np.float64) - want) / ulp))
    print("%s training step: max |theta_device - theta_host| = %.2f ulp (bound %d)" % (which, err, ULPS_PER_STEP))
    assert err <= ULPS_PER_STEP
    for k, t in host_model.bn_stats.items():
        assert torch.equal(t, model.bn_stats[k]), k
    assert int(np.count_nonzero(got != _flat(spec, params))) > 0
