"""BatchNorm moving statistics: inference-mode contexts (icnn_be_fc_context_bn /
icnn_be_conv_context_bn with ICNN_BE_BN_MOVING), the folds of training mode in the context producer and in
surrogate_grad, and the fold count of a solve (bundle_entropy.fg_evaluations)."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import bn_ref
from icnn_amd import _lib, bundle_entropy, picnn
from oracle import bundle_entropy_oracle as oracle

NEW_EXPORTS = ["icnn_be_fc_context_bn_work_floats", "icnn_be_fc_context_bn", "icnn_be_conv_context_bn_work_floats",
               "icnn_be_conv_context_bn", "icnn_be_fc_surrogate_grad_bn", "icnn_be_conv_surrogate_grad_bn"]
BATCH, MOVING = _lib.BN_MODE["batch"], _lib.BN_MODE["moving"]


def _bn_halfcheetah():
    return dataclasses.replace(picnn.halfcheetah_spec(), batchnorm=True)


def _fc_structs(spec):
    """FcModel / FcCtx with placeholder pointers: enough for the argument checks that run before any launch."""
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width, m.wpack = spec.alpha, int(spec.action_box), spec.ctx_width, 64
    c = _lib.FcCtx()
    c.n_features, c.n, c.n_layers = spec.n_features, spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        c.width[i] = w
        c.w_stage[i] = c.b_stage[i] = c.bn_gamma[i] = c.bn_beta[i] = 64
    c.batchnorm, c.bn_eps = int(spec.batchnorm), 1e-5
    return m, c


def _conv_structs():
    spec = picnn.ConvSpec()
    m = _lib.ConvModel()
    m.H, m.W = spec.H, spec.W
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        m.filters[l], m.ksize[l], m.stride[l] = nf, k, s
    m.fc_hidden, m.ctx_width, m.wpack = picnn.CONV_FCS[0], spec.ctx_width, 64
    c = _lib.ConvCtx()
    for i in range(7):
        c.w_stage[i] = c.b_stage[i] = 64
    for i in range(4):
        c.bn_gamma[i] = c.bn_beta[i] = 64
    c.bn_eps = 1e-5
    return m, c


def _mv(layers, decay=0.9):
    mv = _lib.BnMoving()
    for i in layers:
        mv.mean[i] = mv.var[i] = 64
    mv.decay = decay
    return mv


# ------------------------------------------------------------------------------------------------ CPU


def test_new_exports_declared_and_struct_layout():
    import os
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and name + "(" in header
        getattr(lib, name)
    assert lib.icnn_be_struct_size(5) == C.sizeof(_lib.BnMoving)
    # the new work queries cover the plain ones plus the exported statistics
    m, c = _fc_structs(picnn.bibtex_spec())
    assert lib.icnn_be_fc_context_bn_work_floats(C.byref(c), 128) >= lib.icnn_be_fc_context_work_floats(C.byref(c), 128) + 1200
    cm, _ = _conv_structs()
    assert (lib.icnn_be_conv_context_bn_work_floats(C.byref(cm), 70)
            >= lib.icnn_be_conv_context_work_floats(C.byref(cm), 70) + 2 * (32 + 64 + 64 + 512))


def test_bad_bn_arguments_are_rejected_before_launch():
    """ICNN_BE_EINVAL for an unknown mode, updates < 0, folds in moving mode, and -- where mv is needed -- mv == NULL, a
    NULL statistics vector or a decay outside [0, 1].  Every call here must fail before it launches (no GPU needed)."""
    lib = _lib.load()
    fake = C.c_void_p(64)
    spec = picnn.bibtex_spec()
    m, c = _fc_structs(spec)

    def fc(mv, mode, updates):
        return lib.icnn_be_fc_context_bn(C.byref(c), mv, mode, updates, fake, 4, fake, spec.ctx_width, fake, None)

    good = _mv([0])
    assert fc(C.byref(good), 2, 0) == -1
    assert fc(C.byref(good), -1, 0) == -1
    assert fc(C.byref(good), BATCH, -1) == -1
    assert fc(C.byref(good), MOVING, 1) == -1
    assert fc(None, MOVING, 0) == -1
    assert fc(None, BATCH, 1) == -1
    for d in (1.5, -0.1, float("nan")):
        assert fc(C.byref(_mv([0], d)), BATCH, 2) == -1
        assert fc(C.byref(_mv([0], d)), MOVING, 0) == -1
    assert fc(C.byref(_mv([])), MOVING, 0) == -1                   # the layer's vectors are NULL
    # a model without BatchNorm ignores mv, but not the mode or the count
    nbn = dataclasses.replace(spec, batchnorm=False)
    _, c2 = _fc_structs(nbn)
    assert lib.icnn_be_fc_context_bn(C.byref(c2), None, 3, 0, fake, 4, fake, nbn.ctx_width, fake, None) == -1
    assert lib.icnn_be_fc_context_bn(C.byref(c2), None, BATCH, -2, fake, 4, fake, nbn.ctx_width, fake, None) == -1

    def fc_grad(mv, updates):
        return lib.icnn_be_fc_surrogate_grad_bn(C.byref(m), C.byref(c), fake, 4, fake, 8, fake, fake, fake, fake, None, fake,
                                                mv, updates, None)
    assert fc_grad(C.byref(good), -1) == -1
    assert fc_grad(None, 1) == -1
    assert fc_grad(C.byref(_mv([0], 2.0)), 1) == -1

    cm, cc = _conv_structs()

    def conv(mv, mode, updates):
        return lib.icnn_be_conv_context_bn(C.byref(cm), C.byref(cc), mv, mode, updates, fake, 4, fake, fake, None)
    cgood = _mv(range(4))
    assert conv(C.byref(cgood), 7, 0) == -1
    assert conv(C.byref(cgood), BATCH, -1) == -1
    assert conv(C.byref(cgood), MOVING, 3) == -1
    assert conv(None, MOVING, 0) == -1
    assert conv(None, BATCH, 1) == -1
    assert conv(C.byref(_mv(range(3))), MOVING, 0) == -1           # u3's vectors are NULL
    assert conv(C.byref(_mv(range(4), float("inf"))), BATCH, 1) == -1

    def conv_grad(mv, updates):
        return lib.icnn_be_conv_surrogate_grad_bn(C.byref(cm), C.byref(cc), fake, 4, fake, 8, fake, fake, fake, fake, None,
                                                  fake, mv, updates, None)
    assert conv_grad(C.byref(cgood), -1) == -1
    assert conv_grad(None, 1) == -1
    assert conv_grad(C.byref(_mv(range(4), -0.5)), 1) == -1


def test_init_bn_stats_layout():
    b = picnn.init_bn_stats(picnn.bibtex_spec())
    assert list(b) == ["u0/bn/moving_mean", "u0/bn/moving_variance"]
    assert b["u0/bn/moving_mean"].shape == (600,) and b["u0/bn/moving_mean"].dtype == np.float32
    assert (b["u0/bn/moving_mean"] == 0).all() and (b["u0/bn/moving_variance"] == 1).all()
    h = picnn.init_bn_stats(_bn_halfcheetah())
    assert sorted(h) == ["u0/bn/moving_mean", "u0/bn/moving_variance"] and h["u0/bn/moving_variance"].shape == (200,)
    assert picnn.init_bn_stats(picnn.halfcheetah_spec()) == {}
    deep = picnn.init_bn_stats(picnn.FCSpec(45, 11, (70, 33, 18)))
    assert [(k, v.shape) for k, v in deep.items()] == [("u0/bn/moving_mean", (70,)), ("u0/bn/moving_variance", (70,)),
                                                       ("u1/bn/moving_mean", (33,)), ("u1/bn/moving_variance", (33,))]
    cv = picnn.init_bn_stats(picnn.ConvSpec())
    assert [(k, v.shape) for k, v in cv.items()] == [
        ("u%d/bn/%s" % (i, s), (w,)) for i, w in enumerate((32, 64, 64, 512)) for s in ("moving_mean", "moving_variance")]
    # a separate dict: the trainable parameters and the gradient layout do not change
    from icnn_amd import train
    for spec, params in ((picnn.bibtex_spec(), picnn.init_params(picnn.bibtex_spec())),
                         (picnn.ConvSpec(), picnn.init_conv_params(picnn.ConvSpec()))):
        assert not any("moving" in k for k in params)
        assert [n for n, _ in train.grad_layout(spec)] == list(params)


def _fc_problem(spec, B, seed):
    params = picnn.init_params(spec, seed, "spread", **({} if spec.n_features > 100 else dict(yu_bias=1.0, gate_bias=1.0)))
    rng = np.random.RandomState(seed + 100)
    if spec.n_features > 100:
        x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32)
    else:
        x = rng.randn(B, spec.n_features).astype(np.float32)
    return params, x


@pytest.mark.parametrize("which", ["bibtex", "halfcheetah_bn", "small3"])
def test_host_fc_context_moving_mode(which):
    spec = {"bibtex": picnn.bibtex_spec(), "halfcheetah_bn": _bn_halfcheetah(),
            "small3": picnn.FCSpec(45, 11, (70, 33, 18))}[which]
    params, x = _fc_problem(spec, 40, 3)
    stats = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 5)
    ref, _ = bn_ref.fc_context64(spec, params, x, stats)
    host = picnn.context(spec, params, torch.from_numpy(x), bn_stats=stats).numpy()
    assert np.max(np.abs(host - ref)) <= 2e-5 * np.abs(ref).max()
    # one row alone gives the same row
    one = picnn.context(spec, params, torch.from_numpy(x[7:8]), bn_stats=stats).numpy()
    assert np.max(np.abs(one[0] - ref[7])) <= 2e-5 * np.abs(ref).max()
    # moving statistics equal to the batch's own: the batch-mode context
    _, bstats = bn_ref.fc_context64(spec, params, x)
    own = {}
    for i, (mu, var) in bstats.items():
        own["u%d/bn/moving_mean" % i], own["u%d/bn/moving_variance" % i] = mu.astype(np.float32), var.astype(np.float32)
    a = picnn.context(spec, params, torch.from_numpy(x), bn_stats=own).numpy()
    b = picnn.context(spec, params, torch.from_numpy(x)).numpy()
    assert np.max(np.abs(a - b)) <= 2e-5 * np.abs(b).max()


def test_host_conv_context_moving_mode():
    spec = picnn.ConvSpec()
    params = picnn.init_conv_params(spec, 2, "spread")
    x = np.random.RandomState(52).rand(3, spec.H, spec.W, 1).astype(np.float32)
    stats = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 6)
    ref, _ = bn_ref.conv_context64(spec, params, x, stats)
    host = picnn.conv_context(spec, params, torch.from_numpy(x), bn_stats=stats).numpy()
    o = 0
    for name, w in bn_ref.conv_heads(spec):
        scale = max(np.abs(ref[:, o:o + w]).max(), 1e-3)
        assert np.max(np.abs(host[:, o:o + w] - ref[:, o:o + w])) <= 2e-5 * scale, name
        o += w
    _, bstats = bn_ref.conv_context64(spec, params, x)
    own = {}
    for i, (mu, var) in bstats.items():
        own["u%d/bn/moving_mean" % i], own["u%d/bn/moving_variance" % i] = mu.astype(np.float32), var.astype(np.float32)
    a = picnn.conv_context(spec, params, torch.from_numpy(x), bn_stats=own).numpy()
    b = picnn.conv_context(spec, params, torch.from_numpy(x)).numpy()
    assert np.max(np.abs(a - b)) <= 2e-5 * np.abs(b).max()


def test_fold_restatement():
    s = {"u0/bn/moving_mean": np.zeros(3, np.float32), "u0/bn/moving_variance": np.ones(3, np.float32)}
    out = bn_ref.fold32(s, {0: (np.array([1.0, 2.0, -1.0]), np.array([4.0, 0.0, 1.0]))}, 2)
    assert np.allclose(out["u0/bn/moving_mean"], [0.19, 0.38, -0.19], rtol=1e-6)
    assert np.allclose(out["u0/bn/moving_variance"], [1.57, 0.81, 1.0], rtol=1e-6)


def _counting(fg):
    calls = [0]

    def wrapped(y):
        calls[0] += 1
        return fg(y)
    return wrapped, calls


def _energy(ranks, n, seed):
    """per sample u: f = a.y + 0.5 sum_{j < rank_u} (b_j.y)^2 -- its gradients span 1 + rank_u directions, so the rank test
    of the bundle finishes the sample after 1 + rank_u cuts (never, when 1 + rank_u exceeds the iterations)"""
    rng = np.random.RandomState(seed)
    B = len(ranks)
    a = rng.randn(B, n)
    Bm = rng.randn(B, n, n) * (np.arange(n)[None, :, None] < np.asarray(ranks)[:, None, None])

    def fg(y):
        p = np.einsum("ujk,uk->uj", Bm, y)
        return (a * y).sum(1) + 0.5 * (p * p).sum(1), a + np.einsum("ujk,uj->uk", Bm, p)
    return fg


@pytest.mark.parametrize("variant", ["dual", "pdipm"])
@pytest.mark.parametrize("ranks,n_iter", [([0, 0, 0], 6), ([0, 1, 1, 0], 6), ([0, 1, 2, 0], 8), ([0, 1, 8], 5), ([8, 8], 4), ([2], 3)])
def test_fg_evaluations_counts_the_reference_calls(variant, ranks, n_iter):
    """The fold count of one training iteration: solveBatch evaluates fg (and with it the BatchNorm op) once per outer
    iteration until every sample has finished."""
    n = 8
    fg, calls = _counting(_energy(ranks, n, 11))
    y0 = np.full((len(ranks), n), 0.5)
    with np.errstate(all="ignore"):
        res = oracle.solve_batch(fg, y0, n_iter, variant=variant)
    assert bundle_entropy.fg_evaluations(res.n_iters, n_iter) == calls[0]
    assert bundle_entropy.fg_evaluations(res.n_iters, n_iter, res.finished) == calls[0]
    if ranks == [0, 0, 0]:
        assert calls[0] == 2                      # linear energies: every sample finishes at t = 1, nIters = 0
    if any(r + 1 >= n_iter for r in ranks):
        assert calls[0] == n_iter                 # a sample that never finishes: every iteration evaluates fg


# ------------------------------------------------------------------------------------------------ GPU


def _assert_close(got, ref, tol, what=""):
    scale = max(np.abs(ref).max(), 1e-3)
    err = np.max(np.abs(got - ref))
    print("%s max err %.3e of scale %.3e" % (what, err, scale))
    assert err <= tol * scale, (what, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("which,B", [("bibtex", 77), ("bibtex", 4096), ("halfcheetah_bn", 1), ("halfcheetah_bn", 257),
                                     ("small3", 130)])
def test_fc_moving_context_matches_float64(which, B):
    spec = {"bibtex": picnn.bibtex_spec(), "halfcheetah_bn": _bn_halfcheetah(),
            "small3": picnn.FCSpec(45, 11, (70, 33, 18))}[which]
    params, x = _fc_problem(spec, B, 4)
    model = picnn.FCModel(spec, params)
    stats = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 9)
    model.set_bn_stats(stats)
    ctx = model.context(torch.from_numpy(x), bn="moving").cpu().numpy()
    ref, _ = bn_ref.fc_context64(spec, params, x, stats)
    _assert_close(ctx, ref, 2e-5, "%s B=%d" % (which, B))
    # inference mode writes nothing
    after = model.get_bn_stats()
    assert all(np.array_equal(after[k], stats[k]) for k in stats)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["init", "spread"])
@pytest.mark.parametrize("B", [3, 33, 256])
def test_conv_moving_context_matches_float64_and_feeds_fg(regime, B):
    from oracle import picnn_conv_oracle as co
    spec = picnn.ConvSpec()
    params = picnn.init_conv_params(spec, 2, regime)
    x = np.random.RandomState(52).rand(B, spec.H, spec.W, 1).astype(np.float32)
    model = picnn.ConvModel(spec, params)
    stats = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 8)
    model.set_bn_stats(stats)
    ctx_d = model.context(torch.from_numpy(x), bn="moving")
    ctx = ctx_d.cpu().numpy()
    ref, _ = bn_ref.conv_context64(spec, params, x, stats)
    o = 0
    for name, w in bn_ref.conv_heads(spec):
        _assert_close(ctx[:, o:o + w], ref[:, o:o + w], 2e-5, "%s B=%d %s" % (regime, B, name))
        o += w
    y = 0.05 + 0.9 * np.random.RandomState(4).rand(B, spec.n_labels)
    f, g = model.fg(ctx_d, torch.from_numpy(y).cuda())
    f_ref, g_ref = co.energy_and_grad_chain(params, ctx, y, spec.H, spec.W)
    assert np.array_equal(f.cpu().numpy(), f_ref) and np.array_equal(g.cpu().numpy(), g_ref)


@pytest.mark.gpu
def test_moving_mode_rows_are_independent_bit_for_bit():
    spec = picnn.bibtex_spec()
    params, x = _fc_problem(spec, 77, 5)
    model = picnn.FCModel(spec, params)
    model.set_bn_stats(bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 1))
    full = model.context(torch.from_numpy(x), bn="moving").cpu().numpy()
    for j in (0, 33, 76):
        one = model.context(torch.from_numpy(x[j:j + 1]), bn="moving").cpu().numpy()
        assert np.array_equal(one[0], full[j]), j
    cspec = picnn.ConvSpec()
    cmodel = picnn.ConvModel(cspec, picnn.init_conv_params(cspec, 3, "spread"))
    cmodel.set_bn_stats(bn_ref.random_bn_stats(picnn.init_bn_stats(cspec), 2))
    xc = np.random.RandomState(7).rand(33, cspec.H, cspec.W, 1).astype(np.float32)
    full = cmodel.context(torch.from_numpy(xc), bn="moving").cpu().numpy()
    for j in (0, 20, 32):
        one = cmodel.context(torch.from_numpy(xc[j:j + 1]), bn="moving").cpu().numpy()
        assert np.array_equal(one[0], full[j]), j


def _assert_stats(got, exp, tol, what):
    for k in exp:
        err = np.max(np.abs(got[k] - exp[k]))
        scale = np.abs(exp[k]).max()
        print("%s %s: max err %.3e of %.3e" % (what, k, err, scale))
        assert err <= tol * scale, (what, k, err, scale)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("which,B", [("bibtex", 128), ("conv", 70), ("conv", 256)])
def test_batch_mode_folds(which, k, B):
    if which == "bibtex":
        spec = picnn.bibtex_spec()
        params, x = _fc_problem(spec, B, 6)
        model = picnn.FCModel(spec, params)
        _, bstats = bn_ref.fc_context64(spec, params, x)
    else:
        spec = picnn.ConvSpec()
        params = picnn.init_conv_params(spec, 4, "spread")
        x = np.random.RandomState(54).rand(B, spec.H, spec.W, 1).astype(np.float32)
        model = picnn.ConvModel(spec, params)
        _, bstats = bn_ref.conv_context64(spec, params, x)
    start = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 3)
    model.set_bn_stats(start)
    plain = model.context(torch.from_numpy(x)).cpu().numpy()
    assert all(np.array_equal(v, start[k2]) for k2, v in model.get_bn_stats().items())
    folded = model.context(torch.from_numpy(x), bn_updates=k).cpu().numpy()
    assert np.array_equal(folded, plain)
    _assert_stats(model.get_bn_stats(), bn_ref.fold32(start, bstats, k), 1e-6, "%s B=%d k=%d" % (which, B, k))


def _fc_small_feed(spec, seed):
    rng = np.random.RandomState(seed)
    params = picnn.init_params(spec, seed, "spread")
    for k in params:
        if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    counts = rng.randint(1, 5, size=6)
    x = rng.rand(6, spec.n_features).astype(np.float32)
    return params, x, counts, rng


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fc", "conv"])
def test_surrogate_grad_folds_the_feed_row_statistics(which):
    from icnn_amd import train
    if which == "fc":
        spec = picnn.FCSpec(20, 12, (24, 12), batchnorm=True)
        params, x, counts, rng = _fc_small_feed(spec, 3)
        model = picnn.FCModel(spec, params)
    else:
        spec = picnn.ConvSpec()
        rng = np.random.RandomState(5)
        params = picnn.init_conv_params(spec, 5, "spread")
        counts = rng.randint(1, 5, size=6)
        x = rng.rand(6, spec.H, spec.W, 1).astype(np.float32)
        model = picnn.ConvModel(spec, params)
    samp = np.repeat(np.arange(6), counts)
    R = len(samp)
    y, v, c = rng.rand(R, spec.n_labels), rng.randn(R, spec.n_labels), rng.randn(R)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32))
    start = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 4)
    model.set_bn_stats(start)
    F0, F1 = (torch.empty(R, dtype=torch.float32, device="cuda") for _ in range(2))
    g0 = train.surrogate_grad(model, torch.from_numpy(x), (y, v, c), row_offset=off, F_rows=F0)
    g0 = {k2: t.cpu().numpy().copy() for k2, t in g0.items()}
    assert all(np.array_equal(val, start[k2]) for k2, val in model.get_bn_stats().items())
    g1 = train.surrogate_grad(model, torch.from_numpy(x), (y, v, c), row_offset=off, F_rows=F1, bn_updates=1)
    for k2 in g0:
        assert np.array_equal(g0[k2], g1[k2].cpu().numpy()), k2
    assert np.array_equal(F0.cpu().numpy(), F1.cpu().numpy())
    ctx64 = bn_ref.fc_context64 if which == "fc" else bn_ref.conv_context64
    _, rstats = ctx64(spec, params, x[samp])
    _assert_stats(model.get_bn_stats(), bn_ref.fold32(start, rstats, 1), 1e-5, "%s surrogate fold" % which)


@pytest.mark.gpu
def test_folds_and_moving_mode_replay_in_a_graph():
    """context(bn_updates=2) then context(bn="moving"), captured once and replayed twice: the same statistics and context
    bits as the same calls made eagerly from the same starting statistics."""
    spec = picnn.bibtex_spec()
    params, x = _fc_problem(spec, 128, 8)
    x2 = _fc_problem(spec, 40, 9)[1]
    model = picnn.FCModel(spec, params)
    start = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 5)
    xd, x2d = torch.from_numpy(x).cuda(), torch.from_numpy(x2).cuda()
    model.set_bn_stats(start)
    eager = []
    for _ in range(2):
        c1 = model.context(xd, bn_updates=2).cpu().numpy()
        c2 = model.context(x2d, bn="moving").cpu().numpy()
        eager.append((c1, c2, model.get_bn_stats()))
    model.set_bn_stats(start)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g1 = model.context(xd, bn_updates=2)
        g2 = model.context(x2d, bn="moving")
    assert all(np.array_equal(v, start[k]) for k, v in model.get_bn_stats().items())      # capture ran nothing
    for c1, c2, st in eager:
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(g1.cpu().numpy(), c1) and np.array_equal(g2.cpu().numpy(), c2)
        got = model.get_bn_stats()
        assert all(np.array_equal(got[k], st[k]) for k in st)
    assert not np.array_equal(eager[0][2]["u0/bn/moving_mean"], eager[1][2]["u0/bn/moving_mean"])


@pytest.mark.gpu
def test_completion_training_then_moving_mode_test_phase():
    """Two completion training iterations at batch 6 through the library with the reference's fold schedule (one fold per
    fg evaluation of the solve, one for train_step), then the test phase's interior-point solve on the moving-mode
    context against the oracle's solve_batch fed by the kernel-order conv PICNN on that context."""
    from gpu_util import result_to_host
    from test_gpu_parity import _assert_slice_parity, _slice_host
    from icnn_amd import train
    from oracle import picnn_conv_oracle as co
    spec = picnn.ConvSpec()
    params = picnn.init_conv_params(spec, 1, "spread")
    model = picnn.ConvModel(spec, params)
    host_stats = picnn.init_bn_stats(spec)
    rng = np.random.RandomState(21)
    mean_img = 0.2 + 0.6 * rng.rand(spec.n_labels)
    theta = {k: torch.from_numpy(np.array(v)).cuda() for k, v in params.items()}
    opt = train.TFAdam(theta, lr=1e-3)
    folds = []
    for it in range(2):
        x = rng.rand(6, spec.H, spec.W, 1).astype(np.float32)
        y_true = rng.rand(6, spec.n_labels)
        cur = {k: t.cpu().numpy().copy() for k, t in theta.items()}
        xd = torch.from_numpy(x).cuda()
        ctx = model.context(xd)
        res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=np.repeat(mean_img[None], 6, axis=0), nIter=5,
                                        variant="pdipm", native=True)
        k = res.fg_evaluations()
        model.context(xd, bn_updates=k)                            # the solve's folds: the same context, folded k times
        feed = bundle_entropy.implicit_feed(res, y_true, "mse")
        grads = train.surrogate_grad(model, xd, feed, bn_updates=1)
        samp = feed.sample.cpu().numpy()
        _, bstats = bn_ref.conv_context64(spec, cur, x)
        _, rstats = bn_ref.conv_context64(spec, cur, x[samp])
        host_stats = bn_ref.fold32(bn_ref.fold32(host_stats, bstats, k), rstats, 1)
        folds.append(k)
        opt.step(grads)
        new = picnn.project({kk: t.cpu().numpy().copy() for kk, t in theta.items()})
        for kk, t in theta.items():
            t.copy_(torch.from_numpy(new[kk]))
        model.repack(new)
    print("folds per iteration (solve + train_step):", [f + 1 for f in folds])
    _assert_stats(model.get_bn_stats(), host_stats, 1e-5, "after two iterations")
    # test phase, inference mode
    B, n_iter = 33, 5
    valX = rng.rand(B, spec.H, spec.W, 1).astype(np.float32)
    ctx = model.context(torch.from_numpy(valX), bn="moving")
    y0 = np.repeat(mean_img[None], B, axis=0)
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=y0.copy(), nIter=n_iter, variant="pdipm", native=True)
    host = result_to_host(res)
    assert (host["status"] == 0).all()
    ctx_rows = ctx.cpu().numpy()
    fg = co.make_fg_chain(model.params, ctx_rows, spec.H, spec.W)
    with np.errstate(all="ignore"):
        ora = oracle.solve_batch(fg, y0.copy(), n_iter, variant="pdipm")
    idx = np.arange(B)
    _assert_slice_parity(_slice_host(host, idx), ora, lambda rows: co.make_fg_chain(model.params, ctx_rows[rows], spec.H, spec.W),
                         y0, n_iter, 1e-6, "test phase pdipm", max_hard_frac=0.07, seeds=3, variant="pdipm")
    assert not np.array_equal(ctx_rows, model.context(torch.from_numpy(valX)).cpu().numpy())


@pytest.mark.gpu
def test_rl_act_with_batchnorm_at_one_observation():
    """act() of an agent with --icnn_bn: rl_adam.adam on the moving-mode context of ONE observation matches the host Adam
    oracle on that context (tests/test_adam.py's comparison)."""
    from icnn_amd import rl_adam
    from oracle import adam_oracle, picnn_oracle
    spec = dataclasses.replace(picnn.halfcheetah_spec(), action_box=False, batchnorm=True)
    params = picnn.init_params(spec, 11, "spread", yu_bias=1.0, gate_bias=1.0)
    model = picnn.FCModel(spec, params)
    stats = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 12)
    model.set_bn_stats(stats)
    obs = np.random.RandomState(111).randn(1, spec.n_features).astype(np.float32)
    ctx = model.context(torch.from_numpy(obs), bn="moving")
    ref, _ = bn_ref.fc_context64(spec, params, obs, stats)
    _assert_close(ctx.cpu().numpy(), ref, 2e-5, "act ctx")
    act = rl_adam.adam(model, ctx=ctx).cpu().numpy()
    chain = picnn_oracle.make_fg_chain(params, ctx.cpu().numpy(), list(spec.szs), spec.alpha, False)
    best, iters, _ = adam_oracle.adam(adam_oracle.entropy_fg(lambda o, a: chain(a)), ctx.cpu().numpy(), spec.n_labels, 1000)
    assert np.max(np.abs(act - best)) <= 1e-9
    # batch statistics of one row would collapse the u-path to beta: the moving-mode context differs from it
    assert not np.allclose(ctx.cpu().numpy(), model.context(torch.from_numpy(obs)).cpu().numpy())
    assert math.isfinite(float(np.abs(act).max()))
