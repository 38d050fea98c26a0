"""The back-optimisation training step and test phase of the completion model (completion/icnn.back.py:131-165, 210-254;
DESIGN.md §17): the feed kernel icnn_be_gd_feed_px against its NumPy restatement (tests/conv_gd_ref.py) and against
icnn_be_gd_feed, train.ConvGDTrainer against the hand-composed step, its capture, the shipped size and evaluate()."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import conv_gd_ref as ref
from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP32 = 2.0 ** -23
SMALL = picnn.ConvSpec(32, 32)
LR, MU, PX = 0.01, 0.9, 255.0


# ------------------------------------------------------------------------------------------------ CPU


def test_px_feed_is_exported_and_declared():
    from icnn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()
    for name in ("icnn_be_gd_feed_px", "icnn_be_gd_feed_px_work_bytes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_px_feed_rejects_bad_arguments_before_launch():
    from icnn_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(64)
    names = ["yK", "t", "coef", "v", "c", "off", "loss", "work"]

    def call(B=4, n=3, K=5, **null):
        p = {k: (None if null.get(k) else fake) for k in names}
        return lib.icnn_be_gd_feed_px(p["yK"], p["t"], p["coef"], B, n, K, 0.25, 255.0, p["v"], p["c"], p["off"], p["loss"],
                                      p["work"], None)
    for bad in (0, -1):
        assert call(B=bad) == -1 and call(n=bad) == -1 and call(K=bad) == -1
        # the loss-only form checks its sizes as well
        assert call(B=bad, v=True, c=True, off=True, coef=True) == -1
    for k in ("yK", "t", "loss", "work"):
        assert call(**{k: True}) == -1, k
        assert call(v=True, c=True, off=True, coef=True, **{k: True}) == -1, k
    for one in ("v", "c", "off"):                         # one of the three row pointers NULL, then two of them
        assert call(**{one: True}) == -1, one
        two = {k: True for k in ("v", "c", "off") if k != one}
        assert call(**two) == -1, two
    assert call(coef=True) == -1                          # rows without coefficients
    assert call(B=1 << 20, K=1 << 12) == -2               # B K beyond int
    assert call(B=1 << 20, K=1 << 12, v=True, c=True, off=True, coef=True) == -2
    assert call(B=1 << 20, K=1 << 12, yK=True) == -1      # EINVAL first
    assert lib.icnn_be_gd_feed_px_work_bytes(70, 2048, 30) >= 8 * 70 + 4
    assert lib.icnn_be_gd_feed_px_work_bytes(400, 7, 4) > lib.icnn_be_gd_feed_px_work_bytes(100, 7, 4)
    for bad in ((0, 3, 5), (4, 0, 5), (4, 3, 0), (-1, 3, 5)):
        assert lib.icnn_be_gd_feed_px_work_bytes(*bad) == 0


def test_conv_gd_trainer_serves_conv_models_only():
    from icnn_amd import ficnn, train
    for cls in (picnn.FCModel, ficnn.FICNNModel):
        with pytest.raises(TypeError):
            train.ConvGDTrainer(cls, 8)
    with pytest.raises(TypeError):
        train.ConvGDTrainer(None, 8)


def test_conv_gd_trainer_rejects_bad_sizes():
    """every size is checked before anything touches a device: a ConvModel held on the host serves"""
    from icnn_amd import train
    model = picnn.ConvModel(SMALL, picnn.init_conv_params(SMALL, 0, "spread"), "cpu")
    for kw in (dict(batch=0), dict(batch=-3), dict(batch=2, n_iter=0), dict(batch=2, bn_updates=-1),
               dict(batch=2, eval_batch=0), dict(batch=2, eval_batch=-1)):
        with pytest.raises(ValueError):
            train.ConvGDTrainer(model, **kw)


def test_reference_ybar_against_float64():
    """guards tests/conv_gd_ref.py itself: four float32 roundings, each within 2^-24 relative, against 2 px^2 d / (B n) from
    the same float32 d"""
    rng = np.random.RandomState(0)
    B, n = 5, 333
    yK = rng.rand(B, n).astype(np.float32).astype(np.float64)
    t = rng.rand(B, n).astype(np.float32)
    scale = np.float32(1.0) / np.float32(B * n)
    for px in (255.0, 1.0):
        u, ybar = ref.ybar32(yK, t, scale, px)
        d = (yK.astype(np.float32) - t).astype(np.float64)
        want = 2.0 * px * px * d / (B * n)
        assert np.all(np.abs(ybar - want) <= 1e-6 * np.abs(want))
        assert np.abs(want).max() > 0
        assert np.all(np.abs(u - px * d) <= 2.0 ** -24 * np.abs(px * d))      # 255 d rounded once; exact for px = 1
    v, c, off, loss = ref.feed(yK, t, [0.5, -2.0], scale, 255.0)
    assert v.shape == (B * 2, n) and np.array_equal(v[1], -2.0 * ref.ybar32(yK, t, scale, 255.0)[1][0].astype(np.float64))
    assert np.array_equal(off, [0, 2, 4, 6, 8, 10]) and not c.any()
    assert abs(loss - np.mean((255.0 * (yK - t)) ** 2)) <= 1e-6 * loss


# ------------------------------------------------------------------------------------------------ GPU

FEED_SHAPES = [(2, 7, 4), (3, 1024, 9), (5, 2048, 30)]
GUARD = 3                     # rows, and row_offset entries, behind the ones the kernel owns


def _feed_inputs(B, n, K):
    from icnn_amd import train
    rng = np.random.RandomState(B + n + K)
    yK = torch.from_numpy(rng.rand(B, n).astype(np.float32).astype(np.float64)).cuda()
    t = torch.from_numpy(rng.rand(B, n).astype(np.float32)).cuda()
    coef = train.unrolled_coefficients(K, LR, MU, torch.device("cuda"))
    return yK, t, coef


def _run_px(yK, t, coef, K, px, rows=True):
    """one call of icnn_be_gd_feed_px into guard-filled buffers; returns a closure that calls again and clones"""
    from icnn_amd import _lib
    lib = _lib.load()
    B, n = yK.shape
    dev = yK.device
    out = dict(v=torch.full((B * K + GUARD, n), -7.0, dtype=torch.float64, device=dev),
               c=torch.full((B * K + GUARD,), -7.0, dtype=torch.float64, device=dev),
               off=torch.full((B + 1 + GUARD,), -7, dtype=torch.int32, device=dev),
               loss=torch.full((), -7.0, dtype=torch.float32, device=dev))
    work = torch.zeros((int(lib.icnn_be_gd_feed_px_work_bytes(B, n, K)) + 7) // 8, dtype=torch.float64, device=dev)
    scale = float(np.float32(1) / np.float32(B * n))

    def call():
        ptr = [out[k].data_ptr() if rows else None for k in ("v", "c", "off")]
        _lib.check(lib.icnn_be_gd_feed_px(yK.data_ptr(), t.data_ptr(), coef.data_ptr() if rows else None, B, n, K, scale, px,
                                          ptr[0], ptr[1], ptr[2], out["loss"].data_ptr(), work.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream().cuda_stream)), "icnn_be_gd_feed_px")
        torch.cuda.synchronize()
        return {k: v.clone() for k, v in out.items()}
    return call, scale


def _within_one_ulp(loss, want64):
    got, want = float(np.float32(loss.item())), float(np.float32(want64))
    print("loss %.9e, float32 of the float64 mean %.9e" % (got, want))
    assert want > 0 and abs(got - want) <= ULP32 * abs(want), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("px", [255.0, 1.0])
@pytest.mark.parametrize("B,n,K", FEED_SHAPES)
def test_px_feed_against_numpy_restatement(B, n, K, px):
    yK, t, coef = _feed_inputs(B, n, K)
    call, scale = _run_px(yK, t, coef, K, px)
    a = call()
    b = call()                                                    # the ticket re-armed itself: same bits
    v, c, off, loss = ref.feed(yK.cpu().numpy(), t.cpu().numpy(), coef.cpu().numpy(), scale, px)
    R = B * K
    assert np.array_equal(a["v"][:R].cpu().numpy(), v) and np.abs(v).max() > 0
    assert np.array_equal(a["c"][:R].cpu().numpy(), c)
    assert np.array_equal(a["off"][:B + 1].cpu().numpy(), off)
    assert bool((a["v"][R:] == -7.0).all()) and bool((a["c"][R:] == -7.0).all()) and bool((a["off"][B + 1:] == -7).all())
    _within_one_ulp(a["loss"], loss)
    for k in a:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,K", [(3, 1024, 9), (4, 159, 30)])
def test_px_one_equals_gd_feed_bit_for_bit(B, n, K):
    from icnn_amd import _lib
    lib = _lib.load()
    yK, t, coef = _feed_inputs(B, n, K)
    call, scale = _run_px(yK, t, coef, K, 1.0)
    a = call()
    old = dict(v=torch.full((B * K, n), -7.0, dtype=torch.float64, device="cuda"),
               c=torch.full((B * K,), -7.0, dtype=torch.float64, device="cuda"),
               off=torch.full((B + 1,), -7, dtype=torch.int32, device="cuda"),
               loss=torch.full((), -7.0, dtype=torch.float32, device="cuda"))
    work = torch.zeros((int(lib.icnn_be_gd_feed_work_bytes(B)) + 7) // 8, dtype=torch.float64, device="cuda")
    _lib.check(lib.icnn_be_gd_feed(yK.data_ptr(), t.data_ptr(), coef.data_ptr(), B, n, K, scale, old["v"].data_ptr(),
                                   old["c"].data_ptr(), old["off"].data_ptr(), old["loss"].data_ptr(), None, work.data_ptr(),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream)), "icnn_be_gd_feed")
    torch.cuda.synchronize()
    assert torch.equal(a["v"][:B * K], old["v"]) and float(old["v"].abs().max()) > 0
    assert torch.equal(a["c"][:B * K], old["c"])
    assert torch.equal(a["off"][:B + 1], old["off"])
    assert torch.equal(a["loss"], old["loss"]) and float(old["loss"].item()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,K", [(3, 1024, 9), (5, 2048, 30)])
def test_px_feed_loss_only_mode(B, n, K):
    yK, t, coef = _feed_inputs(B, n, K)
    full = _run_px(yK, t, coef, K, PX)[0]()
    call = _run_px(yK, t, coef, K, PX, rows=False)[0]
    a = call()
    b = call()
    assert torch.equal(a["loss"], full["loss"]) and torch.equal(b["loss"], full["loss"])
    assert float(full["loss"].item()) > 0
    for k in ("v", "c", "off"):                                   # nothing but the loss is written
        assert bool((a[k] == -7).all()), k


def _problem(spec, B, seed):
    rng = np.random.RandomState(seed)
    params = picnn.init_conv_params(spec, seed, "spread")
    y0 = 0.2 + 0.6 * rng.rand(spec.n_labels)                      # meanY-like start, an [n] row

    def batch():
        return (torch.from_numpy(rng.rand(B, spec.H, spec.W, 1).astype(np.float32)).cuda(),
                torch.from_numpy(rng.rand(B, spec.n_labels).astype(np.float32)).cuda())
    return params, y0, batch


def _model(spec, params):
    return picnn.ConvModel(spec, {k: v.copy() for k, v in params.items()}, "cuda")


def _ybar_torch(yK, t, px):
    """the contract's float32 operations as torch elementwise launches"""
    d = yK.to(torch.float32) - t
    u = px * d
    ybar = ((u * 2.0) * float(np.float32(1.0) / np.float32(t.numel()))) * px
    assert ybar.dtype == torch.float32
    return u, ybar


def _composed_step(model, opt, x, t, y0, K, bn_updates):
    """the hand-composed step: context, gd.solve, the torch elementwise ops, unrolled_grad, DeviceAdam.step"""
    from icnn_amd import gd, train
    ctx = model.context(x)
    yK, traj, _ = gd.solve(model, ctx, y0, K, LR, MU, trajectory=True)
    _, ybar = _ybar_torch(yK, t, PX)
    grad = train.unrolled_grad(model, x, traj, ybar.to(torch.float64), LR, MU, bn_updates=bn_updates, flat=True)
    opt.step(grad)
    return grad, yK


def _same_state(a, b, model_a, model_b):
    for p, q in ((a.theta, b.theta), (a.m, b.m), (a.v, b.v), (a.arena, b.arena)):
        assert torch.equal(p, q)
    for k, v in model_a.bn_stats.items():
        assert torch.equal(v, model_b.bn_stats[k]), k
    assert a.t == b.t


@pytest.mark.gpu
@pytest.mark.parametrize("bn_updates", [0, 1])
def test_step_equals_hand_composed_step(bn_updates):
    from icnn_amd import train
    B, K = 6, 4
    params, y0, batch = _problem(SMALL, B, 3)
    tr = train.ConvGDTrainer(_model(SMALL, params), B, n_iter=K, lr=LR, momentum=MU, y0=y0, bn_updates=bn_updates)
    other = _model(SMALL, params)
    opt = train.DeviceAdam(other)
    y0d = torch.from_numpy(y0).cuda()
    for step in range(2):
        x, t = batch()
        loss = tr.step(x, t if step == 0 else t.view(B, SMALL.H, SMALL.W, 1))      # targets as images too
        grad2, yK2 = _composed_step(other, opt, x, t, y0d, K, bn_updates)
        torch.cuda.synchronize()
        assert loss is tr.loss and loss.dtype == torch.float32
        assert torch.equal(tr.y, yK2)
        assert torch.equal(tr.grad, grad2) and float(grad2.abs().max()) > 0
        _same_state(tr.opt, opt, tr.model, other)
        _within_one_ulp(loss, ref.loss64(_ybar_torch(tr.y, t, PX)[0].cpu().numpy()))
    for v in tr.model.bn_stats.values():
        assert bn_updates == 0 or float(v.abs().max()) > 0
    assert tr.t_steps == 2
    hp = tr.host_params()
    assert list(hp) == list(params) and any(not np.array_equal(hp[k], params[k]) for k in hp)
    assert list(tr.params()) == list(params)


def _capture(fn):
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = fn()
    torch.cuda.current_stream().wait_stream(s)
    return graph, out


@pytest.mark.gpu
def test_captured_step_and_evaluate_replay_as_eager_ones():
    from icnn_amd import train
    B, K = 6, 4
    params, y0, batch = _problem(SMALL, B, 4)
    x, t = batch()

    def trainer():
        return train.ConvGDTrainer(_model(SMALL, params), B, n_iter=K, lr=LR, momentum=MU, y0=y0, bn_updates=1, eval_batch=B)
    a, b = trainer(), trainer()
    la = [a.step(x, t).clone() for _ in range(3)]
    b.x.copy_(x)
    b.t.copy_(t.view(b.t.shape))
    graph, loss = _capture(b.step)
    lb = []
    for _ in range(3):
        graph.replay()
        lb.append(loss.clone())
    torch.cuda.synchronize()
    assert a.t_steps == b.t_steps == 3
    assert all(torch.equal(p, q) for p, q in zip(la, lb)), (la, lb)
    assert not torch.equal(la[0], la[1])                          # the weights moved between replays
    assert torch.equal(a.y, b.y)
    _same_state(a.opt, b.opt, a.model, b.model)
    # evaluate: nothing changes between replays, so each replay gives the eager call's bits
    ea = a.evaluate(x, t).clone()
    ya = a.y_eval.clone()
    b.x_eval.copy_(x)
    b.t_eval.copy_(t)
    graph_e, eloss = _capture(b.evaluate)
    for _ in range(3):
        graph_e.replay()
        torch.cuda.synchronize()
        assert torch.equal(eloss, ea) and torch.equal(b.y_eval, ya)
    assert float(ea.item()) > 0
    _same_state(a.opt, b.opt, a.model, b.model)


@pytest.mark.gpu
def test_shipped_size_step_once():
    """ConvSpec(), batch 70, nGdIter 30: the gradient is unrolled_grad's on the trainer's own trajectory and ybar (whose float64
    bound tests/test_gd_conv.py holds), the loss the float64 mean within one float32 ulp"""
    from icnn_amd import train
    spec = picnn.ConvSpec()
    B, K = 70, 30
    params, y0, batch = _problem(spec, B, 0)
    x, t = batch()
    tr = train.ConvGDTrainer(_model(spec, params), B, n_iter=K, lr=LR, momentum=MU, y0=y0)
    loss = tr.step(x, t)
    u, ybar = _ybar_torch(tr.y, t, PX)
    twin = _model(spec, params)                                   # the weights of before the update
    grad = train.unrolled_grad(twin, x, tr.traj, ybar.to(torch.float64), LR, MU, flat=True)
    torch.cuda.synchronize()
    assert tr.traj.shape == (B, K, spec.n_labels)
    assert torch.equal(tr.grad, grad) and float(grad.abs().max()) > 0
    _within_one_ulp(loss, ref.loss64(u.cpu().numpy()))
    assert torch.equal(tr.row_offset, torch.arange(0, (B + 1) * K, K, dtype=torch.int32, device="cuda"))


@pytest.mark.gpu
def test_evaluate_is_the_moving_statistics_test_phase_and_changes_nothing():
    from icnn_amd import gd, train
    B, E, K = 6, 5, 4
    params, y0, batch = _problem(SMALL, B, 5)
    (x1, t1), (x2, t2) = batch(), batch()
    xe, te = (v[:E].contiguous() for v in batch())

    def trainer():
        return train.ConvGDTrainer(_model(SMALL, params), B, n_iter=K, lr=LR, momentum=MU, y0=y0, bn_updates=1, eval_batch=E)
    a, b = trainer(), trainer()
    a.step(x1, t1)
    b.step(x1, t1)
    torch.cuda.synchronize()
    before = [v.clone() for v in (a.opt.theta, a.opt.m, a.opt.v, a.opt.arena)] + [v.clone() for v in a.model.bn_stats.values()]
    eloss = a.evaluate(xe, te.view(E, SMALL.H, SMALL.W, 1))
    ctx = a.model.context(xe, bn="moving")
    y = gd.solve(a.model, ctx, torch.from_numpy(y0).cuda(), K, LR, MU)[0]
    torch.cuda.synchronize()
    assert eloss is a.eval_loss and eloss.dtype == torch.float32
    assert a.y_eval.shape == (E, SMALL.n_labels) and torch.equal(a.y_eval, y)
    _within_one_ulp(eloss, ref.loss64(_ybar_torch(y, te, PX)[0].cpu().numpy()))
    after = [a.opt.theta, a.opt.m, a.opt.v, a.opt.arena] + list(a.model.bn_stats.values())
    assert all(torch.equal(p, q) for p, q in zip(before, after)) and a.t_steps == 1
    # the moving statistics are what it read: the batch-statistics context of the same images differs
    assert not torch.equal(ctx, a.model.context(xe))
    la, lb = a.step(x2, t2), b.step(x2, t2)
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(a.y, b.y) and torch.equal(a.grad, b.grad)
    _same_state(a.opt, b.opt, a.model, b.model)
    with pytest.raises(ValueError):
        train.ConvGDTrainer(_model(SMALL, params), B, n_iter=K).evaluate(xe, te)
