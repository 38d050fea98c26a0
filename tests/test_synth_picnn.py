"""The PICNN of synthetic-cls/icnn.py (picnn.FCSpec.relu_last_u, picnn.synthetic_spec) and the fused back-optimisation
training step of the FC PICNNs (icnn_be_gd_feed, train.GDTrainer): spec, host context, the script read literally and the C
ABI on the CPU; on the device the context, energy / gradient bit for bit against the MFMA-order oracle, the surrogate
gradient against a float64 double-backward (tests/synth_picnn_ref.py), the feed kernel against its torch composition, the
trainer against the hand-composed step and against float64 autograd through the unroll, its capture and its convergence."""
import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import synth_picnn_ref as ref
from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S1 = picnn.FCSpec(2, 1, (24, 16), batchnorm=False, relu_last_u=True)         # the synthetic layout shrunk
S2 = picnn.FCSpec(20, 12, (24, 12), batchnorm=True, relu_last_u=True)        # the project's small BatchNorm spec + the flag
S3 = picnn.FCSpec(12, 5, (16,), batchnorm=False, relu_last_u=True)           # L = 1: the only u-layer is the last
SMALL = {"S1": S1, "S2": S2, "S3": S3}
FC_CTX_BYTES = 312            # sizeof(icnn_be_fc_ctx) at the parent commit: 12 ints, a float, 4 bytes of padding, 4 x 8 pointers
ULP32 = 2.0 ** -23


def _off(spec):
    import dataclasses
    return dataclasses.replace(spec, relu_last_u=False)


_problems = {}


def _problem(name, with_v=True):
    key = (name, with_v)
    if key not in _problems:
        _problems[key] = ref.small_problem(SMALL[name], 0, with_v)
    return _problems[key]


_batches = {}


def _batch(name, B):
    key = (name, B)
    if key not in _batches:
        spec = picnn.synthetic_spec() if name == "synthetic" else SMALL[name]
        # the full spec has 600 x B x-only pre-activations: the flag conditions are screened, the margin is not needed
        # where the comparison is bit for bit on the device's own context
        _batches[key] = ref.batch_problem(spec, 0, B, margin=0.0 if name == "synthetic" else ref.MARGIN)
    return _batches[key]


# ------------------------------------------------------------------------------------------------ CPU


def test_spec_flag_defaults_and_synthetic_spec():
    assert picnn.FCSpec(2, 1, (200, 200)).relu_last_u is False
    assert picnn.bibtex_spec().relu_last_u is False and picnn.halfcheetah_spec().relu_last_u is False
    s = picnn.synthetic_spec()
    assert s == picnn.FCSpec(2, 1, (200, 200), batchnorm=False, relu_last_u=True)
    assert s.relu_last_u is True and s.batchnorm is False and s.alpha == 0.0 and not s.action_box
    assert picnn.bn_layers(S2) == picnn.bn_layers(_off(S2)) == [(0, 24)]
    from icnn_amd import train
    for spec in (S1, S2, S3):
        a, b = picnn.init_params(spec, 3, "spread"), picnn.init_params(_off(spec), 3, "spread")
        assert list(a) == list(b) and all(np.array_equal(a[k], b[k]) for k in a)
        assert train.grad_layout(spec) == train.grad_layout(_off(spec))


def test_make_convex_divisor():
    spec = picnn.synthetic_spec()
    rng = np.random.RandomState(0)
    p0 = {k: (v * np.where(rng.rand(*v.shape) < 0.5, -1, 1)).astype(np.float32) for k, v in picnn.init_params(spec, 0).items()}
    today = {k: (np.abs(v) if "proj" in k and k.endswith("/W") else v) for k, v in p0.items()}
    got = picnn.make_convex({k: v.copy() for k, v in p0.items()})
    assert all(got[k].dtype == np.float32 and np.array_equal(got[k], today[k]) for k in p0)
    got = picnn.make_convex({k: v.copy() for k, v in p0.items()}, divisor=10)
    n_proj = 0
    for k, v in p0.items():
        if "proj" in k and k.endswith("/W"):
            n_proj += 1
            assert got[k].dtype == np.float32 and np.array_equal(got[k], np.abs(v) / np.float32(10)), k
            assert (v < 0).any()
        else:
            assert np.array_equal(got[k], v), k
    assert n_proj == 2


@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_host_context_relus_the_last_u_layer(name):
    spec = SMALL[name]
    _, params, x = _batch(name, 33)
    xt = torch.from_numpy(x)
    on = picnn.context(spec, params, xt)
    assert torch.equal(on, ref.context_by_hand(spec, params, xt, True))
    off = picnn.context(_off(spec), params, xt)
    assert torch.equal(off, ref.context_by_hand(spec, params, xt, False))
    L = len(spec.szs)
    first = spec.ctx_offsets[L][0]                 # stage L's columns start at its yu
    assert torch.equal(on[:, :first], off[:, :first])
    assert not torch.equal(on[:, first:], off[:, first:])
    assert on.shape == (33, spec.ctx_width)


def test_synthetic_spec_is_the_script_as_written():
    """f_picnn's loop taken literally against context + y-path for picnn.synthetic_spec(), float64, E and dE/dy"""
    spec = picnn.synthetic_spec()
    params = picnn.make_convex(picnn.init_params(spec, 5, "spread"), divisor=10)
    rng = np.random.RandomState(5)
    for k in params:
        if k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    x = torch.as_tensor(rng.randn(16, 2))
    y1 = torch.tensor(rng.rand(16, 1), requires_grad=True)
    y2 = y1.detach().clone().requires_grad_(True)
    E1 = ref.f_picnn_literal(params, x, y1)
    E2 = ref.context_y_path64(spec, params, ref.context64(spec, params, x), y2)
    g1, = torch.autograd.grad(E1.sum(), y1)
    g2, = torch.autograd.grad(E2.sum(), y2)
    assert float((E1 - E2).abs().max()) <= 1e-12 * float(E1.abs().max())
    assert float((g1 - g2).abs().max()) <= 1e-12 * float(g1.abs().max())
    assert float(g1.abs().max()) > 0
    # and the flag is what makes them agree: with a linear last u-layer the energies differ
    E3 = ref.context_y_path64(_off(spec), params, ref.context64(_off(spec), params, x), y2)
    assert float((E1 - E3).abs().max()) > 1e-6 * float(E1.abs().max())


def test_abi_struct_size_version_and_exports():
    from icnn_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.FcCtx) == lib.icnn_be_struct_size(2) == FC_CTX_BYTES
    assert _lib.FcCtx.u_last_relu.offset == _lib.FcCtx.bn_eps.offset + 4 and _lib.FcCtx.u_last_relu.size == 4
    assert _lib.FcCtx.w_stage.offset == _lib.FcCtx.u_last_relu.offset + 4
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    assert re.search(r"\bint u_last_relu;", header)
    for name in ("icnn_be_gd_feed", "icnn_be_gd_feed_work_bytes"):
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)


def test_gd_feed_rejects_bad_arguments_before_launch():
    from icnn_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(64)
    names = ["yK", "t", "coef", "v", "c", "off", "loss", "tallies", "work"]

    def call(B=4, n=3, K=5, **null):
        p = {k: (None if null.get(k) else fake) for k in names}
        return lib.icnn_be_gd_feed(p["yK"], p["t"], p["coef"], B, n, K, 0.25, p["v"], p["c"], p["off"], p["loss"],
                                   p["tallies"], p["work"], None)
    for bad in (0, -1):
        assert call(B=bad) == -1 and call(n=bad) == -1 and call(K=bad) == -1
    for k in names:
        if k != "tallies":
            assert call(**{k: True}) == -1, k
    assert call(B=1 << 20, K=1 << 12) == -2             # B K beyond int
    assert lib.icnn_be_gd_feed_work_bytes(100) >= 8 * 100 + 4
    assert lib.icnn_be_gd_feed_work_bytes(400) > lib.icnn_be_gd_feed_work_bytes(100)
    assert lib.icnn_be_gd_feed_work_bytes(-1) == 0


def _c_structs(spec):
    from icnn_amd import _lib
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = spec.alpha, int(spec.action_box), spec.ctx_width
    m.wpack = 64
    c = _lib.FcCtx()
    c.n_features, c.n, c.n_layers = spec.n_features, spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        c.width[i] = w
        c.w_stage[i] = c.b_stage[i] = c.bn_gamma[i] = c.bn_beta[i] = 64
    c.batchnorm, c.bn_eps = int(spec.batchnorm), 1e-5
    return m, c


def test_adam_fc_obs_refuses_the_flag():
    """The one entry that takes an icnn_be_fc_ctx and cannot honour the flag (its in-kernel context producer keeps the last
    u-layer linear).  Placeholder pointers, nothing launched: a context WITH BatchNorm is what the entry answers ELIMIT to
    today, on the host and after every argument check -- so with the flag off that answer must still come, and with the
    flag on EINVAL comes first."""
    from icnn_amd import _lib
    lib = _lib.load()
    spec = picnn.FCSpec(17, 6, (200, 200), alpha=0.01, batchnorm=True)
    m, c = _c_structs(spec)
    fake = C.c_void_p(64)

    def call(batch=1):
        return lib.icnn_be_adam_fc_obs(C.byref(m), C.byref(c), fake, batch, 5, fake, fake, fake, fake, None)
    assert c.u_last_relu == 0
    assert call() == -2
    c.u_last_relu = 1
    assert call() == -1
    assert call(batch=0) == -1                          # before the empty batch's early return as well
    c.u_last_relu = 0
    assert call() == -2


def test_gd_trainer_serves_fc_models_only():
    from icnn_amd import ficnn, train
    for cls in (picnn.ConvModel, ficnn.FICNNModel):
        with pytest.raises(TypeError):
            train.GDTrainer(cls, 8)


# ------------------------------------------------------------------------------------------------ GPU


def _close_ctx(got, want):
    got, want = got.double().cpu().numpy(), want.double().cpu().numpy()
    err, bound = float(np.max(np.abs(got - want))), 1e-5 * max(1.0, float(np.max(np.abs(want))))
    print("max|ctx - ref| = %.3e (bound %.3e)" % (err, bound))
    assert err <= bound, (err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_device_context_against_host_mirror(name):
    spec = SMALL[name]
    _, params, x = _batch(name, 33)
    model = picnn.FCModel(spec, params, "cuda")
    xt = torch.from_numpy(x)
    got = model.context(xt)
    torch.cuda.synchronize()
    _close_ctx(got, picnn.context(spec, params, xt))
    L = len(spec.szs)
    off = picnn.FCModel(_off(spec), params, "cuda").context(xt)
    first = spec.ctx_offsets[L][0]
    assert torch.equal(got[:, :first], off[:, :first]) and not torch.equal(got[:, first:], off[:, first:])
    # the staged entry points share the stage launcher
    _close_ctx(model.context_sharded(xt), picnn.context(spec, params, xt))


@pytest.mark.gpu
def test_device_context_moving_mode():
    spec = S2
    _, params, x = _batch("S2", 33)
    model = picnn.FCModel(spec, params, "cuda")
    xt = torch.from_numpy(x)
    folded = model.context(xt, bn_updates=1)
    _close_ctx(folded, picnn.context(spec, params, xt))
    stats = model.get_bn_stats()
    assert np.abs(stats["u0/bn/moving_mean"]).max() > 0
    got = model.context(xt[:5], bn="moving")
    torch.cuda.synchronize()
    _close_ctx(got, picnn.context(spec, params, xt[:5], bn_stats=stats))


@pytest.mark.gpu
def test_flag_off_is_bit_unchanged():
    from icnn_amd import train
    implicit = picnn.FCSpec(20, 12, (24, 12))
    explicit = picnn.FCSpec(20, 12, (24, 12), relu_last_u=False)
    rng = np.random.RandomState(0)
    params = ref.perturbed_params(implicit, 0, rng)
    x = torch.from_numpy(rng.rand(6, 20).astype(np.float32))
    counts = np.array([1, 4, 2, 3, 1, 2])
    R = int(counts.sum())
    rows = (torch.from_numpy(rng.rand(R, 12)).cuda(), torch.from_numpy(rng.randn(R, 12)).cuda(),
            torch.from_numpy(rng.randn(R)).cuda())
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    out = []
    for spec in (implicit, explicit, implicit):
        model = picnn.FCModel(spec, params, "cuda")
        assert model.c_ctx.u_last_relu == 0
        out.append((model.context(x).clone(), train.surrogate_grad(model, x, rows, row_offset=off, flat=True).clone()))
    torch.cuda.synchronize()
    for ctx, g in out[1:]:
        assert torch.equal(ctx, out[0][0]) and torch.equal(g, out[0][1])
    assert float(out[0][1].abs().max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", [("S1", 3), ("S1", 40), ("synthetic", 100)])
def test_fg_bit_exact_against_chain_oracle(name, B):
    from oracle import picnn_oracle
    spec = picnn.synthetic_spec() if name == "synthetic" else SMALL[name]
    _, params, x = _batch(name, B)
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(x))
    y = np.random.RandomState(B).rand(B, spec.n_labels)
    f, g = model.fg(ctx, torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    E_ref, g_ref = picnn_oracle.energy_and_grad_chain(params, ctx.cpu().numpy(), y, list(spec.szs), spec.alpha)
    assert np.array_equal(f.cpu().numpy(), E_ref) and np.array_equal(g.cpu().numpy(), g_ref)
    assert np.abs(g_ref).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("with_v", [True, False])
@pytest.mark.parametrize("name", ["S1", "S2", "S3"])
def test_surrogate_grad_every_variable_matches_float64_double_backward(name, with_v):
    from icnn_amd import train
    spec = SMALL[name]
    p = _problem(name, with_v)
    x = torch.from_numpy(p["x"])
    off = np.concatenate([[0], np.cumsum(p["counts"])]).astype(np.int32)
    R = len(p["samp"])
    rows = (torch.from_numpy(p["y"]).cuda(), torch.from_numpy(p["v"]).cuda() if with_v else None,
            torch.from_numpy(p["c"]).cuda())
    model = picnn.FCModel(spec, p["params"], "cuda")
    F = torch.empty(R, dtype=torch.float32, device="cuda")
    g = train.surrogate_grad(model, x, rows, row_offset=off, F_rows=F)
    g_off = train.surrogate_grad(picnn.FCModel(_off(spec), p["params"], "cuda"), x, rows, row_offset=off)
    torch.cuda.synchronize()
    assert list(g.keys()) == list(p["params"].keys())
    for k, want in p["g64"].items():
        got = g[k].double().cpu().numpy()
        assert got.shape == want.shape, k
        err, scale = float(np.max(np.abs(got - want))), float(np.max(np.abs(want)))
        print("%-14s err %.3e scale %.3e" % (k, err, scale))
        assert err <= 1e-4 * scale + 1e-7, (k, err, scale)
    Fd = F.double().cpu().numpy()
    assert np.max(np.abs(Fd - p["F64"])) <= 1e-5 * np.max(np.abs(p["F64"]))
    last = "u%d/W" % (len(spec.szs) - 1)
    assert float(g[last].abs().max()) > 0
    assert not torch.equal(g[last], g_off[last])                 # the mask is in the backward


FEED_SHAPES = [(6, 1, 5), (7, 12, 5), (100, 1, 30)]


def _feed_inputs(B, n, K):
    rng = np.random.RandomState(B + n + K)
    yK = torch.from_numpy(rng.rand(B, n).astype(np.float32).astype(np.float64)).cuda()
    yK.view(-1)[0] = 0.5                                          # the threshold itself predicts 1
    t = torch.from_numpy((rng.rand(B, n) < 0.4).astype(np.float32)).cuda()
    from icnn_amd import train
    coef = train.unrolled_coefficients(K, 0.01, 0.9, torch.device("cuda"))
    return yK, t, coef


def _run_feed(yK, t, coef, K, tallies=True):
    from icnn_amd import _lib
    lib = _lib.load()
    B, n = yK.shape
    dev = yK.device
    out = dict(v=torch.full((B * K, n), -7.0, dtype=torch.float64, device=dev),
               c=torch.full((B * K,), -7.0, dtype=torch.float64, device=dev),
               off=torch.full((B + 1,), -7, dtype=torch.int32, device=dev),
               loss=torch.full((), -7.0, dtype=torch.float32, device=dev),
               tallies=torch.full((B, 3), -7, dtype=torch.int32, device=dev) if tallies else None)
    work = torch.zeros((int(lib.icnn_be_gd_feed_work_bytes(B)) + 7) // 8, dtype=torch.float64, device=dev)
    scale = float(np.float32(1) / np.float32(B * n))

    def call():
        _lib.check(lib.icnn_be_gd_feed(yK.data_ptr(), t.data_ptr(), coef.data_ptr(), B, n, K, scale, out["v"].data_ptr(),
                                       out["c"].data_ptr(), out["off"].data_ptr(), out["loss"].data_ptr(),
                                       None if out["tallies"] is None else out["tallies"].data_ptr(), work.data_ptr(),
                                       C.c_void_p(torch.cuda.current_stream().cuda_stream)), "icnn_be_gd_feed")
        torch.cuda.synchronize()
        return {k: (None if v is None else v.clone()) for k, v in out.items()}
    return call, scale


def _loss_within_one_ulp(loss, yK, t):
    d = (yK.to(torch.float32) - t).cpu().numpy()
    want = np.float32(np.mean(d.astype(np.float64) ** 2))
    got = np.float32(loss.item())
    print("loss %.9e, float32 of the float64 mean %.9e" % (got, want))
    assert abs(float(got) - float(want)) <= ULP32 * abs(float(want)), (got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("B,n,K", FEED_SHAPES)
def test_feed_kernel_against_torch_composition(B, n, K):
    yK, t, coef = _feed_inputs(B, n, K)
    call, scale = _run_feed(yK, t, coef, K)
    a = call()
    b = call()                                                    # the ticket re-armed itself: same bits
    d = yK.to(torch.float32) - t
    ybar = (d * 2.0) * scale
    assert ybar.dtype == torch.float32
    v = (coef * ybar.to(torch.float64).reshape(B, 1, n)).reshape(B * K, n)
    assert torch.equal(a["v"], v) and float(v.abs().max()) > 0
    assert torch.equal(a["c"], torch.zeros(B * K, dtype=torch.float64, device="cuda"))
    assert torch.equal(a["off"], torch.arange(0, (B + 1) * K, K, dtype=torch.int32, device="cuda"))
    _loss_within_one_ulp(a["loss"], yK, t)
    yh, th = yK.cpu().numpy(), t.cpu().numpy()
    pred, truth = yh >= 0.5, th.astype(np.int64) != 0
    want = np.stack([(pred & truth).sum(1), (pred & ~truth).sum(1), (~pred & truth).sum(1)], axis=1)
    assert np.array_equal(a["tallies"].cpu().numpy(), want) and want.sum() > 0
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c2 = _run_feed(yK, t, coef, K, tallies=False)[0]()            # without tallies: the same rows and loss
    assert torch.equal(c2["v"], a["v"]) and torch.equal(c2["loss"], a["loss"])


def _composed_step(model, opt, x, t, K, lr, mu, bn_updates):
    """the hand-composed step: context, gd.solve, the torch elementwise ops, unrolled_grad, DeviceAdam.step"""
    from icnn_amd import gd, train
    B, n = t.shape
    ctx = model.context(x)
    yK, traj, _ = gd.solve(model, ctx, 0.5, K, lr, mu, trajectory=True)
    d = yK.to(torch.float32) - t
    loss = torch.mean(d * d)
    ybar = (d * 2.0) * float(np.float32(1.0) / np.float32(B * n))
    grad = train.unrolled_grad(model, x, traj, ybar.to(torch.float64), lr, mu, bn_updates=bn_updates, flat=True)
    opt.step(grad)
    return loss, grad, yK


@pytest.mark.gpu
@pytest.mark.parametrize("name,bn_updates", [("S2", 1), ("S1", 0)])
def test_trainer_step_equals_hand_composed_step(name, bn_updates):
    from icnn_amd import train
    spec = SMALL[name]
    B, K, lr, mu = 6, 5, 0.1, 0.3
    _, params, x = _batch(name, B)
    rng = np.random.RandomState(1)
    xs = torch.from_numpy(x).cuda()
    ts = torch.from_numpy((rng.rand(B, spec.n_labels) < 0.4).astype(np.float32)).cuda()
    tr = train.GDTrainer(picnn.FCModel(spec, {k: v.copy() for k, v in params.items()}, "cuda"), B, n_iter=K, lr=lr,
                         momentum=mu, bn_updates=bn_updates, f1=True)
    other = picnn.FCModel(spec, {k: v.copy() for k, v in params.items()}, "cuda")
    opt = train.DeviceAdam(other)
    loss = tr.step(xs, ts)
    loss2, grad2, yK2 = _composed_step(other, opt, xs, ts, K, lr, mu, bn_updates)
    torch.cuda.synchronize()
    assert loss is tr.loss and loss.dtype == torch.float32
    assert torch.equal(tr.y, yK2)
    assert torch.equal(tr.grad, grad2) and float(grad2.abs().max()) > 0
    for a, b in ((tr.opt.theta, opt.theta), (tr.opt.m, opt.m), (tr.opt.v, opt.v), (tr.opt.arena, opt.arena)):
        assert torch.equal(a, b)
    for k, v in tr.model.bn_stats.items():
        assert torch.equal(v, other.bn_stats[k]), k
        assert bn_updates == 0 or float(v.abs().max()) > 0
    _loss_within_one_ulp(loss, tr.y, ts)
    # torch's float32 mean of the float32 squares: each square within 2^-24, a sum of B n terms within (B n - 1) 2^-24
    assert abs(float(loss.item()) - float(loss2.item())) <= (B * spec.n_labels + 1) * 2.0 ** -24 * float(loss2.item())
    assert tr.t_steps == 1 and 0.0 <= tr.macro_f1() <= 1.0
    hp = tr.host_params()
    assert list(hp) == list(params) and any(not np.array_equal(hp[k], params[k]) for k in hp)


def _unroll_problem(name, B, K, lr, mu, margin):
    """screened on the CPU: x-only margins, the flag conditions, and the float64 trajectory's z-path margin"""
    spec = picnn.synthetic_spec() if name == "synthetic" else SMALL[name]
    seed = 0
    for _ in range(400):
        seed, params, x = ref.batch_problem(spec, seed, B, margin)
        rng = np.random.RandomState(seed + 7)
        t = (rng.rand(B, spec.n_labels) < 0.4).astype(np.float32)
        _, _, _, m = ref.unrolled_autograd(spec, params, x, np.full(t.shape, 0.5), t, K, lr, mu)
        if m >= margin:
            return spec, params, x, t
        seed += 1
    raise AssertionError("no screened seed")


# The full spec has 8 x 30 x 400 z-path pre-activations along the trajectory; none of them within 1e-4 of zero would need
# thousands of seeds.  What has to hold is that the float32 sign of each equals the float64 one: the device's
# pre-activations are sums of at most 201 float32 products of magnitude <= 4, off by less than 201 x 4 x 2^-24 = 5e-5 in
# the worst case and ~1e-6 typically, so the full spec screens at 1e-5 and checks the margin at the DEVICE trajectory too, and every case checks the gate signs
# of the DEVICE context against the float64 ones.
UNROLL_CASES = [("S1", 6, 5, 0.1, 0.3, ref.MARGIN), ("S3", 6, 5, 0.1, 0.3, ref.MARGIN), ("synthetic", 8, 30, 0.01, 0.9, 1e-5)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,K,lr,mu,margin", UNROLL_CASES, ids=[c[0] for c in UNROLL_CASES])
def test_trainer_gradient_against_float64_autograd_through_the_unroll(name, B, K, lr, mu, margin):
    from icnn_amd import gd, train
    spec, params, x, t = _unroll_problem(name, B, K, lr, mu, margin)
    model = picnn.FCModel(spec, {k: v.copy() for k, v in params.items()}, "cuda")
    xs = torch.from_numpy(x).cuda()
    ctx = model.context(xs)
    traj = gd.solve(model, ctx, 0.5, K, lr, mu, trajectory=True)[1].cpu().numpy()
    # the x-only masks the device took, where the context shows them: every gate column is positive exactly where the
    # float64 gate pre-activation is
    with torch.no_grad():
        gates = ref.energy(spec, {k: torch.as_tensor(np.asarray(p, np.float64)) for k, p in params.items()},
                           torch.as_tensor(x.astype(np.float64)), torch.full(t.shape, 0.5, dtype=torch.float64))[2]
    ctx = ctx.cpu().numpy()
    for i, g64 in enumerate(gates, start=1):
        at, w = spec.ctx_offsets[i][2], spec.widths[i - 1]
        assert g64.shape[1] == w and np.array_equal(ctx[:, at:at + w] > 0, g64.numpy() > 0), i
    tr = train.GDTrainer(model, B, n_iter=K, lr=lr, momentum=mu)
    tr.step(xs, torch.from_numpy(t).cuda())
    torch.cuda.synchronize()
    g64, yK, _, m = ref.unrolled_autograd(spec, params, x, np.full(t.shape, 0.5), t, K, lr, mu, mask_traj=traj)
    print("min |z pre-activation| at the device trajectory %.2e" % m)
    assert m >= 0.5 * margin
    assert np.abs(yK - tr.y.cpu().numpy()).max() <= 1e-5 * max(1.0, float(np.abs(yK).max()))
    got = {k: v.double().cpu().numpy() for k, v in train.unpack_grad(spec, tr.grad).items()}
    nonzero = 0
    for k, want in g64.items():
        err, scale = float(np.max(np.abs(got[k] - want))), float(np.max(np.abs(want)))
        print("%-14s err %.3e scale %.3e" % (k, err, scale))
        assert err <= 1e-4 * scale + 1e-12, (k, err, scale)        # tests/test_gd.py's bound for its unrolled check
        nonzero += scale > 0
    assert nonzero > len(g64) // 2
    assert float(np.abs(g64["u%d/W" % (len(spec.szs) - 1)]).max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,K", [("S2", 6, 5), ("synthetic", 100, 30)])
def test_captured_step_replays_as_eager_steps(name, B, K):
    from icnn_amd import train
    spec = picnn.synthetic_spec() if name == "synthetic" else SMALL[name]
    _, params, x = _batch(name, B)
    rng = np.random.RandomState(2)
    xs = torch.from_numpy(x).cuda()
    ts = torch.from_numpy((rng.rand(B, spec.n_labels) < 0.4).astype(np.float32)).cuda()
    x2 = torch.from_numpy(rng.rand(B, spec.n_features).astype(np.float32)).cuda()
    t2 = 1.0 - ts
    bn = 1 if spec.batchnorm else 0

    def trainer():
        return train.GDTrainer(picnn.FCModel(spec, {k: v.copy() for k, v in params.items()}, "cuda"), B, n_iter=K,
                               bn_updates=bn)
    a, b = trainer(), trainer()
    la = [a.step(xs, ts).clone() for _ in range(3)]
    la.append(a.step(x2, t2).clone())
    b.x.copy_(xs)
    b.t.copy_(ts)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loss = b.step()
    torch.cuda.current_stream().wait_stream(s)
    lb = []
    for _ in range(3):
        graph.replay()
        lb.append(loss.clone())
    torch.cuda.synchronize()
    assert b.t_steps == 3
    lb.append(b.step(x2, t2).clone())                              # eager, on the captured trainer: copies into b.x, b.t
    graph.replay()                                                 # the captured step after step(x2, t2): the new batch
    lb.append(loss.clone())
    la.append(a.step().clone())
    torch.cuda.synchronize()
    assert torch.equal(b.x, x2) and torch.equal(b.t, t2)
    assert len(la) == len(lb) == 5 and all(torch.equal(p, q) for p, q in zip(la, lb)), (la, lb)
    assert not torch.equal(la[2], la[3])                           # the new batch was read
    assert torch.equal(a.opt.theta, b.opt.theta) and torch.equal(a.opt.arena, b.opt.arena)
    for k, v in a.model.bn_stats.items():
        assert torch.equal(v, b.model.bn_stats[k]), k
    assert a.t_steps == b.t_steps == 5


def _example():
    spec = importlib.util.spec_from_file_location("synthetic_cls_example", os.path.join(REPO, "examples", "synthetic_cls.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.gpu
def test_loss_decreases_on_moons():
    """data, step count and criterion of tests/test_ficnn_train.py::test_loss_decreases_on_moons, through the example's
    --model picnn branch"""
    from icnn_amd import train
    ex = _example()
    x, t = ref.moons(100, 2)
    tr = ex.make_trainer("picnn", "sum", 100, 2)
    assert isinstance(tr, train.GDTrainer) and tr.spec == picnn.synthetic_spec()
    xs, ts = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    first = float(tr.step(xs, ts).item())
    for _ in range(99):
        last = tr.step()
    last = float(last.item())
    print("loss %.5e -> %.5e" % (first, last))
    assert last < first, (first, last)
    hp = tr.host_params()
    assert all((hp[k] >= 0).all() for k in hp if "proj" in k and k.endswith("/W"))
