"""The training kernels away from the shipped architectures: the FC surrogate gradient (icnn_be_fc_surrogate_grad) at every
depth the ABI takes, at widths and label counts on the GEMM tile edges and at the edges of the feed (empty samples, one
sample, split-K at its cap), the BatchNorm folds at a deep model, and the conv kernels (context, fg, training gradient,
solve) at image sizes other than 64 x 32.  References: the float64 statements tests/train_ref.py, tests/train_conv_ref.py
and tests/bn_ref.py, and the kernel-order oracle oracle/picnn_conv_chain.c."""
import ctypes as C

import numpy as np
import pytest
import torch

import bn_ref
import train_conv_ref
import train_ref
from gemm_ref import MAX_SPLITS, gemm_splits
from gpu_util import compare_with_oracle, result_to_host
from icnn_amd import picnn
from test_train_grad_conv import BN_TOL, MARGIN, ZERO_VARS

FC = picnn.FCSpec
# 8 z-layers (ICNN_BE_MAX_LAYERS): six batch-normalised u-layers chained, leaky z-layers
DEEP = FC(20, 12, (40, 36, 33, 30, 27, 24, 21), alpha=0.01, batchnorm=True)
CHAIN2 = FC(20, 12, (70, 33, 18), batchnorm=True)          # two chained batch-normalised u-layers
FC_CASES = {
    "L1_bn": FC(20, 12, (24,), batchnorm=True),               # one hidden layer: no BatchNorm layer, linear last u only
    "L1_leaky": FC(20, 12, (24,), alpha=0.01, batchnorm=False),
    "chain2_bn": CHAIN2,
    "deep8_bn_leaky": DEEP,
    "edges_n1": FC(9, 1, (15, 65), batchnorm=True),           # pq_ld = n + w at n = 1
    "edges_n5": FC(9, 5, (63, 17, 129), batchnorm=True),
    "edges_n17": FC(9, 17, (129, 15, 65, 17), alpha=0.01, batchnorm=False),
    "box_depth4": FC(20, 12, (30, 20, 16), alpha=0.01, batchnorm=True, action_box=True),
    "box_L1": FC(17, 6, (24,), alpha=0.01, batchnorm=False, action_box=True),
}
def _perturbed(params, rng):
    for k in params:                             # non-trivial BatchNorm parameters and biases
        if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
            params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
    return params


def _float32_restatement_error(spec, params, x_rows, y, v, c, g64):
    """Worst relative error over the variables of the same double backward in float32 on the CPU.  Batch-normalised
    channels that are active on one or two samples only have variances near 1e-6, and the BatchNorm backward scales by
    gamma / sqrt(var + 1e-5) there: chained over several layers, float32 arithmetic itself then misses float64 by 1e-3
    (measured at the deep model with five samples).  Such a problem says nothing about the kernels; the screen keeps
    problems on which plain float32 is ten times inside the kernels' bound.  (Without BatchNorm the error of this
    restatement is its own summation order over the rows, not the problem's: it is not used there.)"""
    theta = {k: torch.tensor(np.asarray(a, np.float32), requires_grad=True) for k, a in params.items()}
    yt = torch.tensor(np.asarray(y, np.float32), requires_grad=True)
    E, _ = train_ref.energy(spec, theta, torch.as_tensor(np.asarray(x_rows, np.float32)), yt)
    F = torch.as_tensor(np.asarray(c, np.float32)) * E
    if v is not None:
        dEdy, = torch.autograd.grad(E.sum(), yt, create_graph=True)
        F = F + (dEdy * torch.as_tensor(np.asarray(v, np.float32))).sum(dim=1)
    gs = torch.autograd.grad(F.sum(), list(theta.values()), allow_unused=True)
    worst = 0.0
    for (k, ref), g in zip(g64.items(), gs):
        got = np.zeros_like(ref) if g is None else g.detach().double().numpy()
        worst = max(worst, float(np.max(np.abs(got - ref))) / max(float(np.max(np.abs(ref))), 1e-30))
    return worst


def _fc_problem(spec, seed, with_v, counts=None):
    """Seeded model and feed as tests/test_train_grad.py's _small_problem (6 samples with 1-4 rows each, or the given
    row counts), screened so that no float64 pre-activation is within 1e-4 of zero and, with BatchNorm, that float32
    arithmetic itself is well-conditioned on the problem (_float32_restatement_error)."""
    for s in range(seed, seed + 200):
        rng = np.random.RandomState(s)
        params = _perturbed(picnn.init_params(spec, s, "spread"), rng)
        cnt = np.asarray(counts) if counts is not None else rng.randint(1, 5, size=6)
        x = rng.rand(len(cnt), spec.n_features).astype(np.float32)
        samp = np.repeat(np.arange(len(cnt)), cnt)
        R = len(samp)
        y = rng.rand(R, spec.n_labels)
        v = rng.randn(R, spec.n_labels) if with_v else None
        c = rng.randn(R)
        if train_ref.u_margin(spec, params, x[samp]) < 1e-4:
            continue
        g64, F64, margin = train_ref.surrogate_grad64(spec, params, x[samp], y, v, c)
        if margin < 1e-4 or (spec.batchnorm and _float32_restatement_error(spec, params, x[samp], y, v, c, g64) > 1e-5):
            continue
        return dict(params=params, x=x, samp=samp, counts=cnt, y=y, v=v, c=c, g64=g64, F64=F64)
    raise AssertionError("no screened seed")


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


def _fc_grad(model, p, x=None, counts=None, F_rows=None, **kw):
    from icnn_amd import train
    y = torch.from_numpy(p["y"]).cuda()
    v = torch.from_numpy(p["v"]).cuda() if p["v"] is not None else None
    c = torch.from_numpy(p["c"]).cuda()
    x = p["x"] if x is None else x
    off = _offsets(p["counts"] if counts is None else counts)
    return train.surrogate_grad(model, torch.from_numpy(x), (y, v, c), row_offset=off, F_rows=F_rows, **kw)


def _check_every_variable(g, p, what):
    """every variable to 1e-4 max|g64| + 1e-7 (test_small_every_variable_matches_float64_double_backward's bound); prints the
    worst relative error next to it"""
    assert list(g.keys()) == list(p["g64"].keys())
    worst, bad = (0.0, ""), []
    for k, ref in p["g64"].items():
        got = g[k].double().cpu().numpy()
        assert got.shape == ref.shape, k
        err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
        worst = max(worst, (err / max(scale, 1e-30), k))
        if not err <= 1e-4 * scale + 1e-7:
            bad.append((k, err, scale))
    print("%s: worst relative error %.2e (%s), bound 1e-4" % (what, worst[0], worst[1]))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ CPU


def test_architectures_are_in_the_abi_range():
    from icnn_amd import _lib
    assert DEEP.n_layers == _lib.MAX_LAYERS
    assert sum(1 for k in picnn.init_params(DEEP) if k.endswith("/bn/gamma")) == 6
    assert sum(1 for k in picnn.init_params(CHAIN2) if k.endswith("/bn/gamma")) == 2
    assert not any(k.endswith("/bn/gamma") for k in picnn.init_params(FC_CASES["L1_bn"]))


@pytest.mark.parametrize("name", sorted(FC_CASES))
def test_fc_architecture_sizes_agree_with_the_library(name):
    from icnn_amd import _lib, train
    from test_train_grad import _c_structs
    spec = FC_CASES[name]
    lib = _lib.load()
    m, c = _c_structs(spec)
    n = lib.icnn_be_fc_grad_floats(C.byref(m), C.byref(c))
    assert n == sum(int(np.prod(s)) for _, s in train.grad_layout(spec)) == sum(
        a.size for a in picnn.init_params(spec).values())
    assert lib.icnn_be_fc_surrogate_grad_work_floats(C.byref(m), C.byref(c), 7, 3000) > 0


def test_split_plan_restatement():
    # a large output needs no split, a one-tile output with a short K is not split below 64 per chunk
    assert gemm_splits(1024, 1024, 5000) == (1, 5008)
    assert gemm_splits(12, 24, 100) == (2, 64)
    # the longest weight-gradient product of the suite's FC tests (Bibtex, K = 2R = 1462) stays below the cap
    assert gemm_splits(159, 1, 1462)[0] == 23
    assert gemm_splits(3, 6, 5000) == (MAX_SPLITS, 160)         # test_fc_large_feed_split_k_at_the_cap: last chunk 40
    assert gemm_splits(3, 6, 2500) == (MAX_SPLITS, 80)           # the same feed without v: last chunk 20
    assert gemm_splits(3, 6, 5130) == (30, 176)                  # near the cap, not every K reaches it


# sizes conv_layout accepts besides 64 x 32: a square one with n = 1024, a non-square one with n = 3 * 1024
CONV_SIZES = [(32, 32), (48, 64)]


def _conv_structs(H, W):
    from icnn_amd import _lib
    m = _lib.ConvModel()
    m.H, m.W = H, W
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        m.filters[l], m.ksize[l], m.stride[l] = nf, k, s
    m.fc_hidden, m.ctx_width, m.wpack = picnn.CONV_FCS[0], picnn.ConvSpec(H, W).ctx_width, 64
    m.work, m.work_batch = 64, 8
    c = _lib.ConvCtx()
    for i in range(7):
        c.w_stage[i] = c.b_stage[i] = 64
    for i in range(4):
        c.bn_gamma[i] = c.bn_beta[i] = 64
    c.bn_eps = 1e-5
    return m, c


@pytest.mark.parametrize("H,W", CONV_SIZES + [(16, 64), (64, 64), (64, 32)])
def test_conv_sizes_accepted(H, W):
    from icnn_amd import _lib, train
    lib = _lib.load()
    spec = picnn.ConvSpec(H, W)
    m, c = _conv_structs(H, W)
    assert lib.icnn_be_conv_pack_floats(C.byref(m)) > 0
    assert lib.icnn_be_conv_work_floats(C.byref(m), 8) > 0
    assert lib.icnn_be_conv_context_work_floats(C.byref(m), 8) > 0
    assert lib.icnn_be_conv_surrogate_grad_work_floats(C.byref(m), C.byref(c), 8, 20) > 0
    assert lib.icnn_be_conv_grad_floats(C.byref(m), C.byref(c)) == sum(
        int(np.prod(s)) for _, s in train.grad_layout(spec)) == sum(
        a.size for a in picnn.init_conv_params(spec).values())
    model = picnn.ConvModel(spec, picnn.init_conv_params(spec, 1, "spread"), device="cpu")
    assert model.wpack.numel() == lib.icnn_be_conv_pack_floats(C.byref(m))


def test_fixture_size_16x8_is_refused_before_launch():
    """16 x 8 (the CPU fixture's size) breaks the implicit-GEMM mapping (positions in multiples of 16): every size query
    says 0, every entry point ICNN_BE_ELIMIT with placeholder pointers (nothing is launched), ConvModel raises."""
    from icnn_amd import _lib
    lib = _lib.load()
    m, c = _conv_structs(16, 8)
    fake = C.c_void_p(64)
    assert lib.icnn_be_conv_pack_floats(C.byref(m)) == 0
    assert lib.icnn_be_conv_work_floats(C.byref(m), 4) == 0
    assert lib.icnn_be_conv_grad_floats(C.byref(m), C.byref(c)) == 0
    assert lib.icnn_be_conv_surrogate_grad_work_floats(C.byref(m), C.byref(c), 4, 8) == 0
    assert lib.icnn_be_conv_context_work_floats(C.byref(m), 4) == 0
    assert lib.icnn_be_conv_fg(C.byref(m), fake, fake, 4, fake, fake, None, None) == -2
    assert lib.icnn_be_conv_context(C.byref(m), C.byref(c), fake, 4, fake, fake, None) == -2
    assert lib.icnn_be_conv_surrogate_grad(C.byref(m), C.byref(c), fake, 4, fake, 8, fake, fake, fake, fake, None, fake,
                                           None) == -2
    spec = picnn.ConvSpec(16, 8)
    with pytest.raises(ValueError):
        picnn.ConvModel(spec, picnn.init_conv_params(spec), device="cpu")


# ------------------------------------------------------------------------------------------------ GPU: FC


@pytest.mark.gpu
@pytest.mark.parametrize("with_v", [True, False], ids=["v", "no_v"])
@pytest.mark.parametrize("name", list(FC_CASES))
def test_fc_every_variable_against_float64(name, with_v):
    spec = FC_CASES[name]
    p = _fc_problem(spec, 100, with_v)
    model = picnn.FCModel(spec, p["params"], "cuda")
    F = torch.empty(len(p["samp"]), dtype=torch.float32, device="cuda")
    g = _fc_grad(model, p, F_rows=F)
    torch.cuda.synchronize()
    _check_every_variable(g, p, "%s %s R=%d" % (name, "v" if with_v else "no v", len(p["samp"])))
    assert np.max(np.abs(F.double().cpu().numpy() - p["F64"])) <= 1e-5 * np.max(np.abs(p["F64"]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["chain2_bn", "deep8_bn_leaky"])
def test_fc_empty_samples(name):
    """Samples with no feed row (first, middle, last): they carry weight 0 in the BatchNorm statistics and no gradient, so
    the result is the float64 gradient on the gathered rows, and the gradient of the same feed without those samples."""
    spec = FC_CASES[name]
    counts = np.array([0, 3, 2, 1, 0, 4, 2, 0])
    p = _fc_problem(spec, 300, True, counts=counts)
    model = picnn.FCModel(spec, p["params"], "cuda")
    F = torch.empty(len(p["samp"]), dtype=torch.float32, device="cuda")
    g = _fc_grad(model, p, F_rows=F)
    keep = counts > 0
    g_kept = _fc_grad(model, p, x=p["x"][keep], counts=counts[keep])
    torch.cuda.synchronize()
    _check_every_variable(g, p, "%s with empty samples" % name)
    assert np.max(np.abs(F.double().cpu().numpy() - p["F64"])) <= 1e-5 * np.max(np.abs(p["F64"]))
    for k in g:
        a, b = g[k].double(), g_kept[k].double()
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), k


@pytest.mark.gpu
@pytest.mark.parametrize("with_v", [True, False], ids=["v", "no_v"])
def test_fc_one_sample(with_v):
    # BatchNorm off: over one sample's rows the batch variance is 0, and the u-path gradient is float32 rounding amplified by
    # 1/sqrt(eps) -- no tolerance would mean anything there
    spec = FC(20, 12, (70, 33, 18), batchnorm=False)
    p = _fc_problem(spec, 400, with_v, counts=[5])
    model = picnn.FCModel(spec, p["params"], "cuda")
    g = _fc_grad(model, p)
    torch.cuda.synchronize()
    _check_every_variable(g, p, "B = 1, %s" % ("v" if with_v else "no v"))


@pytest.mark.gpu
def test_fc_large_feed_split_k_at_the_cap():
    """A few thousand rows on a small model: the weight-gradient products (y*yu)^T abar have a one-tile output and
    K = 2R, which gemm_splits cuts into its 32 splits with a short last chunk."""
    spec = FC(8, 3, (6,), alpha=0.01, batchnorm=False)
    counts = 45 + (np.arange(40) * 13) % 35
    counts[-1] += 2500 - counts.sum()
    R = 2500
    K = 2 * R
    splits, kchunk = gemm_splits(spec.n_labels, spec.szs[0], K)
    # 5000 = 31 chunks of 160 + 40; not every K near here reaches the cap (5130 gives 30 chunks of 176)
    assert splits == MAX_SPLITS and K % kchunk != 0, (R, splits, kchunk)
    p = _fc_problem(spec, 500, True, counts=counts)
    assert len(p["samp"]) == R
    model = picnn.FCModel(spec, p["params"], "cuda")
    F = torch.empty(R, dtype=torch.float32, device="cuda")
    g = _fc_grad(model, p, F_rows=F)
    torch.cuda.synchronize()
    _check_every_variable(g, p, "R=%d, K=%d in %d splits of %d (last %d)" % (R, K, splits, kchunk, K - (splits - 1) * kchunk))
    assert np.max(np.abs(F.double().cpu().numpy() - p["F64"])) <= 1e-5 * np.max(np.abs(p["F64"]))


@pytest.mark.gpu
def test_fc_deep_bitwise_repeatable():
    p = _fc_problem(DEEP, 600, True)
    model = picnn.FCModel(DEEP, p["params"], "cuda")
    a = _fc_grad(model, p, flat=True).clone()
    b = _fc_grad(model, p, flat=True).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3])
def test_fc_deep_surrogate_grad_folds_every_layer(k):
    """bn_updates = k at six batch-normalised layers: every layer's moving mean and variance are the weighted feed-row
    statistics folded k times (tolerance of test_surrogate_grad_folds_the_feed_row_statistics), the gradient unchanged."""
    p = _fc_problem(DEEP, 700, True)
    model = picnn.FCModel(DEEP, p["params"], "cuda")
    start = bn_ref.random_bn_stats(picnn.init_bn_stats(DEEP), 4)
    model.set_bn_stats(start)
    g0 = {n: t.cpu().numpy().copy() for n, t in _fc_grad(model, p).items()}
    assert all(np.array_equal(val, start[n]) for n, val in model.get_bn_stats().items())
    g1 = _fc_grad(model, p, bn_updates=k)
    for n in g0:
        assert np.array_equal(g0[n], g1[n].cpu().numpy()), n
    _, rstats = bn_ref.fc_context64(DEEP, p["params"], p["x"][p["samp"]])
    assert sorted(rstats) == list(range(6))
    got = model.get_bn_stats()
    exp = bn_ref.fold32(start, rstats, k)
    for name in exp:
        err = np.max(np.abs(got[name] - exp[name]))
        scale = np.abs(exp[name]).max()
        print("deep k=%d %s: max err %.3e of %.3e" % (k, name, err, scale))
        assert err <= 1e-5 * scale, (name, err, scale)


# ------------------------------------------------------------------------------------------------ GPU: conv


def _conv_problem(spec, regime, seed, with_v, B=6):
    """tests/test_train_grad_conv.py's _small_problem at another image size: seeded model and feed (B samples with 1-4
    rows each), screened so that no float64 pre-activation is within MARGIN of zero."""
    for s in range(seed, seed + 300):
        rng = np.random.RandomState(s)
        params = _perturbed(picnn.init_conv_params(spec, s, regime), rng)
        counts = rng.randint(1, 5, size=B)
        x = rng.rand(B, spec.H, spec.W, 1).astype(np.float32)
        samp = np.repeat(np.arange(B), counts)
        R = len(samp)
        y = rng.rand(R, spec.n_labels)
        v = rng.randn(R, spec.n_labels) if with_v else None
        c = rng.randn(R)
        if train_conv_ref.u_margin(spec, params, x[samp]) < MARGIN:
            continue
        g64, F64, margin = train_conv_ref.surrogate_grad64(spec, params, x[samp], y, v, c)
        if margin < MARGIN:
            continue
        return dict(params=params, x=x, samp=samp, counts=counts, y=y, v=v, c=c, g64=g64, F64=F64)
    raise AssertionError("no screened seed")


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", CONV_SIZES)
def test_conv_context_and_fg_at_other_sizes(H, W):
    """Context against oracle/picnn_conv_oracle.context (2e-4, test_conv_energy_and_gradient's bound); E and dE/dy bit for
    bit against the kernel-order oracle on that context (test_conv_energy_and_gradient_bit_exact_vs_kernel_order_oracle)."""
    from oracle import picnn_conv_oracle as co
    spec = picnn.ConvSpec(H, W)
    B = 9
    params = picnn.init_conv_params(spec, 2, "spread")
    x = np.random.RandomState(52).rand(B, H, W, 1).astype(np.float32)
    model = picnn.ConvModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    ref = co.flat_context(co.context(params, torch.from_numpy(x)))
    assert ctx.shape == ref.shape == (B, spec.ctx_width)
    err = float(np.max(np.abs(ctx.cpu().numpy() - ref)))
    print("%d x %d: context max err %.2e, bound 2e-4 * %.2e" % (H, W, err, max(1.0, np.abs(ref).max())))
    assert err <= 2e-4 * max(1.0, np.abs(ref).max())
    y = 0.05 + 0.9 * np.random.RandomState(4).rand(B, spec.n_labels)
    f, g = model.fg(ctx, torch.from_numpy(y).cuda())
    f_ref, g_ref = co.energy_and_grad_chain(params, ctx.cpu().numpy(), y, H, W)
    assert np.array_equal(f.cpu().numpy(), f_ref), np.abs(f.cpu().numpy() - f_ref).max()
    assert np.array_equal(g.cpu().numpy(), g_ref), np.abs(g.cpu().numpy() - g_ref).max()


@pytest.mark.gpu
@pytest.mark.parametrize("with_v", [True, False], ids=["v", "no_v"])
@pytest.mark.parametrize("H,W", CONV_SIZES)
def test_conv_every_variable_at_other_sizes(H, W, with_v):
    """test_every_variable_against_float64 at another image size: BN_TOL for the u-path, 1e-4 elsewhere, exact zeros for
    the variables F does not reach."""
    from icnn_amd import train
    spec = picnn.ConvSpec(H, W)
    p = _conv_problem(spec, "spread", 21, with_v)
    model = picnn.ConvModel(spec, p["params"])
    R = len(p["samp"])
    F = torch.empty(R, dtype=torch.float32, device="cuda")
    x = torch.from_numpy(p["x"]).cuda()
    off = torch.from_numpy(_offsets(p["counts"])).cuda()
    y, c = torch.from_numpy(p["y"]).cuda(), torch.from_numpy(p["c"]).cuda()
    rows = (y, torch.from_numpy(p["v"]).cuda(), c) if with_v else (y, c)
    g = train.surrogate_grad(model, x, rows, row_offset=off, F_rows=F)
    torch.cuda.synchronize()
    assert list(g.keys()) == list(p["params"].keys())
    bad, worst = [], (0.0, "")
    for name, ref in p["g64"].items():
        got = g[name].double().cpu().numpy().reshape(ref.shape)
        if name in ZERO_VARS:
            if not (np.all(got == 0) and np.all(ref == 0)):
                bad.append(name)
            continue
        scale = np.max(np.abs(ref))
        err = np.max(np.abs(got - ref))
        tol = BN_TOL if name.startswith("u") else 1e-4
        worst = max(worst, (err / scale if scale > 0 else np.inf, name))
        if not (scale > 0 and err <= tol * scale):
            bad.append((name, err / scale if scale > 0 else err))
    print("%d x %d %s R=%d: worst relative error %.2e (%s), bounds 1e-4 / %.0e (u-path)"
          % (H, W, "v" if with_v else "no v", R, worst[0], worst[1], BN_TOL))
    assert not bad, bad
    F64 = p["F64"]
    assert np.max(np.abs(F.double().cpu().numpy() - F64)) <= 1e-4 * np.max(np.abs(F64))


@pytest.mark.gpu
@pytest.mark.parametrize("H,W", CONV_SIZES)
def test_conv_fused_solve_at_other_sizes(H, W):
    """One small fused solve against the oracle solver fed by the kernel-order PICNN: identical active sets and iteration
    counts, y* within 1e-7 (test_fused_conv_completion_matches_oracle)."""
    from icnn_amd import bundle_entropy
    from oracle import bundle_entropy_oracle as oracle
    from oracle import picnn_conv_oracle as co
    spec = picnn.ConvSpec(H, W)
    B, n_iter = 8, 5
    params = picnn.init_conv_params(spec, 1, "spread")
    x = np.random.RandomState(51).rand(B, H, W, 1).astype(np.float32)
    model = picnn.ConvModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    y0 = np.repeat((0.2 + 0.6 * np.random.RandomState(9).rand(spec.n_labels))[None], B, axis=0)
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=y0.copy(), nIter=n_iter, native=True)
    fg = co.make_fg_chain(params, ctx.cpu().numpy(), H, W)
    with np.errstate(all="ignore"):
        ora = oracle.solve_batch(fg, y0.copy(), n_iter)
    host = result_to_host(res)
    dy, discrete = compare_with_oracle(host, ora)
    print("%d x %d fused B=%d nIter=%d vs kernel-order oracle: max|dy| = %.3e, %d discrete differences, cuts %s"
          % (H, W, B, n_iter, dy.max(), len(discrete), np.bincount([len(a) for a in host["active"]])))
    assert (host["status"] == 0).all()
    assert dy.max() <= 1e-7 and not discrete, (dy.max(), discrete)
