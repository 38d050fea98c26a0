"""Solver comparison on the device (icnn_amd.pgd, be_pgd.hip): projected gradient descent on E - H(y), the objective's traces
and the bundle's lower bound.  CPU: the exports, the C entries' argument checks, the restated gradient against autograd and
the bound against the oracle's solves of the float64 quadratic.  GPU: the FC loop against the restatement around the
MFMA-order oracle (only the float64 logarithms can differ), the bits of a sample across batches and under graph replay, the
objective, the trace of a fused solve against the scripts' callback, the bound, and the order-independent certificate
objective >= bound.  The conv model's cases are in test_pgd_conv.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import pgd_ref
import problems
import train_ref
from icnn_amd import picnn
from pgd_ref import HI, LO, ULP

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_pgd_workspace_bytes", "icnn_be_fc_pgd", "icnn_be_conv_pgd", "icnn_be_entropy_objective",
               "icnn_be_bundle_trace", "icnn_be_dual_bound"]
LRS = (0.1, 0.01, 0.001)                 # the scripts' learning rates (ebundle-vs-gd.py:119)
# The certificate's margin: the cuts carry float32 energies.  Measured on the CPU: the largest |E32 - E64| of the oracle's
# float32 chain (picnn_oracle.energy_and_grad_chain) against its float64 energy (energy_and_grad_f64) over every point the
# bibtex "spread" solves (seed 0, B = 24, nIter 10, variants dual and pdipm: the 10 bundle iterates and y*) and the 3 x 10 PGD
# iterates visit is 1.151e-5 (|E| up to 73).  Times 4: the two cut energies that can bound a point from below plus the
# objective's own energy, with slack.
M_BIBTEX = 4 * 1.151e-5


def _small_spec():
    return picnn.FCSpec(20, 12, (24, 12), batchnorm=True)          # the small spec of test_gd.py


def _spec(which):
    return {"small": _small_spec(), "deep3": picnn.FCSpec(40, 24, (64, 48, 32)), "bibtex": picnn.bibtex_spec()}[which]


def entr(x):
    """the scripts' entr(), as they write it (multi-label-cls/ebundle-vs-gd.py:38-41)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = -x * np.log(x) - (1. - x) * np.log(1. - x)
    z[z != z] = 0.0
    return np.sum(z, axis=1)


# ------------------------------------------------------------------------------------------------ CPU


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
    a = lib.icnn_be_pgd_workspace_bytes(128, 159)
    assert a >= 128 * 159 * 4 + 128 * 4
    assert lib.icnn_be_pgd_workspace_bytes(1024, 159) > a
    assert lib.icnn_be_pgd_workspace_bytes(0, 159) > 0
    assert lib.icnn_be_pgd_workspace_bytes(-1, 159) == 0
    assert lib.icnn_be_pgd_workspace_bytes(4, 0) == 0


def _fc_struct(spec):
    from icnn_amd import _lib
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = spec.alpha, int(spec.action_box), spec.ctx_width
    m.wpack = 64
    return m


def _refusals(call):
    """what both PGD entries refuse alike; `call` passes placeholder pointers"""
    assert call(K=0) == -1
    assert call(K=-5) == -1
    assert call(batch=-1) == -1
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert call(lr=bad) == -1, bad
    assert call(lo=0.0) == -1
    assert call(lo=-1e-6) == -1
    assert call(lo=1e-60) == -1                       # float32(lo) == 0
    assert call(hi=1.0) == -1
    assert call(hi=1.0 - 1e-12) == -1                 # float32(hi) == 1
    assert call(lo=0.6, hi=0.4) == -1
    assert call(lo=0.5, hi=0.5) == -1
    assert call(lo=float("nan")) == -1
    assert call(hi=float("nan")) == -1
    assert call(mm=None) == -1
    assert call(ctx=None) == -1
    assert call(y0=None) == -1
    assert call(y=None) == -1
    assert call(ws=None) == -1
    assert call(batch=0) == 0                         # nothing to do, nothing launched


def test_fc_entry_rejects_bad_arguments_before_launch():
    """Placeholder pointers everywhere: every call below must be refused on the host (nothing would survive a launch)."""
    from icnn_amd import _lib
    lib = _lib.load()
    spec = picnn.bibtex_spec()
    m = _fc_struct(spec)
    fake = C.c_void_p(64)

    def call(mm=m, batch=4, K=3, lr=0.1, lo=LO, hi=HI, ctx=fake, y0=fake, y=fake, ws=fake):
        return lib.icnn_be_fc_pgd(None if mm is None else C.byref(mm), ctx, y0, batch, K, lr, lo, hi, y, None, None, ws, None)
    _refusals(call)
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
    m5.action_box = 1                                 # the RL wrapper's box
    assert call(mm=m5) == -1


def test_conv_entry_rejects_bad_arguments_before_launch():
    from icnn_amd import _lib
    lib = _lib.load()
    spec = picnn.ConvSpec()

    def struct():
        m = _lib.ConvModel()
        m.H, m.W = spec.H, spec.W
        for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
            m.filters[l], m.ksize[l], m.stride[l] = nf, k, s
        m.fc_hidden, m.ctx_width = picnn.CONV_FCS[0], spec.ctx_width
        m.wpack, m.work, m.work_batch = 64, 64, 8
        return m
    m = struct()
    fake = C.c_void_p(64)

    def call(mm=m, batch=4, K=3, lr=0.1, lo=LO, hi=HI, ctx=fake, y0=fake, y=fake, ws=fake):
        return lib.icnn_be_conv_pgd(None if mm is None else C.byref(mm), ctx, y0, batch, K, lr, lo, hi, y, None, None, ws, None)
    _refusals(call)
    assert call(batch=9) == -1                        # beyond the model's work_batch
    m2 = struct()
    m2.work = None
    assert call(mm=m2) == -1
    m3 = struct()
    m3.ctx_width += 1
    assert call(mm=m3) == -1
    m4 = struct()
    m4.wpack = None
    assert call(mm=m4) == -1


def test_trace_bound_and_objective_entries_reject_bad_arguments():
    from icnn_amd import _lib
    lib = _lib.load()
    fake = C.c_void_p(64)
    assert lib.icnn_be_entropy_objective(None, fake, 4, 5, fake, None) == -1
    assert lib.icnn_be_entropy_objective(fake, None, 4, 5, fake, None) == -1
    assert lib.icnn_be_entropy_objective(fake, fake, 4, 5, None, None) == -1
    assert lib.icnn_be_entropy_objective(fake, fake, -1, 5, fake, None) == -1
    assert lib.icnn_be_entropy_objective(fake, fake, 4, 0, fake, None) == -1
    assert lib.icnn_be_entropy_objective(fake, fake, 0, 5, fake, None) == 0
    assert lib.icnn_be_bundle_trace(None, fake, fake, None) == -1
    assert lib.icnn_be_dual_bound(None, fake, None) == -1

    def state(variant="dual", batch=4):
        s = _lib.State()
        s.batch, s.n, s.slots, s.cut_dtype, s.variant = batch, 12, 5, _lib.CUT_F32, _lib.VARIANT[variant]
        for name, kind in _lib.State._fields_:
            if kind is C.c_void_p:                    # placeholder buffers
                setattr(s, name, 64)
        return s
    s = state()
    assert lib.icnn_be_bundle_trace(C.byref(s), None, fake, None) == -1
    assert lib.icnn_be_bundle_trace(C.byref(s), fake, None, None) == -1
    assert lib.icnn_be_dual_bound(C.byref(s), None, None) == -1
    assert lib.icnn_be_bundle_trace(C.byref(state("rl")), fake, fake, None) == -1
    s2 = state()
    s2.fvals = None
    assert lib.icnn_be_bundle_trace(C.byref(s2), fake, fake, None) == -1
    s3 = state()
    s3.iters = 9                                      # more iterations than slots: no per-iteration history
    assert lib.icnn_be_bundle_trace(C.byref(s3), fake, fake, None) == -2
    assert lib.icnn_be_bundle_trace(C.byref(state(batch=0)), fake, fake, None) == 0
    assert lib.icnn_be_dual_bound(C.byref(state(batch=0)), fake, None) == 0


def test_python_solve_refuses_bad_arguments():
    from icnn_amd import pgd
    spec = _small_spec()

    class _M:                                          # solve checks its arguments before touching the library
        gd_entry, pgd_entry = "icnn_be_fc_gd", "icnn_be_fc_pgd"

    class _F:                                          # a model class that states no pgd_entry, like ficnn.FICNNModel
        gd_entry = "icnn_be_ficnn_gd"
    m = _M()
    m.spec, m.device = spec, torch.device("cpu")
    ctx = torch.zeros(3, spec.ctx_width)
    for kw in (dict(n_iter=0), dict(lr=float("nan")), dict(lr=float("inf")), dict(lo=0.0), dict(hi=1.0), dict(lo=0.7, hi=0.3)):
        args = dict(n_iter=3, lr=0.1)
        args.update(kw)
        with pytest.raises(ValueError):
            pgd.solve(m, ctx, 0.5, **args)
    with pytest.raises(AssertionError):
        pgd.solve(m, torch.zeros(3, spec.ctx_width + 1), 0.5, 3, 0.1)
    m.spec = picnn.halfcheetah_spec()
    with pytest.raises(ValueError):
        pgd.solve(m, ctx, 0.5, 3, 0.1)
    m = _F()
    m.spec, m.device = spec, torch.device("cpu")
    with pytest.raises(TypeError, match="pgd serves FCModel and ConvModel, not _F"):
        pgd.solve(m, ctx, 0.5, 3, 0.1)
    from icnn_amd import ficnn
    assert not hasattr(ficnn.FICNNModel, "pgd_entry")
    assert (picnn.FCModel.pgd_entry, picnn.ConvModel.pgd_entry) == ("icnn_be_fc_pgd", "icnn_be_conv_pgd")
    with pytest.raises(TypeError):
        pgd.bundle_trace(object())


def test_restated_gradient_is_autograd_of_the_restated_objective():
    """G = dE/dy + log y - log(1 - y) of pgd_ref against float64 autograd of E - H on the small spec."""
    spec = _small_spec()
    rng = np.random.RandomState(3)
    params = picnn.init_params(spec, 3, "spread")
    B = 6
    x = rng.rand(B, spec.n_features).astype(np.float32)
    y = LO + (HI - LO) * rng.rand(B, spec.n_labels)
    y[0, :3] = (LO, HI, 0.5)
    theta = {k: torch.tensor(np.asarray(p, np.float64)) for k, p in params.items()}
    xt = torch.as_tensor(x.astype(np.float64))
    yt = torch.tensor(y, requires_grad=True)
    E, _ = train_ref.energy(spec, theta, xt, yt)
    g, = torch.autograd.grad(E.sum(), yt, retain_graph=True)
    obj = E + (yt * torch.log(yt) + (1.0 - yt) * torch.log(1.0 - yt)).sum(1)
    G_auto, = torch.autograd.grad(obj.sum(), yt)
    G = pgd_ref.grad(g.numpy(), y)
    assert np.abs(G - G_auto.numpy()).max() <= 16 * ULP * np.abs(G).max()
    assert np.abs(G).max() > 10 and np.abs(g.numpy()).max() > 1e-3          # both terms are in it
    assert np.allclose(obj.detach().numpy(), pgd_ref.objective(E.detach().numpy(), y), rtol=1e-14, atol=0)


@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_dual_bound_is_below_the_objective_on_the_quadratic(variant):
    """BASELINE configs[0] through the oracle's solveBatch: obj(y*) - d(lam) >= 0, and every iterate of the restated PGD
    stays >= d.  A float64 quadratic: there is no float32 cut error, so the margin is 0."""
    from oracle import bundle_entropy_oracle as oracle
    prob = problems.quadratic()
    with np.errstate(all="ignore"):
        y, A, b, lam, _, _ = oracle.solveBatch(prob.fg, prob.y0(), 10, variant=variant)
    d, _ = pgd_ref.dual_bounds(A, b, lam)
    assert np.isfinite(d).all()
    f, _ = prob.fg(y)
    gap = pgd_ref.objective(f, y) - d
    print("quadratic %s: gap in [%.3e, %.3e]" % (variant, gap.min(), gap.max()))
    assert (gap >= 0).all() and gap.max() > 0 and gap.max() < 1e-3
    for lr in LRS:
        run = pgd_ref.pgd(prob.fg, prob.y0(), 10, lr, final=True)
        assert (run["obj"] >= d[None]).all() and (run["obj_final"] >= d).all(), lr
    assert (run["obj_final"] < run["obj"][0]).all()                         # at the smallest rate PGD descends (0.1 overshoots here)


# ------------------------------------------------------------------------------------------------ GPU

_FC_CACHE = {}


def _fc_setup(which, B, seed):
    """(spec, params, model, ctx, fg): the model on the device, its context, and the MFMA-order oracle on that very context
    (bit-exact to the kernels' E and dE/dy: tests/test_gd.py)"""
    key = (which, B, seed)
    if key not in _FC_CACHE:
        from oracle import picnn_oracle
        spec = _spec(which)
        params = picnn.init_params(spec, seed, "spread")
        rng = np.random.RandomState(seed)
        x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32) if spec.n_features > 100 else \
            rng.rand(B, spec.n_features).astype(np.float32)
        model = picnn.FCModel(spec, params, "cuda")
        ctx = model.context(torch.from_numpy(x))
        fg = picnn_oracle.make_fg_chain(params, ctx.cpu().numpy(), list(spec.szs), spec.alpha)
        _FC_CACHE[key] = (spec, params, model, ctx, fg)
    return _FC_CACHE[key]


def _start(kind, B, n, seed):
    if kind == "scalar":
        return 0.5, np.full((B, n), 0.5)
    y0 = np.random.RandomState(seed + 7).rand(B, n)
    flat = y0.reshape(-1)
    flat[::11] = (-0.2, 0.0, 1.0, 1.3, 1e-9, 1.0 - 1e-9)[seed % 6]       # outside [lo, hi]
    flat[5::13] = 1.25
    flat[3::17] = -1.0
    return y0, y0


def _screened(which, B, kind, K, lr, seed0=0):
    """The first seed whose restatement feeds the float32 energy the same bits with np.log and with a logarithm one ulp off
    (pgd_ref.screen_feeds): on it a device logarithm a few ulp off np.log moves y by the update's rounding alone."""
    for seed in range(seed0, seed0 + 20):
        spec, params, model, ctx, fg = _fc_setup(which, B, seed)
        y0_arg, y0 = _start(kind, B, spec.n_labels, seed)
        ref, same = pgd_ref.screen_feeds(fg, y0, K, lr)
        if same:
            return spec, model, ctx, y0_arg, ref
    raise AssertionError("no screened seed")


def _check_against(ref, y, obj, fin, K, lr):
    y, obj = y.cpu().numpy(), obj.cpu().numpy()
    dy = np.abs(y - ref["y"])
    de = np.abs(obj - ref["obj"]) / (8 * ULP * ref["scale"])
    print("  max |dy| %.3e (bound %.3e), worst e_k error %.3f of its bound" % (dy.max(), pgd_ref.y_tolerance(K, lr), de.max()))
    assert dy.max() <= pgd_ref.y_tolerance(K, lr)
    edge = (ref["y"] == LO) | (ref["y"] == HI)
    assert np.array_equal(y[edge], ref["y"][edge])
    assert y.min() >= LO and y.max() <= HI
    assert de.max() <= 1.0
    if fin is not None:
        assert (np.abs(fin.cpu().numpy() - ref["obj_final"]) <= 8 * ULP * ref["scale_final"]).all()


FC_CASES = ([("small", B, K, lr, kind) for B in (1, 2, 17, 300, 530) for K in (1, 3, 10) for lr in (0.1, 0.001)
             for kind in ("scalar", "random")]
            + [("deep3", B, 3, 0.1, "random") for B in (2, 17, 530)]
            + [("bibtex", B, K, lr, "random") for B in (1, 3) for K, lr in ((3, 0.1), (10, 0.001))]
            + [("bibtex", 2, 10, 0.1, "scalar")])


@pytest.mark.gpu
@pytest.mark.parametrize("which,B,K,lr,kind", FC_CASES)
def test_fc_solve_against_restatement(which, B, K, lr, kind):
    """B = 1, 2, 17: the rows path with one sample per workgroup; 300: with two; 530: the persistent tiles with a partial last
    tile.  bibtex: n = 159 drives the lane-strided loops past 64 with a ragged tail."""
    from icnn_amd import pgd
    spec, model, ctx, y0_arg, ref = _screened(which, B, kind, K, lr)
    y0 = y0_arg if np.ndim(y0_arg) == 0 else torch.from_numpy(y0_arg).cuda()
    y, obj, fin = pgd.solve(model, ctx, y0, K, lr, final=True)
    torch.cuda.synchronize()
    assert y.shape == (B, spec.n_labels) and obj.shape == (K, B) and fin.shape == (B,)
    assert y.dtype == obj.dtype == fin.dtype == torch.float64
    _check_against(ref, y, obj, fin, K, lr)
    assert np.abs(ref["y"] - ref["iterates"][0]).max() > 1e-5                   # y did move


@pytest.mark.gpu
@pytest.mark.parametrize("B", [17, 530])
def test_fc_clip_case(B):
    """lr = 1.0 on the small spec: the restatement's iterates hold exact lo and exact hi, and the device agrees there bit for
    bit."""
    from icnn_amd import pgd
    K, lr = 5, 1.0
    spec, model, ctx, y0_arg, ref = _screened("small", B, "random", K, lr)
    its = np.stack(ref["iterates"][1:])
    assert (its == LO).any() and (its == HI).any()
    assert (ref["y"] == LO).any() and (ref["y"] == HI).any()
    y, obj, fin = pgd.solve(model, ctx, torch.from_numpy(y0_arg).cuda(), K, lr, final=True)
    torch.cuda.synchronize()
    _check_against(ref, y, obj, fin, K, lr)


@pytest.mark.gpu
def test_optional_outputs_do_not_change_y():
    from icnn_amd import pgd
    for B in (17, 530):
        spec, params, model, ctx, fg = _fc_setup("small", B, 0)
        y, obj, fin = pgd.solve(model, ctx, 0.5, 7, 0.1, final=True)
        y2, obj2, fin2 = pgd.solve(model, ctx, 0.5, 7, 0.1, trace=False, final=False)
        y3, obj3, fin3 = pgd.solve(model, ctx, 0.5, 7, 0.1, trace=True, final=False)
        torch.cuda.synchronize()
        assert obj2 is None and fin2 is None and fin3 is None
        assert torch.equal(y, y2) and torch.equal(y, y3) and torch.equal(obj, obj3)
        # the loop decides by null pointers what it records: all four combinations, on the rows path (17) and on the tiles
        # with a partial last tile (530), leave y and every output that is present unchanged
        yf, objf, finf = pgd.solve(model, ctx, 0.5, 3, 0.1, trace=True, final=True)
        for trace in (True, False):
            for final in (True, False):
                yc, objc, finc = pgd.solve(model, ctx, 0.5, 3, 0.1, trace=trace, final=final)
                torch.cuda.synchronize()
                assert (objc is not None) == trace and (finc is not None) == final
                assert torch.equal(yc, yf), (B, trace, final)
                assert objc is None or torch.equal(objc, objf), (B, trace, final)
                assert finc is None or torch.equal(finc, finf), (B, trace, final)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "bibtex"])
def test_a_sample_does_not_depend_on_its_batch(which):
    """A sample solved alone equals the same sample inside a batch of 17 (one per workgroup), of 300 (two per workgroup) and of
    530 (the tiles), in y, e_k and e_K, bit for bit: the context rows are those of the large batch."""
    from icnn_amd import pgd
    spec, params, model, ctx, fg = _fc_setup(which, 530, 1)
    K, lr = 5, 0.1
    y0 = torch.from_numpy(_start("random", 530, spec.n_labels, 1)[1]).cuda()
    y, obj, fin = pgd.solve(model, ctx, y0, K, lr, final=True)
    for i in (0, 16, 529):
        for lo_, hi_ in ((i, i + 1), (max(i - 16, 0), max(i - 16, 0) + 17), (max(i - 299, 0), max(i - 299, 0) + 300)):
            ys, objs, fins = pgd.solve(model, ctx[lo_:hi_].contiguous(), y0[lo_:hi_], K, lr, final=True)
            torch.cuda.synchronize()
            assert torch.equal(ys[i - lo_], y[i]), (i, lo_, hi_)
            assert torch.equal(objs[:, i - lo_], obj[:, i]) and torch.equal(fins[i - lo_], fin[i]), (i, lo_, hi_)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [17, 530])
def test_captured_replay_equals_eager(B):
    from icnn_amd import pgd
    spec, params, model, ctx, fg = _fc_setup("small", B, 2)
    y0 = torch.from_numpy(_start("random", B, spec.n_labels, 2)[1]).cuda()
    eager = [t.clone() for t in pgd.solve(model, ctx, y0, 6, 0.1, final=True)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pgd.solve(model, ctx, y0, 6, 0.1, final=True)
    for t in out:
        t.fill_(0.123)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [5, 64, 65, 159])
@pytest.mark.parametrize("B", [1, 17])
def test_objective_against_numpy(n, B):
    from icnn_amd import pgd
    spec = picnn.FCSpec(20, n, (24, 12), batchnorm=True)
    rng = np.random.RandomState(n + B)
    params = picnn.init_params(spec, n, "spread")
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(rng.rand(B, spec.n_features).astype(np.float32)))
    y = rng.rand(B, n)
    y[0, 0], y[0, n - 1] = 0.0, 1.0                   # 0 log 0 := 0 on both sides
    y[B - 1, n // 2] = 1.0
    yd = torch.from_numpy(y).cuda()
    got = pgd.objective(model, ctx, yd)
    E, _ = model.fg(ctx, yd)
    torch.cuda.synchronize()
    E = E.cpu().numpy()
    got = got.cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (B,) and np.isfinite(got).all()
    ref = E - entr(y)                                 # as the scripts write it
    scale = pgd_ref.objective_scale(E, y)
    assert (np.abs(got - ref) <= 8 * ULP * scale).all()
    assert (np.abs(got - pgd_ref.objective(E, y)) <= 8 * ULP * scale).all()
    # rows of exact zeros and ones: no entropy at all, the energy alone
    corner = (rng.rand(B, n) < 0.5).astype(np.float64)
    cd = torch.from_numpy(corner).cuda()
    got = pgd.objective(model, ctx, cd)
    E, _ = model.fg(ctx, cd)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), E.cpu().numpy().astype(np.float64))


def _fused_bibtex(regime, variant, seed, B=24, n_iter=10):
    """A fused bibtex solve (native result) whose host callback records es - entr(x), exactly as the scripts do"""
    from icnn_amd import bundle_entropy
    spec = picnn.bibtex_spec()
    params = picnn.init_params(spec, seed, regime)
    x = (np.random.RandomState(seed + 100).rand(B, spec.n_features) < 0.04).astype(np.float32)
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(x))
    seen = []
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=np.full((B, spec.n_labels), 0.5), nIter=n_iter, variant=variant,
                                    native=True, check=False,
                                    callback=lambda t, es, xs: seen.append((es - entr(xs), pgd_ref.objective_scale(es, xs))))
    return spec, model, ctx, res, seen


def check_trace(res, seen, T):
    from icnn_amd import pgd
    obj, calls = pgd.bundle_trace(res)
    torch.cuda.synchronize()
    obj, calls = obj.cpu().numpy(), int(calls.item())
    assert obj.shape == (T, res.state.B)
    assert calls == len(seen)
    ref, scale = np.stack([s[0] for s in seen]), np.stack([s[1] for s in seen])
    assert np.isfinite(obj[:calls]).all()
    worst = (np.abs(obj[:calls] - ref) / (8 * ULP * scale)).max()
    print("  bundle trace: %d calls of %d, worst error %.3f of its bound" % (calls, T, worst))
    assert worst <= 1.0
    assert np.isnan(obj[calls:]).all()
    return obj, calls


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
@pytest.mark.parametrize("regime", ["init", "spread"])
def test_bundle_trace_against_the_scripts_callback(regime, variant):
    """regime "init", variant dual: a batch in which the rank test stops some samples early while others run every iteration
    (reseeded until it is one).  Variant pdipm has no such batch: in this regime the interior-point iterate falls back onto
    the first cut's linear piece at t = 1 or 2 and the rank test ends EVERY sample -- 0 of 24 samples ran on in each of 70
    seeds at the inputs used here, and in 64 more draws with denser or Gaussian inputs and random starts (CPU oracle).  There
    the solve ends early as a whole (fewer calls than iterations, NaN rows behind them), and the samples that run every
    iteration are those of the "spread" regime, where all 24 do."""
    T = 10
    for seed in range(10):
        spec, model, ctx, res, seen = _fused_bibtex(regime, variant, seed, n_iter=T)
        B = res.state.B
        fin = res.finished[:B].cpu().numpy().astype(bool)
        n_iters = res.n_iters[:B].cpu().numpy()
        early, full = fin & (n_iters < T - 2), ~fin
        if regime != "init" or (early.any() and (full.any() or variant == "pdipm")):
            break
    else:
        raise AssertionError("no seed with an early finish next to a full run")
    obj, calls = check_trace(res, seen, T)
    if regime == "spread":
        assert full.any() and calls == T
        return
    assert early.any()
    if variant == "dual":
        assert full.any() and calls == T
    else:
        assert fin.all() and calls == int(n_iters.max()) + 2 < T
    u = int(np.nonzero(early)[0][0])                  # a finished sample keeps its last objective
    assert np.all(obj[n_iters[u] + 1:calls, u] == obj[n_iters[u] + 1, u])


@pytest.mark.gpu
def test_bundle_trace_ends_with_the_last_sample():
    """A batch of one sample of the "init" regime that the rank test stops early: the loop ends after that iteration, so there
    are fewer calls than iterations and the rows beyond them are NaN."""
    from icnn_amd import bundle_entropy
    T = 10
    for seed in range(10):
        spec, model, ctx, res, seen = _fused_bibtex("init", "dual", seed, n_iter=T)
        B = res.state.B
        fin = res.finished[:B].cpu().numpy().astype(bool)
        n_iters = res.n_iters[:B].cpu().numpy()
        early = np.nonzero(fin & (n_iters < T - 2))[0]
        if len(early):
            break
    else:
        raise AssertionError("no early finish")
    u = int(early[0])
    seen = []
    res1 = bundle_entropy.solveBatch(f=model, ctx=ctx[u:u + 1].contiguous(), y0=np.full((1, spec.n_labels), 0.5), nIter=T,
                                     variant="dual", native=True, check=False,
                                     callback=lambda t, es, xs: seen.append((es - entr(xs), pgd_ref.objective_scale(es, xs))))
    obj, calls = check_trace(res1, seen, T)
    assert calls < T


@pytest.mark.gpu
def test_bundle_trace_refuses_variant_rl():
    from icnn_amd import bundle_entropy, pgd
    spec = picnn.halfcheetah_spec()
    params = picnn.init_params(spec, 0, "spread", yu_bias=1.0, gate_bias=1.0)
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(np.random.RandomState(0).randn(8, spec.n_features).astype(np.float32)))
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=np.full((8, spec.n_labels), 0.5), nIter=5, variant="rl", native=True,
                                    check=False)
    with pytest.raises(ValueError):
        pgd.bundle_trace(res)


def _check_bound(res):
    from icnn_amd import pgd
    d = pgd.dual_bound(res)
    torch.cuda.synchronize()
    d = d.cpu().numpy()
    _, A, b, lam, _, _ = res.as_reference_tuple()
    ref, scale = pgd_ref.dual_bounds(A, b, lam)
    inf = np.isinf(ref)
    assert np.array_equal(d[inf], ref[inf])
    err = np.abs(d[~inf] - ref[~inf]) / (16 * ULP * scale[~inf])
    print("  dual bound: worst error %.3f of its bound, %d samples without a cut" % (err.max(), int(inf.sum())))
    assert err.max() <= 1.0
    return d, inf


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_dual_bound_float32_cuts(variant):
    spec, model, ctx, res, _ = _fused_bibtex("spread", variant, 0)
    d, inf = _check_bound(res)
    assert not inf.any() and np.isfinite(d).all()


@pytest.mark.gpu
def test_dual_bound_float64_cuts_and_empty_bundles():
    from icnn_amd import bundle_entropy
    prob = problems.quadratic()                       # generic mode with a float64 fg
    res = bundle_entropy.solveBatch(prob.fg, prob.y0(), nIter=10, variant="dual", native=True)
    assert res.G.dtype == torch.float64
    d, inf = _check_bound(res)
    assert not inf.any()
    f, _ = prob.fg(res.y.cpu().numpy())
    assert (pgd_ref.objective(f, res.y.cpu().numpy()) - d >= 0).all()        # float64 cuts: no margin
    prob = problems.zero_gradient_rows()              # some first cuts are the zero vector: no bundle, no bound
    res = bundle_entropy.solveBatch(prob.fg, prob.y0(), nIter=6, variant="dual", native=True)
    d, inf = _check_bound(res)
    assert np.array_equal(inf, prob.dead) and (d[prob.dead] == -np.inf).all() and np.isfinite(d[~prob.dead]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_certificate_objective_above_bound_bibtex(variant):
    """Whatever the summation order: the objective at y* and at every PGD iterate is above the bundle's bound, up to the
    float32 rounding of the energies inside the cuts (M_BIBTEX)."""
    from icnn_amd import pgd
    spec, model, ctx, res, _ = _fused_bibtex("spread", variant, 0)
    d = pgd.dual_bound(res)
    gap = pgd.gap(model, ctx, res)
    torch.cuda.synchronize()
    print("  %s: gap in [%.3e, %.3e]" % (variant, float(gap.min()), float(gap.max())))
    assert bool((gap >= -M_BIBTEX).all())
    assert float(gap.max()) > 0
    for lr in LRS:
        y, obj, fin = pgd.solve(model, ctx, 0.5, 10, lr, final=True)
        torch.cuda.synchronize()
        assert bool((obj >= d[None] - M_BIBTEX).all()) and bool((fin >= d - M_BIBTEX).all()), lr
        assert float(fin.mean()) < float(obj[0].mean())
