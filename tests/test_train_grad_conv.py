"""Training gradient of the conv PICNN of the completion experiment (icnn_be_conv_surrogate_grad, icnn_amd.train): HIP
kernels against a float64 torch double-backward statement of the reference graph on the gathered feed rows
(tests/train_conv_ref.py); the C ABI's sizes and argument checks on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import train_conv_ref
from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_conv_grad_floats", "icnn_be_conv_surrogate_grad_work_floats", "icnn_be_conv_surrogate_grad"]
SPEC = picnn.ConvSpec()
# Screening margin of the pre-activations.  A problem of this size has ~1e5 pre-activations per sample set, so a 1e-4 screen
# (tests/test_train_grad.py's) passes almost no seed; 1e-5 is still ten times the float32 rounding of a 2048-term sum.
MARGIN = 1e-5
ZERO_VARS = ("u4/W", "u4/b", "z2_y_red/W", "z2_y_red/b")
# The u-path variables sit behind the BatchNorm backward, whose output over 6 samples is the small residue of
# du - mean(du) - xhat mean(du xhat): float32 rounding of du is amplified there (measured: 1.15e-4 of max|g64| at worst).
BN_TOL = 2e-4
# Variables that reach F only through zu3 / zu4: their gradient is sum_r c_r (x-only term) per sample, which cancels when the
# rows of a sample share their masks and c sums to zero per sample (the implicit feed's does)
CANCEL_CANDIDATES = ("z3_u/W", "z3_u/b", "z4_u/W", "z4_u/b")


def _small_problem(regime, seed, with_v):
    """Seeded model and feed (6 samples with 1-4 rows each), screened so that no float64 pre-activation (z-path, u-path,
    gates) is within MARGIN of zero: the float32 masks then agree with the float64 ones."""
    for s in range(seed, seed + 300):
        rng = np.random.RandomState(s)
        params = picnn.init_conv_params(SPEC, s, regime)
        for k in params:                         # non-trivial BatchNorm parameters and biases
            if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
                params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
        B = 6
        counts = rng.randint(1, 5, size=B)
        x = rng.rand(B, SPEC.H, SPEC.W, 1).astype(np.float32)
        samp = np.repeat(np.arange(B), counts)
        R = len(samp)
        y = rng.rand(R, SPEC.n_labels)
        v = rng.randn(R, SPEC.n_labels) if with_v else None
        c = rng.randn(R)
        if train_conv_ref.u_margin(SPEC, params, x[samp]) < MARGIN:
            continue
        g64, F64, margin = train_conv_ref.surrogate_grad64(SPEC, params, x[samp], y, v, c)
        if margin < MARGIN:
            continue
        return dict(params=params, x=x, samp=samp, counts=counts, y=y, v=v, c=c, g64=g64, F64=F64)
    raise AssertionError("no screened seed")


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ CPU


def _c_structs():
    """ConvModel / ConvCtx with placeholder pointers: enough for the host-side size queries and argument checks."""
    from icnn_amd import _lib
    m = _lib.ConvModel()
    m.H, m.W = SPEC.H, SPEC.W
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        m.filters[l], m.ksize[l], m.stride[l] = nf, k, s
    m.fc_hidden, m.ctx_width, m.wpack = picnn.CONV_FCS[0], SPEC.ctx_width, 64
    c = _lib.ConvCtx()
    for i in range(7):
        c.w_stage[i] = c.b_stage[i] = 64
    for i in range(4):
        c.bn_gamma[i] = c.bn_beta[i] = 64
    c.bn_eps = 1e-5
    return m, c


def test_conv_exports_in_header_and_library():
    from icnn_amd import _lib
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()


def test_conv_grad_layout_matches_library_size():
    from icnn_amd import _lib, train
    lib = _lib.load()
    m, c = _c_structs()
    n = lib.icnn_be_conv_grad_floats(C.byref(m), C.byref(c))
    layout = train.grad_layout(SPEC)
    params = picnn.init_conv_params(SPEC)
    assert [k for k, _ in layout] == list(params.keys())
    assert all(tuple(params[k].shape) == shape for k, shape in layout)
    assert n == sum(int(np.prod(s)) for _, s in layout) == sum(p.size for p in params.values())
    views = train.unpack_grad(SPEC, torch.arange(n, dtype=torch.float64))
    assert list(views.keys()) == list(params.keys())
    assert int(views["u0/b"].reshape(-1)[0]) == params["u0/W"].size           # the bias follows its weight
    assert lib.icnn_be_conv_surrogate_grad_work_floats(C.byref(m), C.byref(c), 70, 350) > 0
    # a free image size that passes the layout checks is accepted as icnn_be_conv_fg accepts it
    m.H, m.W = 32, 32
    m.ctx_width = picnn.ConvSpec(32, 32).ctx_width
    assert lib.icnn_be_conv_pack_floats(C.byref(m)) > 0
    assert lib.icnn_be_conv_grad_floats(C.byref(m), C.byref(c)) == sum(
        int(np.prod(s)) for _, s in train.grad_layout(picnn.ConvSpec(32, 32)))


def test_conv_bad_shapes_are_rejected_before_launch():
    from icnn_amd import _lib
    lib = _lib.load()
    m, c = _c_structs()
    fake = C.c_void_p(64)

    def call(mm, cc, batch, rows, x=fake, ro=fake, y=fake, v=fake, cv=fake, grad=fake, work=fake):
        return lib.icnn_be_conv_surrogate_grad(C.byref(mm), C.byref(cc), x, batch, ro, rows, y, v, cv, grad, None, work, None)
    assert call(m, c, 0, 4) == -1                     # no samples
    assert call(m, c, -3, 4) == -1                    # negative batch
    assert call(m, c, 4, 0) == -1                     # no rows
    assert call(m, c, 4, -1) == -1
    assert call(m, c, 4, 1 << 28) == -2               # rows beyond the int indexing of the im2col buffers
    assert call(m, c, 4, 1 << 28, v=None) == -2
    for k in ("x", "ro", "y", "cv", "grad", "work"):  # NULL required pointers
        assert call(m, c, 4, 4, **{k: None}) == -1, k
    c2 = _c_structs()[1]
    c2.w_stage[3] = None
    assert call(m, c2, 4, 4) == -1
    m2 = _c_structs()[0]
    m2.ksize[1] = 5                                   # not the reference's hyper-parameters (icnn_be_conv_fg refuses them)
    assert call(m2, c, 4, 4) != 0
    assert lib.icnn_be_conv_grad_floats(C.byref(m2), C.byref(c)) == 0
    m3 = _c_structs()[0]
    m3.filters[0] = 16
    m3.ctx_width = 0
    assert call(m3, c, 4, 4) != 0
    m4 = _c_structs()[0]
    m4.ctx_width += 1                                 # context width that does not match the shape
    assert call(m4, c, 4, 4) == -1
    assert lib.icnn_be_conv_surrogate_grad_work_floats(C.byref(m4), C.byref(c), 4, 4) == 0


def test_python_rejects_row_offset_of_another_batch():
    from icnn_amd import train
    model = picnn.ConvModel(SPEC, picnn.init_conv_params(SPEC), device="cpu")
    x = torch.zeros(3, SPEC.H, SPEC.W, 1)
    y = torch.zeros(4, SPEC.n_labels, dtype=torch.float64)
    with pytest.raises(ValueError):
        train.surrogate_grad(model, x, (y, y, torch.zeros(4, dtype=torch.float64)), row_offset=np.array([0, 1, 4], np.int32))


def test_reference_helper_states_the_oracle_network():
    """The float64 helper's E and dE/dy agree with oracle/picnn_conv_oracle (float32) on a seeded problem."""
    from oracle import picnn_conv_oracle as oracle
    rng = np.random.RandomState(3)
    params = picnn.init_conv_params(SPEC, 3, "spread")
    R = 5
    x = rng.rand(R, SPEC.H, SPEC.W, 1).astype(np.float32)
    y = rng.rand(R, SPEC.n_labels)
    ctx = oracle.context(params, torch.from_numpy(x))
    fg = oracle.make_fg_from_context(params, oracle.flat_context(ctx), SPEC.H, SPEC.W)
    E32, g32 = fg(y)
    E64, g64 = train_conv_ref.energy_and_grad64(SPEC, params, x, y.astype(np.float32))
    assert np.max(np.abs(E64 - E32)) <= 1e-4 * np.max(np.abs(E64))
    assert np.max(np.abs(g64 - g32)) <= 1e-4 * np.max(np.abs(g64))


# ------------------------------------------------------------------------------------------------ GPU


def _surrogate(model, x, y, v, c, off, F_rows=None):
    from icnn_amd import train
    return train.surrogate_grad(model, x, (y, v, c) if v is not None else (y, c), row_offset=off, F_rows=F_rows)


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["init", "spread"])
@pytest.mark.parametrize("with_v", [True, False], ids=["v", "no_v"])
def test_every_variable_against_float64(regime, with_v):
    prob = _small_problem(regime, 11 if regime == "init" else 21, with_v)
    model = picnn.ConvModel(SPEC, prob["params"])
    R = len(prob["samp"])
    F = torch.empty(R, dtype=torch.float32, device="cuda")
    x = torch.from_numpy(prob["x"]).cuda()
    off = torch.from_numpy(_offsets(prob["counts"])).cuda()
    y, c = torch.from_numpy(prob["y"]).cuda(), torch.from_numpy(prob["c"]).cuda()
    v = torch.from_numpy(prob["v"]).cuda() if with_v else None
    g = _surrogate(model, x, y, v, c, off, F_rows=F)
    torch.cuda.synchronize()
    assert list(g.keys()) == list(prob["params"].keys())
    bad = []
    for name, ref in prob["g64"].items():
        got = g[name].double().cpu().numpy().reshape(ref.shape)
        if name in ZERO_VARS:
            if not (np.all(got == 0) and np.all(ref == 0)):
                bad.append(name)
            continue
        scale = np.max(np.abs(ref))
        err = np.max(np.abs(got - ref))
        if not (scale > 0 and err <= (BN_TOL if name.startswith("u") else 1e-4) * scale):
            bad.append((name, err / scale if scale > 0 else err))
    assert not bad, bad
    F64 = prob["F64"]
    assert np.max(np.abs(F.double().cpu().numpy() - F64)) <= 1e-4 * np.max(np.abs(F64))


@pytest.mark.gpu
def test_one_row_per_sample_matches_shipped_fg():
    """F_rows = c E + <dE/dy, v> from ConvModel.fg on ConvModel.context(x): with one row per sample the weighted BatchNorm is
    the plain one of the shipped context producer."""
    rng = np.random.RandomState(7)
    params = picnn.init_conv_params(SPEC, 7, "spread")
    model = picnn.ConvModel(SPEC, params)
    B = 8
    x = torch.from_numpy(rng.rand(B, SPEC.H, SPEC.W, 1).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.rand(B, SPEC.n_labels)).cuda()
    v = torch.from_numpy(rng.randn(B, SPEC.n_labels)).cuda()
    c = torch.from_numpy(rng.randn(B)).cuda()
    F = torch.empty(B, dtype=torch.float32, device="cuda")
    _surrogate(model, x, y, v, c, torch.arange(B + 1, dtype=torch.int32, device="cuda"), F_rows=F)
    E, g = model.fg(model.context(x), y)
    want = c * E.double() + (g.double() * v).sum(1)
    torch.cuda.synchronize()
    scale = float(want.abs().max())
    assert float((F.double() - want).abs().max()) <= 1e-4 * scale


@pytest.mark.gpu
def test_end_to_end_reference_training_batch():
    """solve -> implicit_feed(mse) -> surrogate_grad at the reference's training batch (70, nIter 5), every variable within
    1e-4 relative Frobenius error of float64.  z4_u/* reach F only through zu4, whose gradient is sum_r c_r per sample, and
    the implicit feed's c sums to zero per sample: their float64 gradient is rounding residue, so they are checked against
    the size of the cancelling terms (the same gradient with c replaced by |c|).  z3_u/* do the same where every row of a
    sample has the same fc3 mask."""
    from icnn_amd import bundle_entropy
    B, n_iter = 70, 5
    rng = np.random.RandomState(70)
    params = picnn.init_conv_params(SPEC, 70, "spread")
    model = picnn.ConvModel(SPEC, params)
    x = rng.rand(B, SPEC.H, SPEC.W, 1).astype(np.float32)
    xd = torch.from_numpy(x).cuda()
    ctx = model.context(xd)
    y0 = np.repeat((0.2 + 0.6 * rng.rand(SPEC.n_labels))[None], B, axis=0)
    res = bundle_entropy.FusedSolver(model, B, n_iter, "dual").solve(ctx, torch.from_numpy(y0).cuda())
    labels = rng.rand(B, SPEC.n_labels)
    feed = bundle_entropy.implicit_feed(res, labels, "mse")
    from icnn_amd import train
    g = train.surrogate_grad(model, xd, feed)
    torch.cuda.synchronize()
    samp = feed.sample.cpu().numpy()
    yr, vr, cr = feed.y.cpu().numpy(), feed.v.cpu().numpy(), feed.c.cpu().numpy()
    assert len(samp) > B
    g64, _, _ = train_conv_ref.surrogate_grad64(SPEC, params, x[samp], yr, vr, cr)
    gabs, _, _ = train_conv_ref.surrogate_grad64(SPEC, params, x[samp], yr, None, np.abs(cr))
    assert np.linalg.norm(g64["z4_u/b"]) <= 1e-6 * np.linalg.norm(gabs["z4_u/b"])      # c sums to zero per sample
    for name, ref in g64.items():
        got = g[name].double().cpu().numpy().reshape(ref.shape)
        if name in ZERO_VARS:
            assert np.all(got == 0), name
            continue
        err = np.linalg.norm(got - ref)
        size = np.linalg.norm(gabs[name])
        if name in CANCEL_CANDIDATES and np.linalg.norm(ref) <= 1e-6 * size:
            assert err <= 1e-4 * size, (name, err, size)
            continue
        assert err <= 1e-4 * np.linalg.norm(ref), (name, err, np.linalg.norm(ref))


@pytest.mark.gpu
def test_deterministic_and_graph_capture():
    from icnn_amd import _lib, train
    prob = _small_problem("spread", 31, True)
    model = picnn.ConvModel(SPEC, prob["params"])
    R, B = len(prob["samp"]), len(prob["counts"])
    x = torch.from_numpy(prob["x"]).cuda()
    off = torch.from_numpy(_offsets(prob["counts"])).cuda()
    y, v, c = (torch.from_numpy(prob[k]).cuda() for k in ("y", "v", "c"))
    g1 = torch.cat([t.reshape(-1) for t in _surrogate(model, x, y, v, c, off).values()])
    g2 = torch.cat([t.reshape(-1) for t in _surrogate(model, x, y, v, c, off).values()])
    assert torch.equal(g1, g2)
    # the raw entry point captured on one stream, then replayed
    n = train.grad_floats(model)
    nw = int(model._lib.icnn_be_conv_surrogate_grad_work_floats(C.byref(model.c_model), C.byref(model.c_ctx), B, R))
    grad = torch.empty(n, dtype=torch.float32, device="cuda")
    work = torch.empty(nw, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=s):
        rc = model._lib.icnn_be_conv_surrogate_grad(
            C.byref(model.c_model), C.byref(model.c_ctx), x.data_ptr(), B, off.data_ptr(), R, y.data_ptr(), v.data_ptr(),
            c.data_ptr(), grad.data_ptr(), None, work.data_ptr(), C.c_void_p(s.cuda_stream))
    _lib.check(rc, "icnn_be_conv_surrogate_grad")
    grad.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(grad, g1)


@pytest.mark.gpu
def test_duplicated_rows_double_the_gradient():
    prob = _small_problem("init", 41, True)
    model = picnn.ConvModel(SPEC, prob["params"])
    x = torch.from_numpy(prob["x"]).cuda()
    counts = prob["counts"]
    y, v, c = (torch.from_numpy(prob[k]).cuda() for k in ("y", "v", "c"))
    g1 = _surrogate(model, x, y, v, c, torch.from_numpy(_offsets(counts)).cuda())
    # every sample's rows twice, still grouped by sample: BatchNorm statistics are unchanged, F doubles
    idx = np.concatenate([np.tile(np.arange(a, b), 2) for a, b in zip(_offsets(counts)[:-1], _offsets(counts)[1:])])
    it = torch.from_numpy(idx).cuda()
    g2 = _surrogate(model, x, y[it], v[it], c[it], torch.from_numpy(_offsets(2 * counts)).cuda())
    torch.cuda.synchronize()
    for name in g1:
        a, b = g1[name].double(), g2[name].double()
        scale = float(a.abs().max())
        assert float((b - 2 * a).abs().max()) <= 1e-5 * scale, name
