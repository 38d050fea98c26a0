"""Training gradient of the FC PICNN (icnn_be_fc_surrogate_grad, icnn_amd.train): HIP kernels against a float64 torch
double-backward statement of the reference graph on the gathered feed rows (tests/train_ref.py); the C ABI's sizes and
argument checks and TFAdam on the host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import train_ref
from icnn_amd import picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_fc_grad_floats", "icnn_be_fc_surrogate_grad_work_floats", "icnn_be_fc_surrogate_grad"]


def _small_spec(bn, alpha, box):
    return picnn.FCSpec(20, 12, (24, 12), alpha=alpha, batchnorm=bn, action_box=box)


def _small_problem(spec, seed, with_v):
    """Seeded model and feed (6 samples with 1-4 rows each); screened so that no float64 pre-activation is within 1e-4 of
    zero (the float32 masks then agree with the float64 ones)."""
    for s in range(seed, seed + 200):
        rng = np.random.RandomState(s)
        params = picnn.init_params(spec, s, "spread")
        for k in params:                         # non-trivial BatchNorm parameters and biases
            if k.endswith("/bn/gamma") or k.endswith("/bn/beta") or k.endswith("/b"):
                params[k] = (params[k] + 0.1 * rng.randn(*params[k].shape)).astype(np.float32)
        B = 6
        counts = rng.randint(1, 5, size=B)
        x = rng.rand(B, spec.n_features).astype(np.float32)
        samp = np.repeat(np.arange(B), counts)
        R = len(samp)
        y = rng.rand(R, spec.n_labels)
        v = rng.randn(R, spec.n_labels) if with_v else None
        c = rng.randn(R)
        g64, F64, margin = train_ref.surrogate_grad64(spec, params, x[samp], y, v, c)
        if margin < 1e-4 or train_ref.u_margin(spec, params, x[samp]) < 1e-4:
            continue
        return dict(params=params, x=x, samp=samp, counts=counts, y=y, v=v, c=c, g64=g64, F64=F64)
    raise AssertionError("no screened seed")


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)


# ------------------------------------------------------------------------------------------------ CPU


def _c_structs(spec):
    """FcModel / FcCtx of a spec with placeholder pointers: enough for the host-side size queries and argument checks."""
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


def test_new_exports_in_header_and_library():
    from icnn_amd import _lib
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS
        assert hasattr(lib, name)
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()


@pytest.mark.parametrize("spec", [picnn.bibtex_spec(), picnn.halfcheetah_spec(), _small_spec(True, 0.0, False)],
                         ids=["bibtex", "halfcheetah", "small"])
def test_grad_layout_matches_library_size(spec):
    from icnn_amd import _lib, train
    lib = _lib.load()
    m, c = _c_structs(spec)
    n = lib.icnn_be_fc_grad_floats(C.byref(m), C.byref(c))
    layout = train.grad_layout(spec)
    params = picnn.init_params(spec)
    assert [k for k, _ in layout] == list(params.keys())
    assert all(tuple(params[k].shape) == shape for k, shape in layout)
    assert n == sum(int(np.prod(s)) for _, s in layout) == sum(p.size for p in params.values())
    views = train.unpack_grad(spec, torch.arange(n, dtype=torch.float32))
    assert list(views.keys()) == list(params.keys())
    assert int(views[layout[1][0]].reshape(-1)[0]) == int(np.prod(layout[0][1]))      # second variable starts behind the first
    assert lib.icnn_be_fc_surrogate_grad_work_floats(C.byref(m), C.byref(c), 128, 1280) > 0


def test_bad_shapes_are_rejected_before_launch():
    from icnn_amd import _lib
    lib = _lib.load()
    spec = _small_spec(True, 0.0, False)
    m, c = _c_structs(spec)
    fake = C.c_void_p(64)

    def call(mm, cc, batch, rows, v=fake):
        return lib.icnn_be_fc_surrogate_grad(C.byref(mm), C.byref(cc), fake, batch, fake, rows, fake, v, fake, fake, None,
                                             fake, None)
    assert call(m, c, 0, 4) == -1                     # no samples
    assert call(m, c, 4, 0) == -1                     # no rows
    assert call(m, c, 4, 1 << 30) == -2               # rows beyond the int indexing of the row kernels
    assert call(m, c, 4, 1 << 30, v=None) == -2
    m2, c2 = _c_structs(spec)
    c2.width[0] = 23                                  # context weights of another shape
    assert call(m2, c2, 4, 4) == -1
    assert lib.icnn_be_fc_grad_floats(C.byref(m2), C.byref(c2)) == 0
    m3, c3 = _c_structs(spec)
    m3.width[spec.n_layers - 1] = 2                   # last layer not scalar
    assert call(m3, c3, 4, 4) == -1
    m4, c4 = _c_structs(spec)
    m4.wpack = None
    assert call(m4, c4, 4, 4) == -1
    assert lib.icnn_be_fc_surrogate_grad(None, C.byref(c), fake, 4, fake, 4, fake, fake, fake, fake, None, fake, None) == -1
    assert lib.icnn_be_fc_surrogate_grad_work_floats(C.byref(m), C.byref(c), 0, 4) == 0


def test_tfadam_matches_tensorflow_update_rule():
    """tf.train.AdamOptimizer (documented rule: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t), theta -= lr_t m / (sqrt(v) + eps))."""
    from icnn_amd.train import TFAdam
    rng = np.random.RandomState(3)
    theta0 = {"a/W": rng.randn(5, 3), "a/b": rng.randn(3)}
    grads = [{k: rng.randn(*v.shape) for k, v in theta0.items()} for _ in range(6)]
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    ref = {k: v.copy() for k, v in theta0.items()}
    m = {k: np.zeros_like(v) for k, v in ref.items()}
    s = {k: np.zeros_like(v) for k, v in ref.items()}
    for t, g in enumerate(grads, 1):
        lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
        for k in ref:
            m[k] = b1 * m[k] + (1 - b1) * g[k]
            s[k] = b2 * s[k] + (1 - b2) * g[k] * g[k]
            ref[k] = ref[k] - lr_t * m[k] / (np.sqrt(s[k]) + eps)
    params = {k: torch.tensor(v) for k, v in theta0.items()}
    opt = TFAdam(params, lr=lr, beta1=b1, beta2=b2, eps=eps)
    for g in grads:
        opt.step({k: torch.tensor(v) for k, v in g.items()})
    for k in ref:
        assert np.allclose(params[k].numpy(), ref[k], rtol=1e-12, atol=1e-14), k
    # and it is not torch.optim.Adam (eps inside the bias correction there)
    p2 = torch.tensor(theta0["a/b"], requires_grad=True)
    tadam = torch.optim.Adam([p2], lr=lr, betas=(b1, b2), eps=eps)
    for g in grads:
        p2.grad = torch.tensor(g["a/b"])
        tadam.step()
    assert not np.array_equal(p2.detach().numpy(), params["a/b"].numpy())


# ------------------------------------------------------------------------------------------------ GPU

SMALL_CASES = [  # (batchnorm, alpha, action_box, with_v)
    (True, 0.0, False, True),
    (False, 0.0, False, True),
    (True, 0.01, False, True),
    (False, 0.01, True, True),
    (True, 0.0, True, True),
    (True, 0.0, False, False),
    (False, 0.01, True, False),
]


@pytest.mark.gpu
@pytest.mark.parametrize("bn,alpha,box,with_v", SMALL_CASES)
@pytest.mark.parametrize("seed", [0, 1000])
def test_small_every_variable_matches_float64_double_backward(bn, alpha, box, with_v, seed):
    from icnn_amd import bundle_entropy, train
    spec = _small_spec(bn, alpha, box)
    p = _small_problem(spec, seed, with_v)
    model = picnn.FCModel(spec, p["params"], "cuda")
    dev = model.device
    R = len(p["samp"])
    y = torch.from_numpy(p["y"]).to(dev)
    c = torch.from_numpy(p["c"]).to(dev)
    v = torch.from_numpy(p["v"]).to(dev) if with_v else None
    F = torch.empty(R, dtype=torch.float32, device=dev)
    if with_v:      # the feed form implicit_feed returns
        feed = bundle_entropy.ImplicitFeed(torch.from_numpy(p["samp"].astype(np.int32)).to(dev), y, v, c)
        g = train.surrogate_grad(model, torch.from_numpy(p["x"]), feed, F_rows=F)
    else:
        g = train.surrogate_grad(model, torch.from_numpy(p["x"]), (y, None, c), row_offset=_offsets(p["counts"]), F_rows=F)
    torch.cuda.synchronize()
    assert list(g.keys()) == list(picnn.init_params(spec).keys())
    worst = []
    for k, ref in p["g64"].items():
        got = g[k].double().cpu().numpy()
        assert got.shape == ref.shape, k
        err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
        worst.append((err / max(scale, 1e-30), k))
        assert err <= 1e-4 * scale + 1e-7, (k, err, scale)
    Fd = F.double().cpu().numpy()
    assert np.max(np.abs(Fd - p["F64"])) <= 1e-5 * np.max(np.abs(p["F64"]))
    print("worst relative error %.2e (%s)" % max(worst))


@pytest.mark.gpu
def test_rl_critic_form_one_row_per_sample():
    """(y, c) with one row per sample: the RL critic's gradient of sum_r c_r Q-energy (RL/src/icnn.py:90-109)."""
    from icnn_amd import train
    spec = picnn.FCSpec(17, 6, (200, 200), alpha=0.01, batchnorm=False, action_box=True)
    rng = np.random.RandomState(7)
    params = picnn.init_params(spec, 7, "init", yu_bias=1.0, gate_bias=1.0)
    B = 64
    x = rng.randn(B, 17).astype(np.float32)
    y = rng.rand(B, 6)
    c = rng.randn(B)
    g64, _, _ = train_ref.surrogate_grad64(spec, params, x, y, None, c)
    model = picnn.FCModel(spec, params, "cuda")
    g = train.surrogate_grad(model, torch.from_numpy(x), (torch.from_numpy(y).cuda(), torch.from_numpy(c).cuda()))
    for k, ref in g64.items():
        got = g[k].double().cpu().numpy()
        assert np.linalg.norm(got - ref) <= 1e-3 * np.linalg.norm(ref) + 1e-7, k


def _bibtex_feed():
    from icnn_amd import bundle_entropy
    spec = picnn.bibtex_spec()
    params = picnn.init_params(spec, 0, "spread")
    B = 128
    rng = np.random.RandomState(0)
    x = (rng.rand(B, spec.n_features) < 0.04).astype(np.float32)
    labels = (rng.rand(B, spec.n_labels) < 0.05).astype(np.float64)
    model = picnn.FCModel(spec, params, "cuda")
    ctx = model.context(torch.from_numpy(x))
    res = bundle_entropy.FusedSolver(model, B, 10, "dual").solve(ctx, 0.5)
    feed = bundle_entropy.implicit_feed(res, labels, "xent")
    return spec, params, model, x, feed


@pytest.mark.gpu
def test_bibtex_end_to_end_against_float64():
    from icnn_amd import train
    spec, params, model, x, feed = _bibtex_feed()
    g = train.surrogate_grad(model, torch.from_numpy(x), feed)
    torch.cuda.synchronize()
    samp = feed.sample.cpu().numpy()
    R = len(samp)
    assert R > 128
    g64, _, margin = train_ref.surrogate_grad64(spec, params, x[samp], feed.y.cpu().numpy(), feed.v.cpu().numpy(),
                                                feed.c.cpu().numpy())
    ratios = {}
    for k, ref in g64.items():
        got = g[k].double().cpu().numpy()
        ratios[k] = float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))
    print("bibtex R = %d, min |pre-activation| %.2e" % (R, margin))
    for k, r in ratios.items():
        print("  %-16s |g - g64|_F / |g64|_F = %.2e" % (k, r))
    # The final layer's x-only term 'z{L}_u' has the gradient sum_r c_r [u_{L-1}(x_r), 1]: the c of one sample's rows are the
    # adjoints of multipliers constrained to sum to one (the dual's simplex), so they sum to zero per sample and these two
    # gradients are pure rounding residue of the float32 feed -- compared against the size of the terms that cancel instead
    L = len(spec.szs)
    c = feed.c.cpu().numpy().astype(np.float32).astype(np.float64)
    per_sample = np.bincount(samp, weights=c, minlength=x.shape[0])
    per_sample_abs = np.bincount(samp, weights=np.abs(c), minlength=x.shape[0])
    assert np.all(np.abs(per_sample) <= 1e-5 * per_sample_abs + 1e-12)
    u_last = train_ref.last_u(spec, params, x[samp])
    terms = {"z%d_u/b" % L: np.sum(np.abs(c)), "z%d_u/W" % L: np.sum(np.abs(c) * np.linalg.norm(u_last, axis=1))}
    for k, size in terms.items():
        err = float(np.linalg.norm(g[k].double().cpu().numpy() - g64[k]))
        print("  %-16s |g - g64|_F = %.2e against cancelling terms of size %.2e (%.2e)" % (k, err, size, err / size))
        assert err <= 1e-5 * size, (k, err, size)
        del ratios[k]
    bad = {k: r for k, r in ratios.items() if not r <= 1e-3}
    assert not bad, bad


@pytest.mark.gpu
def test_bitwise_repeatable_and_graph_capturable():
    from icnn_amd import train
    spec, params, model, x, feed = _bibtex_feed()
    xd = torch.from_numpy(x).cuda()
    B = x.shape[0]
    offs = torch.searchsorted(feed.sample, torch.arange(B + 1, dtype=torch.int32, device="cuda"), out_int32=True)
    rows = (feed.y, feed.v, feed.c)

    def flat(g):
        return torch.cat([t.reshape(-1) for t in g.values()])
    a = flat(train.surrogate_grad(model, xd, rows, row_offset=offs)).clone()
    b = flat(train.surrogate_grad(model, xd, rows, row_offset=offs)).clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        train.surrogate_grad(model, xd, rows, row_offset=offs)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = train.surrogate_grad(model, xd, rows, row_offset=offs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(flat(out), a)


@pytest.mark.gpu
@pytest.mark.parametrize("with_v", [True, False])
def test_doubling_every_multiplicity_doubles_the_gradient(with_v):
    from icnn_amd import train
    spec = _small_spec(True, 0.0, False)
    p = _small_problem(spec, 0, with_v)
    model = picnn.FCModel(spec, p["params"], "cuda")
    counts, samp = p["counts"], p["samp"]
    idx = np.concatenate([np.concatenate([np.flatnonzero(samp == j)] * 2) for j in range(len(counts))])
    x = torch.from_numpy(p["x"])

    def run(sel, offs):
        y = torch.from_numpy(p["y"][sel]).cuda()
        v = torch.from_numpy(p["v"][sel]).cuda() if with_v else None
        c = torch.from_numpy(p["c"][sel]).cuda()
        return train.surrogate_grad(model, x, (y, v, c), row_offset=offs)
    g1 = run(np.arange(len(samp)), _offsets(counts))
    g2 = run(idx, _offsets(2 * counts))
    torch.cuda.synchronize()
    for k in g1:
        two = 2 * g1[k].double()
        assert float((g2[k].double() - two).abs().max()) <= 1e-5 * float(two.abs().max()) + 1e-12, k
