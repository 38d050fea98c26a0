"""The FICNN of synthetic-cls/icnn.py (icnn_amd.ficnn, be_ficnn.hip): the reference's never-reassigned z, the host
layouts and argument checks of the C entries, and on the device E / dE/dy against float64, the GD loop bit for bit against
a loop of fg plus the float32 recurrence, and solveBatch(f=model) against the generic path."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import ficnn_ref
import gd_ref
from icnn_amd import _lib, ficnn, train

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_ficnn_pack_floats", "icnn_be_ficnn_pack", "icnn_be_ficnn_context_work_floats", "icnn_be_ficnn_context",
               "icnn_be_ficnn_fg", "icnn_be_ficnn_gd", "icnn_be_solve_ficnn", "icnn_be_ficnn_grad_floats",
               "icnn_be_ficnn_surrogate_grad_work_floats", "icnn_be_ficnn_surrogate_grad"]
F32 = 2.0 ** -24


def _struct(spec, wpack=64):
    m = _lib.FicnnModel()
    m.n_features, m.n, m.n_layers = spec.n_features, spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.head = _lib.FICNN_HEAD[spec.head]
    m.ctx_width = spec.ctx_width
    m.wpack = wpack
    return m


def _kblocks(K):
    return (-(-K // 16) + 4) // 5 * 5


def _packed(K, N):
    return _kblocks(K) * (-(-N // 16)) * 256


def _a64(v):
    return -(-v // 64) * 64


def _pack_floats(spec):
    """host restatement of the pack layout of include/icnn_be.h / be_ficnn_dev.h"""
    w, n, nf, C_ = spec.widths, spec.n_labels, spec.n_features, spec.ctx_width
    t = _a64(nf * C_) + _a64(C_)
    for i in range(len(spec.szs)):
        t += _a64(_packed(n, w[i])) + _a64(_packed(w[i], n))
        if i > 0:
            t += _a64(_packed(w[i - 1], w[i])) + _a64(_packed(w[i], w[i - 1]))
    if spec.head == "linear":
        t += _a64(-(-n // 16) * 16) + _a64(-(-w[-2] // 16) * 16)
    return t


SPECS = [ficnn.synthetic_spec(), ficnn.synthetic_spec("linear"), ficnn.FICNNSpec(5, 17, (15, 16, 17), "linear"),
         ficnn.FICNNSpec(3, 1, (64,), "sum"), ficnn.FICNNSpec(4, 5, (65, 129, 7, 9, 11, 13, 15), "sum"),
         ficnn.FICNNSpec(1836, 159, (600, 600), "linear")]


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("szs", [(200, 200), (7,), (5, 6, 7)])
def test_reference_loop_is_the_sum_head(szs):
    """f_ficnn as written returns the last hidden layer; the energy tf.gradients differentiates is its sum."""
    spec = ficnn.FICNNSpec(2, 1, szs)
    p = ficnn_ref.wide_params(spec, 1)
    theta = {k: torch.tensor(v, dtype=torch.float64) for k, v in p.items()}
    rng = np.random.RandomState(0)
    x = torch.tensor(rng.randn(9, 2))
    y = torch.tensor(rng.rand(9, 1))
    z = ficnn_ref.reference_loop(spec, theta, x, y)
    assert z.shape == (9, szs[-1])
    E, _ = ficnn_ref.energy(spec, theta, x, y)
    assert torch.equal(z.sum(1), E)


@pytest.mark.parametrize("spec", SPECS, ids=lambda s: "%s-%s" % (s.szs, s.head))
def test_layouts_agree_with_the_library(spec):
    lib = _lib.load()
    m = _struct(spec)
    layout = train.grad_layout(spec)
    assert [k for k, _ in layout] == list(ficnn.init_params(spec).keys())
    assert lib.icnn_be_ficnn_grad_floats(C.byref(m)) == sum(int(np.prod(s)) for _, s in layout)
    assert lib.icnn_be_ficnn_pack_floats(C.byref(m)) == _pack_floats(spec)


@pytest.mark.parametrize("spec", SPECS[:5], ids=lambda s: "%s-%s" % (s.szs, s.head))
def test_param_map_and_pack_is_a_copy(spec):
    """ParamMap builds through the index image: every packed float is one parameter element or padding, and every
    variable the kernels read lands in the pack (the unused head of 'sum' does not)"""

    class Host:                       # the arena hooks of FICNNModel without a device
        pass
    h = Host()
    h.spec, h._lib, h.c_model = spec, _lib.load(), _struct(spec, None)
    h.n_pack_floats = h._lib.icnn_be_ficnn_pack_floats(C.byref(h.c_model))
    h._pack_host = lambda params: ficnn.FICNNModel._pack_host(h, params)
    h.arena_parts = lambda params: ficnn.FICNNModel.arena_parts(h, params)
    pm = train.ParamMap(h)
    counts = np.diff(pm.dest_off)
    at = 0
    for name, shape in train.grad_layout(spec):
        size = int(np.prod(shape))
        used = counts[at:at + size]
        head = name.startswith("z_x%d/" % len(spec.szs)) or name.startswith("z_z%d_" % len(spec.szs))
        if head and spec.head == "sum":
            assert used.max() == 0, name
        elif name.endswith("/W") and name.startswith("z_x"):
            assert used.min() >= 1, name
        at += size
    assert [pm.proj[i][1] - pm.proj[i][0] for i in range(len(pm.proj))] == \
        [spec.widths[i - 1] * spec.widths[i] for i in range(1, spec.n_layers)]


def test_argument_checks_before_launch():
    lib = _lib.load()
    spec = ficnn.synthetic_spec()
    dummy = C.c_void_p(64)
    good = _struct(spec)
    st = _lib.State()
    for bad in [dict(head=2), dict(ctx_width=401), dict(n_layers=1), dict(width=(200, 200, 2)), dict(n=0)]:
        m = _struct(spec)
        for k, v in bad.items():
            if k == "width":
                for i, w in enumerate(v):
                    m.width[i] = w
            else:
                setattr(m, k, v)
        assert lib.icnn_be_ficnn_pack_floats(C.byref(m)) == 0, bad
        assert lib.icnn_be_ficnn_fg(C.byref(m), dummy, dummy, 4, dummy, dummy, None, None) == -1, bad
        assert lib.icnn_be_ficnn_grad_floats(C.byref(m)) == 0, bad
    m = _struct(spec)
    m.n_layers = 9
    assert lib.icnn_be_ficnn_fg(C.byref(m), dummy, dummy, 4, dummy, dummy, None, None) == -2
    wide = _struct(ficnn.FICNNSpec(2, 1, (4000, 4000)))
    assert lib.icnn_be_ficnn_pack_floats(C.byref(wide)) == 0
    assert lib.icnn_be_ficnn_fg(C.byref(wide), dummy, dummy, 4, dummy, dummy, None, None) == -2
    assert lib.icnn_be_ficnn_fg(C.byref(good), None, dummy, 4, dummy, dummy, None, None) == -1
    assert lib.icnn_be_ficnn_fg(C.byref(good), dummy, dummy, -1, dummy, dummy, None, None) == -1
    assert lib.icnn_be_ficnn_fg(C.byref(good), dummy, dummy, 0, dummy, dummy, None, None) == 0
    assert lib.icnn_be_ficnn_gd(C.byref(good), dummy, dummy, 4, 0, 0.01, 0.9, dummy, None, None, dummy, None) == -1
    assert lib.icnn_be_ficnn_gd(C.byref(good), dummy, dummy, 4, 3, float("nan"), 0.9, dummy, None, None, dummy, None) == -1
    assert lib.icnn_be_ficnn_context(C.byref(good), dummy, 4, None, dummy, None) == -1
    assert lib.icnn_be_solve_ficnn(C.byref(good), dummy, C.byref(st), dummy, dummy, None) == -1
    assert lib.icnn_be_ficnn_surrogate_grad(C.byref(good), dummy, 0, dummy, 4, dummy, None, dummy, dummy, None, dummy,
                                            None) == -1
    assert lib.icnn_be_ficnn_surrogate_grad(C.byref(good), dummy, 4, dummy, 4, None, None, dummy, dummy, None, dummy,
                                            None) == -1
    assert lib.icnn_be_ficnn_surrogate_grad_work_floats(C.byref(good), 4, 0) == 0
    assert lib.icnn_be_ficnn_surrogate_grad_work_floats(C.byref(good), 4, 120) > 0
    assert lib.icnn_be_ficnn_context_work_floats(C.byref(good), -1) == 0


def test_exports_and_struct_size():
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    lib = _lib.load()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.icnn_be_struct_size(8) == C.sizeof(_lib.FicnnModel) == 64      # 13 ints, padding, wpack
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()


# ------------------------------------------------------------------------------------------------ GPU

MARGIN = 1e-4


def _problem(spec, B, seed, rows=None):
    rng = np.random.RandomState(seed)
    p = ficnn_ref.wide_params(spec, seed)
    x = rng.randn(B, spec.n_features).astype(np.float32)
    y = rng.rand(B, spec.n_labels).astype(np.float32).astype(np.float64)
    return p, x, y


def _check_fg(spec, B, seed, subset=None):
    p, x, y = _problem(spec, B, seed)
    model = ficnn.FICNNModel(spec, p)
    xd = torch.from_numpy(x).cuda()
    ctx = model.context(xd)
    yd = torch.from_numpy(y).cuda()
    f, g = model.fg(ctx, yd)
    f2, g2 = model.fg(ctx, yd)
    assert torch.equal(f, f2) and torch.equal(g, g2), "second call differs"
    f, g = f.cpu().numpy(), g.cpu().numpy()
    rows = np.arange(B) if subset is None else subset
    E, G, margin, Ea, Ga = ficnn_ref.fg64(spec, p, x[rows], y[rows])
    depth = 4 * (spec.n_layers + 1) * (spec.n_features + spec.n_labels + max(spec.szs))
    ok = margin > MARGIN
    assert ok.mean() > 0.5, ok.mean()
    tolE = depth * F32 * (Ea + 1e-30)
    tolG = depth * F32 * (Ga + 1e-30)
    errE = np.abs(f[rows] - E)
    errG = np.abs(g[rows] - G)
    assert (errE[ok] <= tolE[ok]).all(), (errE[ok].max(), tolE[ok].min())
    assert (errG[ok] <= tolG[ok]).all(), ((errG - tolG)[ok].max())
    return model, ctx, yd


FG_CASES = [(ficnn.synthetic_spec(), 100), (ficnn.synthetic_spec(), 400), (ficnn.synthetic_spec("linear"), 100),
            (ficnn.synthetic_spec("linear"), 400),
            (ficnn.FICNNSpec(3, 1, (15, 16, 17), "sum"), 17), (ficnn.FICNNSpec(3, 5, (64, 65, 129), "linear"), 16),
            (ficnn.FICNNSpec(2, 17, (129,), "sum"), 15), (ficnn.FICNNSpec(2, 17, (16,), "linear"), 1),
            (ficnn.FICNNSpec(4, 5, (65, 17, 16, 15, 64, 129, 33), "sum"), 1000),
            (ficnn.FICNNSpec(4, 5, (65, 17, 16, 15, 64, 129, 33), "linear"), 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("spec,B", FG_CASES, ids=lambda v: str(v) if isinstance(v, int) else "%s-%s" % (v.szs, v.head))
def test_fg_against_float64(spec, B):
    _check_fg(spec, B, B)


@pytest.mark.gpu
def test_fg_large_spec_on_a_subset():
    spec = ficnn.FICNNSpec(1836, 159, (600, 600), "linear")
    _check_fg(spec, 4096, 7, subset=np.r_[0:20, 2040:2060, 4080:4096])


@pytest.mark.gpu
def test_fg_leaves_finished_samples_untouched():
    spec = ficnn.synthetic_spec()
    p, x, y = _problem(spec, 40, 3)
    model = ficnn.FICNNModel(spec, p)
    ctx = model.context(torch.from_numpy(x).cuda())
    yd = torch.from_numpy(y).cuda()
    fin = torch.zeros(40, dtype=torch.int32, device="cuda")
    fin[5:30] = 1                                       # tile 1 (16..31) all but two rows, and every row of ...
    fin[16:32] = 1                                      # ... tile 1 after all: that tile must not run at all
    f = torch.full((40,), 7.0, device="cuda")
    g = torch.full((40, 1), 9.0, device="cuda")
    model.fg_into(ctx, yd, f, g, fin)
    f0, g0 = model.fg(ctx, yd)
    keep = fin.bool()
    assert (f[keep] == 7.0).all() and (g[keep] == 9.0).all()
    assert torch.equal(f[~keep], f0[~keep]) and torch.equal(g[~keep], g0[~keep])


@pytest.mark.gpu
@pytest.mark.parametrize("spec,B", [(ficnn.synthetic_spec(), 100), (ficnn.synthetic_spec("linear"), 37),
                                    (ficnn.FICNNSpec(3, 5, (64, 65), "sum"), 1000)],
                         ids=["synthetic-100", "linear-37", "wide-1000"])
def test_gd_is_a_loop_of_fg_and_the_float32_update(spec, B):
    from icnn_amd import gd
    p, x, _ = _problem(spec, B, 11)
    p = ficnn.make_convex(ficnn.init_params(spec, 11)) if B == 100 else p
    model = ficnn.FICNNModel(spec, p)
    ctx = model.context(torch.from_numpy(x).cuda())
    y0 = np.random.RandomState(2).rand(B, spec.n_labels)
    K, lr, mu = 30, 0.01, 0.9

    def fg(yy):
        f, g = model.fg(ctx, torch.from_numpy(np.ascontiguousarray(yy)).cuda())
        return f.cpu().numpy(), g.cpu().numpy()
    yK, traj, E = gd_ref.unroll_f32(fg, y0, K, lr, mu)
    y, tr, f = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True, energy=True)
    assert np.array_equal(y.cpu().numpy(), yK.astype(np.float64))
    assert np.array_equal(tr.cpu().numpy(), traj)
    assert np.array_equal(f.cpu().numpy(), E)
    assert np.abs(yK - y0).max() > 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_solve_batch_fused_equals_generic(variant):
    from icnn_amd import bundle_entropy
    spec = ficnn.synthetic_spec("linear")
    B = 64
    p, x, _ = _problem(spec, B, 5)
    model = ficnn.FICNNModel(spec, p)
    ctx = model.context(torch.from_numpy(x).cuda())
    y0 = np.full((B, 1), 0.5)
    fused = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=y0.copy(), nIter=10, variant=variant, native=True, check=False)
    gen = bundle_entropy.solveBatch(lambda yy: model.fg(ctx, yy), torch.from_numpy(y0.copy()).cuda(), 10, variant=variant,
                                    fg_on_device=True, native=True, check=False)
    assert torch.equal(fused.y[:B], gen.y[:B])
    assert torch.equal(fused.status[:B], gen.status[:B])
    from oracle import bundle_entropy_oracle as bo

    def fg_host(yy):
        f, g = model.fg(ctx, torch.from_numpy(np.ascontiguousarray(yy)).cuda())
        return f.cpu().numpy(), g.cpu().numpy()
    ora = bo.solve_batch(fg_host, y0.copy(), 10, variant=variant)
    dy = np.abs(np.asarray(ora.y) - fused.y[:B].cpu().numpy()).max(1)
    assert (dy < 1e-5).mean() >= 0.9, np.sort(dy)[-8:]
