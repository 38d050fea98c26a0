"""The FICNN kernels (be_ficnn.hip, be_train_ficnn.hip) across the shapes the ABI accepts, beyond the one or two shapes of
tests/test_ficnn.py and tests/test_ficnn_train.py: the surrogate gradient and F_r at every depth, at widths that straddle
a 16-column tile, at label counts past one and two 64-lane passes, on row layouts with empty samples, one long sample
and split-K weight products; GD bit for bit at n > 64, K = 1 and partial tiles; the 160 KB LDS limit of the evaluation
tile (restated on the host, and run at the widest model it admits); solveBatch(f=FICNNModel) at n > 1 in every variant
and schedule; and the trainer's step at other batches, iteration counts and specs."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

import ficnn_ref
import gd_ref
from gemm_ref import MAX_SPLITS, gemm_splits
from gpu_util import result_to_host
from icnn_amd import _lib, ficnn, gd, train
from test_ficnn import _check_fg, _kblocks, _struct
from test_ficnn_train import _host_step, _moons

Spec = ficnn.FICNNSpec
MARGIN = 1e-4
HEADS = ["sum", "linear"]


def _head(spec, head):
    return dataclasses.replace(spec, head=head)


def _head_vars(spec):
    L = len(spec.szs)
    return lambda k: k.startswith("z_x%d/" % L) or k.startswith("z_z%d_" % L)


# ------------------------------------------------------------------------------------------------ LDS restatement

TM = 16                          # samples per evaluation tile (be_picnn_fc_dev.h)
LDS_BYTES = 160 * 1024           # the LDS of one workgroup on gfx950


def lds_pitch(width):
    """be_picnn_fc_dev.h lds_pitch: the padded k-blocks, then up to == 8 (mod 64) in steps of 4"""
    p = _kblocks(width) * 16
    while p % 64 != 8:
        p += 4
    return p


def ficnn_lds_bytes(spec):
    """be_ficnn_dev.h ficnn_lds: y | dE/dy | z_0 .. z_{L-1} | delta_{L-1}, TM rows each"""
    floats = 2 * TM * lds_pitch(spec.n_labels) + sum(TM * lds_pitch(w) for w in spec.szs) + TM * lds_pitch(spec.szs[-1])
    return 4 * floats


def widest(family, top=6000):
    """the largest w with family(w) inside the LDS (the tile only grows with w)"""
    w = 1
    while w < top and ficnn_lds_bytes(family(w + 1)) <= LDS_BYTES:
        w += 1
    assert w < top
    return w


LDS_FAMILIES = {
    "one_layer_n1": lambda w: Spec(2, 1, (w,)),
    "two_layers_n5": lambda w: Spec(3, 5, (w, w), "linear"),
    "first_of_three": lambda w: Spec(4, 3, (w, 64, 32)),
    "labels": lambda w: Spec(2, w, (16,)),
}


# ------------------------------------------------------------------------------------------------ CPU


def test_lds_restatement_matches_the_shipped_shapes():
    # the synthetic-cls model, and the widest spec tests/test_ficnn.py evaluates (150 KB of the 160)
    assert ficnn_lds_bytes(ficnn.synthetic_spec()) == 4 * TM * (2 * 136 + 3 * 264)
    assert ficnn_lds_bytes(Spec(1836, 159, (600, 600))) == 4 * TM * (2 * 200 + 3 * 648)
    assert all(lds_pitch(w) % 64 == 8 and lds_pitch(w) >= _kblocks(w) * 16 for w in range(1, 700))


def test_lds_boundary_of_one_hidden_layer_is_1040():
    # 2 * 16 * 136 for y and dE/dy, 2 * 16 * pitch(w) for z_0 and delta_0: pitch(1040) = 1096 fits, pitch(1041) = 1160 not
    assert widest(LDS_FAMILIES["one_layer_n1"]) == 1040


def _accepted(lib, spec):
    """whether the FICNN entries accept spec, asked before any launch (batch 0 and shape queries); they must all agree"""
    m = _struct(spec)
    dummy = C.c_void_p(64)
    fg = lib.icnn_be_ficnn_fg(C.byref(m), dummy, dummy, 0, dummy, dummy, None, None)
    gdr = lib.icnn_be_ficnn_gd(C.byref(m), dummy, dummy, 0, 3, 0.01, 0.9, dummy, None, None, dummy, None)
    assert fg in (0, -2) and gdr == fg, (fg, gdr)
    ok = fg == 0
    assert (lib.icnn_be_ficnn_pack_floats(C.byref(m)) > 0) == ok
    assert (lib.icnn_be_ficnn_grad_floats(C.byref(m)) > 0) == ok
    assert (lib.icnn_be_ficnn_surrogate_grad_work_floats(C.byref(m), 4, 8) > 0) == ok
    assert (lib.icnn_be_ficnn_context_work_floats(C.byref(m), 4) > 0) == ok
    return ok


@pytest.mark.parametrize("family", sorted(LDS_FAMILIES))
def test_lds_limit_is_where_the_restatement_puts_it(family):
    """The widest model of the family whose tile fits 160 KB is accepted by every entry, the next width is refused with
    ICNN_BE_ELIMIT before any launch."""
    lib = _lib.load()
    make = LDS_FAMILIES[family]
    w = widest(make)
    assert ficnn_lds_bytes(make(w)) <= LDS_BYTES < ficnn_lds_bytes(make(w + 1))
    assert _accepted(lib, make(w)), (family, w)
    assert not _accepted(lib, make(w + 1)), (family, w + 1)
    assert _accepted(lib, make(w // 2))


def test_split_plan_of_the_large_feed():
    """The split_k feed of test_surrogate_grad_row_layouts: every weight-gradient product (K = 2R with v, R without) is
    cut into the 32 splits with a short last chunk; the context product (K = B) is not split."""
    spec, counts = _split_feed()
    R = int(counts.sum())
    w = spec.szs
    for K in (2 * R, R):
        products = [(spec.n_labels, wi) for wi in w] + [(w[i - 1], w[i]) for i in range(1, len(w))]
        for M, N in products:
            splits, kchunk = gemm_splits(M, N, K)
            assert splits == MAX_SPLITS and K % kchunk != 0, (M, N, K, splits, kchunk)
    assert gemm_splits(spec.n_features, w[0], len(counts))[0] == 1


# ------------------------------------------------------------------------------------------------ GPU: surrogate gradient

GRAD_SPECS = {
    "L1_n1": Spec(3, 1, (17,)),                                     # one hidden layer
    "deep8_n16": Spec(4, 16, (15, 16, 17, 63, 65, 129, 33)),        # n_layers = 8 = ICNN_BE_MAX_LAYERS
    "n17": Spec(5, 17, (129, 63, 16)),
    "n65": Spec(3, 65, (65, 15)),
    "n159": Spec(1836, 159, (600, 600)),                            # the multi-label width, modest R
}
EMPTY_FIRST_MIDDLE_LAST = np.array([0, 3, 1, 0, 2, 5, 0])


def _split_feed():
    """a few thousand rows on a small model: K = 2R = 5000 = 31 chunks of 160 + 40 (R: 32 chunks, the last 20)"""
    counts = 45 + (np.arange(40) * 13) % 35
    counts[-1] += 2500 - counts.sum()
    return Spec(3, 3, (6, 5)), counts


def _screened_rows(spec, params, x, counts, seed):
    """rows y (float32 values) drawn until no float64 hidden pre-activation lies within MARGIN of zero: the ReLU masks of
    the kernels and of float64 must agree"""
    rng = np.random.RandomState(seed)
    samp = np.repeat(np.arange(len(counts)), counts)
    y = rng.rand(len(samp), spec.n_labels).astype(np.float32).astype(np.float64)
    for _ in range(100):
        margin = ficnn_ref.fg64(spec, params, x[samp], y)[2]
        bad = margin <= MARGIN
        if not bad.any():
            return y
        y[bad] = rng.rand(int(bad.sum()), spec.n_labels).astype(np.float32)
    raise AssertionError("no screened rows")


def _check_surrogate(spec, counts, with_v, seed):
    counts = np.asarray(counts)
    params = ficnn_ref.wide_params(spec, seed)
    rng = np.random.RandomState(seed + 1)
    B = len(counts)
    x = rng.randn(B, spec.n_features).astype(np.float32)
    y = _screened_rows(spec, params, x, counts, seed + 2)
    R = y.shape[0]
    v = rng.randn(R, spec.n_labels) if with_v else None
    c = rng.randn(R)
    ref, F64 = ficnn_ref.surrogate_grad64(spec, params, x, counts, y, v, c)
    model = ficnn.FICNNModel(spec, params)
    off = torch.tensor(np.r_[0, np.cumsum(counts)], dtype=torch.int32, device="cuda")
    yd, cd = torch.from_numpy(y).cuda(), torch.from_numpy(c).cuda()
    rows = (yd, torch.from_numpy(v).cuda(), cd) if with_v else (yd, None, cd)
    xd = torch.from_numpy(x).cuda()
    outs = []
    for _ in range(2):
        F = torch.empty(R, dtype=torch.float32, device="cuda")
        outs.append((train.surrogate_grad(model, xd, rows, row_offset=off, F_rows=F, flat=True), F))
    (g, F), (g2, F2) = outs
    torch.cuda.synchronize()
    assert torch.equal(g, g2) and torch.equal(F, F2), "second call differs"
    got = {k: t.cpu().numpy() for k, t in train.unpack_grad(spec, g).items()}
    head = _head_vars(spec)
    worst, bad = (0.0, ""), []
    for k in params:
        scale = float(np.abs(ref[k]).max())
        if spec.head == "sum" and head(k):
            assert scale == 0 and not got[k].any(), k
            continue
        err = float(np.abs(got[k] - ref[k]).max())
        worst = max(worst, (err / max(scale, 1e-30), k))
        if not err <= 1e-4 * scale + 1e-6:
            bad.append((k, err, scale))
    Ferr = float(np.abs(F.double().cpu().numpy() - F64).max())
    print("%s R=%d: worst relative error %.2e (%s), F_r %.2e" % (spec, R, worst[0], worst[1], Ferr / np.abs(F64).max()))
    assert not bad, bad
    assert Ferr <= 1e-5 * np.abs(F64).max(), Ferr
    return R


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("with_v", [True, False], ids=["v", "no_v"])
@pytest.mark.parametrize("name", list(GRAD_SPECS))
def test_surrogate_grad_every_variable(name, with_v, head):
    spec = _head(GRAD_SPECS[name], head)
    counts = [0, 4, 0, 3, 1, 0] if spec.n_labels > 100 else EMPTY_FIRST_MIDDLE_LAST
    _check_surrogate(spec, counts, with_v, 10 + len(spec.szs))


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("with_v", [True, False], ids=["v", "no_v"])
@pytest.mark.parametrize("layout", ["one_sample", "long_sample", "split_k"])
def test_surrogate_grad_row_layouts(layout, with_v, head):
    if layout == "one_sample":
        spec, counts = GRAD_SPECS["deep8_n16"], [6]
    elif layout == "long_sample":                                   # one sample of 1200 rows between short ones
        spec, counts = GRAD_SPECS["n17"], [2, 1200, 0, 3]
    else:
        spec, counts = _split_feed()
    R = _check_surrogate(_head(spec, head), counts, with_v, 30)
    assert R == sum(counts)


# ------------------------------------------------------------------------------------------------ GPU: GD


def _check_gd_loop(model, ctx, y0, K, lr=0.01, mu=0.9):
    """gd.solve against gd_ref.unroll_f32 around model.fg, bit for bit: y_K, the trajectory, E(y_K); and y_K alone"""
    def fg(yy):
        f, g = model.fg(ctx, torch.from_numpy(np.ascontiguousarray(yy)).cuda())
        return f.cpu().numpy(), g.cpu().numpy()
    yK, traj, E = gd_ref.unroll_f32(fg, y0, K, lr, mu)
    y, tr, f = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True, energy=True)
    assert np.array_equal(y.cpu().numpy(), yK.astype(np.float64))
    assert np.array_equal(tr.cpu().numpy(), traj)
    assert np.array_equal(f.cpu().numpy(), E)
    bare, none_t, none_f = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu)
    assert none_t is None and none_f is None
    assert torch.equal(bare, y)
    assert np.abs(yK - np.asarray(y0, np.float32)).max() > 1e-5
    return yK


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("K", [1, 30])
@pytest.mark.parametrize("B", [1, 17, 33, 1000])
@pytest.mark.parametrize("n", [17, 65, 159])
def test_gd_wide_labels_bit_for_bit(n, B, K, head):
    """n > 64: the init and update loops of ficnn_gd_kernel take a second (and third) pass over the lanes; B = 17, 33 end
    in a partial tile, with the trajectory written"""
    spec = Spec(3, n, (33, 17), head)
    p = ficnn_ref.wide_params(spec, n)
    rng = np.random.RandomState(B + K)
    model = ficnn.FICNNModel(spec, p)
    ctx = model.context(torch.from_numpy(rng.randn(B, 3).astype(np.float32)).cuda())
    _check_gd_loop(model, ctx, rng.rand(B, n), K)


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
def test_deep_unrolled_grad_against_float64_autograd(head):
    """five hidden layers: train.unrolled_grad on the device trajectory against float64 autograd through the unroll"""
    spec = Spec(3, 4, (24, 17, 16, 15, 20), head)
    K, lr, mu, B = 5, 0.05, 0.9, 6

    def energy(theta, x, y):
        return ficnn_ref.energy(spec, theta, x, y)
    for seed in range(40):
        params = ficnn_ref.wide_params(spec, seed)
        rng = np.random.RandomState(seed)
        x = rng.randn(B, 3).astype(np.float32)
        y0 = rng.rand(B, 4).astype(np.float32).astype(np.float64)
        t = rng.rand(B, 4)
        g64, yK, _, _, margin = gd_ref.unrolled_autograd(energy, params, x, y0, t, K, lr, mu)
        if margin > MARGIN:
            break
    else:
        raise AssertionError("no screened problem")
    assert np.abs(yK - y0).max() > 1e-3
    model = ficnn.FICNNModel(spec, params)
    xd = torch.from_numpy(x).cuda()
    y, traj, _ = gd.solve(model, model.context(xd), torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True)
    ybar = 2.0 * (y - torch.from_numpy(t).cuda()) / y.numel()
    g = train.unrolled_grad(model, xd, traj, ybar, lr, mu)
    torch.cuda.synchronize()
    head_var = _head_vars(spec)
    for k, ref in g64.items():
        got = g[k].double().cpu().numpy()
        err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
        if head == "sum" and head_var(k):
            assert scale == 0 and not got.any(), k
        assert err <= 1e-4 * scale + 1e-12, (k, err, scale)


# ------------------------------------------------------------------------------------------------ GPU: the LDS limit

LIMIT_CASES = [("one_layer_n1", 37), ("two_layers_n5", 33)]


@pytest.mark.gpu
@pytest.mark.parametrize("family,B", LIMIT_CASES, ids=[f for f, _ in LIMIT_CASES])
def test_widest_accepted_model_fg_and_gd(family, B):
    """the widest model of the family: fg against float64, and the persistent GD launch at the full tile against the loop
    of fg"""
    make = LDS_FAMILIES[family]
    w = widest(make)
    spec = make(w)
    assert ficnn_lds_bytes(spec) <= LDS_BYTES < ficnn_lds_bytes(make(w + 1))
    model, ctx, _ = _check_fg(spec, B, 3)
    _check_gd_loop(model, ctx, np.random.RandomState(4).rand(B, spec.n_labels), 12)


# ------------------------------------------------------------------------------------------------ GPU: solveBatch

B_SOLVE = 37                   # three tiles of 16, the last one partial


def _solve_problem(n, head):
    spec = Spec(4, n, (33, 17), head)
    p = ficnn_ref.wide_params(spec, n)
    model = ficnn.FICNNModel(spec, p)
    rng = np.random.RandomState(n)
    ctx = model.context(torch.from_numpy(rng.randn(B_SOLVE, 4).astype(np.float32)).cuda())
    y0 = 0.2 + 0.6 * rng.rand(B_SOLVE, n)
    return model, ctx, y0


def _fused(model, ctx, y0, variant, flags, n_iter=10):
    from icnn_amd import bundle_entropy
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=torch.from_numpy(y0.copy()).cuda(), nIter=n_iter, variant=variant,
                                    native=True, check=False, flags=flags)
    torch.cuda.synchronize()
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("variant", ["dual", "rl", "pdipm"])
def test_solve_batch_fused_equals_generic(variant, n, head):
    from icnn_amd import bundle_entropy
    model, ctx, y0 = _solve_problem(n, head)
    B = B_SOLVE
    fused = _fused(model, ctx, y0, variant, 0)
    gen = bundle_entropy.solveBatch(lambda yy: model.fg(ctx, yy), torch.from_numpy(y0.copy()).cuda(), 10, variant=variant,
                                    fg_on_device=True, native=True, check=False)
    torch.cuda.synchronize()
    assert torch.equal(fused.y[:B], gen.y[:B])
    assert torch.equal(fused.status[:B], gen.status[:B])
    assert np.abs(fused.y[:B].cpu().numpy() - y0).max() > 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("n", [5, 17])
@pytest.mark.parametrize("variant", ["dual", "rl"])
def test_solve_batch_time_sliced_equals_lockstep(variant, n, head):
    """what test_time_sliced_rounds_equal_lockstep_rounds promises: y, the active sets, nIters, the multipliers and the
    Newton counts bit for bit (the round count may differ)"""
    model, ctx, y0 = _solve_problem(n, head)
    B = B_SOLVE
    a = _fused(model, ctx, y0, variant, _lib.FLAG_TIME_SLICE)
    b = _fused(model, ctx, y0, variant, _lib.FLAG_LOCKSTEP)
    assert a.state.rounds >= b.state.rounds == 10
    ha, hb = result_to_host(a), result_to_host(b)
    assert np.array_equal(ha["y"][:B], hb["y"][:B])
    assert ha["active"] == hb["active"] and ha["n_iters"] == hb["n_iters"]
    assert all((p is None and q is None) or np.array_equal(p, q) for p, q in zip(ha["lam"], hb["lam"]))
    assert np.array_equal(ha["newton"], hb["newton"])


@pytest.mark.gpu
def test_solve_batch_sum_head_against_the_oracle():
    from oracle import bundle_entropy_oracle as bo
    model, ctx, y0 = _solve_problem(5, "sum")
    B = B_SOLVE
    fused = _fused(model, ctx, y0, "dual", 0)

    def fg_host(yy):
        f, g = model.fg(ctx, torch.from_numpy(np.ascontiguousarray(yy)).cuda())
        return f.cpu().numpy(), g.cpu().numpy()
    ora = bo.solve_batch(fg_host, y0.copy(), 10, variant="dual")
    dy = np.abs(np.asarray(ora.y) - fused.y[:B].cpu().numpy()).max(1)
    assert (dy < 1e-5).mean() >= 0.9, np.sort(dy)[-8:]


# ------------------------------------------------------------------------------------------------ GPU: GDTrainer

TRAINER_CASES = [(ficnn.synthetic_spec(), 1, 30), (ficnn.synthetic_spec(), 37, 30), (ficnn.synthetic_spec(), 257, 30),
                 (ficnn.synthetic_spec("linear"), 37, 12), (Spec(2, 1, (48, 33, 17), "linear"), 37, 30)]


def _trainer_data(spec, B, seed):
    x, t = _moons(B, seed)
    params = ficnn.make_convex(ficnn.init_params(spec, seed))
    return params, x, t


@pytest.mark.gpu
@pytest.mark.parametrize("spec,B,K", TRAINER_CASES,
                         ids=["B1", "B37", "B257", "linear_K12", "deep3_linear"])
def test_trainer_steps_against_host_restatement(spec, B, K):
    """two steps against _host_step with tests/test_ficnn_train.py's bounds"""
    params, x, t = _trainer_data(spec, B, B + K)
    tr = ficnn.GDTrainer(ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()}), B, n_iter=K)
    state, host = [None], {k: v.copy() for k, v in params.items()}
    for s in range(2):
        loss = float(tr.step(torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()).item())
        host, hloss = _host_step(spec, host, x, t, K, 0.01, 0.9, state)
        assert abs(loss - hloss) <= 1e-4 * hloss, (s, loss, hloss)
        dev = tr.host_params()
        for k in host:
            diff = np.abs(dev[k] - host[k]).max()
            assert diff <= 2e-5 + 1e-3 * np.abs(host[k]).max(), (s, k, diff)


@pytest.mark.gpu
def test_captured_step_at_a_partial_tile_replays_as_eager_steps():
    spec, B, K = ficnn.synthetic_spec(), 37, 12
    params, x, t = _trainer_data(spec, B, 5)
    xs, ts = torch.from_numpy(x).cuda(), torch.from_numpy(t).cuda()
    a = ficnn.GDTrainer(ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()}), B, n_iter=K)
    b = ficnn.GDTrainer(ficnn.FICNNModel(spec, {k: v.copy() for k, v in params.items()}), B, n_iter=K)
    k = 3
    la = [float(a.step(xs, ts).item()) for _ in range(k + 1)]
    b.step(xs, ts)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            loss = b.step()
    torch.cuda.current_stream().wait_stream(s)
    lb = []
    for _ in range(k):
        graph.replay()
        lb.append(float(loss.item()))
    torch.cuda.synchronize()
    assert la[1:] == lb
    assert torch.equal(a.opt.theta, b.opt.theta)
    assert a.t_steps == b.t_steps == k + 1
