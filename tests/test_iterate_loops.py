"""The iterate loop of momentum GD and PGD (be_gd_dev.h, be_gd_rows_dev.h, be_gd.hip, be_pgd.hip) at the shapes no other
module reaches: the ragged rows workgroup (two samples per workgroup, the last one holding one), both sides of the dispatch
edge (B = 512 / 513), PGD off the shipped nets, the conv form at other image sizes and at B = 17, and NaN / Inf containment
inside a shared rows workgroup, a shared 16-row tile and a shared conv launch.  Nothing here has a tolerance of its own: GD is
bit for bit against gd_ref.unroll_f32 around the kernel-order oracles, PGD lies within pgd_ref.y_tolerance and 8 ULP of its
scale around the screened restatement (test_pgd._check_against), and every oracle runs on the device's own context.

  1. CPU: the dispatch rule of rows_per_wg restated, and a table that says which form every FC batch of this module takes;
     the PGD entry's refusal of the box specs; the feed screen of section 3 on the host's context.
  2. GPU, FC: both rules at B = 257, 511, 512, 513, 528 on the small spec, n = 270 and n = 1; a sample's bits across forms.
  3. GPU, FC: PGD on the architecture family of test_fc_solve_architectures.py.
  4. GPU, conv: 32 x 32, 48 x 64 and 16 x 64 at B = 3 and 17, the optional outputs, a sample alone, scratch regrowth, graph
     replay and the forms of the start.
  5. GPU: one poisoned sample (a NaN start entry, a NaN or +Inf context entry) leaves every other sample's bits alone, in the
     three forms and under both rules; PGD's clip(y0) turns a NaN start entry into lo."""
import functools

import numpy as np
import pytest
import torch

import gd_ref
import pgd_ref
from icnn_amd import picnn
from oracle import picnn_conv_oracle, picnn_oracle
from pgd_ref import LO, ULP
from test_fc_solve_architectures import SPECS, TAME, _first_difference, _need_256_cus, _problem
from test_pgd import _check_against, _small_spec, _start
from test_solve_plan import CUS

FC_SPECS = dict(SPECS, small=_small_spec())
GD_K, GD_LR, GD_MU = 4, 0.05, 0.9
PGD_SCHEDULES = [(3, 0.1), (10, 0.001)]
EDGE_BATCHES = [257, 511, 512, 513, 528]
EDGE_SPECS = ["small", "n270", "L1_n1"]
FAMILY = ["L1_n1", "L1_n9", "n20_deep4", "n33", "n70", "n270", "deep8"]
FAMILY_BATCHES = [37, 530]
CROSS_BATCH, CROSS_SAMPLES, CROSS_PREFIXES = 513, (0, 255, 256, 512), (257, 512)
# containment: form -> (batch, the poisoned sample, the samples that share its workgroup / tile)
POISONED = {"rows": (300, 101, [100]), "tiles": (530, 37, [u for u in range(32, 48) if u != 37])}
CONV_SIZES = [(32, 32), (48, 64), (16, 64)]
CONV_BATCHES = [3, 17]
CONV_GD = (5, 0.01, 0.9)                 # K and the completion defaults of test_gd_conv.py
CONV_POISONED = (17, 5)


# ------------------------------------------------------------------------------------------------ 1. the dispatch rule


def form(B, cus=CUS):
    """rows_per_wg (be_picnn_fc_rows_dev.h) and the grids of launch_fc_gd_rule, restated: (form, samples per workgroup,
    workgroups, samples in the last workgroup)"""
    per_wg = -(-B // cus)
    if per_wg <= 2:
        wgs = -(-B // per_wg)
        return "rows", per_wg, wgs, B - per_wg * (wgs - 1)
    tiles = -(-B // 16)
    return "tiles", 16, tiles, B - 16 * (tiles - 1)


def fc_batches():
    """every FC batch size this module launches"""
    return sorted(set(EDGE_BATCHES) | set(FAMILY_BATCHES) | {CROSS_BATCH, 1} | set(CROSS_PREFIXES)
                  | {b for b, _, _ in POISONED.values()})


def test_fc_cases_reach_every_form():
    forms = {B: form(B) for B in fc_batches()}
    assert forms[37] == ("rows", 1, 37, 1)                             # one sample per workgroup
    assert forms[512] == ("rows", 2, 256, 2)                           # the last rows batch: every workgroup whole
    assert forms[257] == ("rows", 2, 129, 1) and forms[511] == ("rows", 2, 256, 1)        # the last workgroup holds one sample
    assert forms[513] == ("tiles", 16, 33, 1)                          # the first tile batch: a one-row last tile
    assert forms[528] == ("tiles", 16, 33, 16)                         # no partial tile
    assert forms[530] == ("tiles", 16, 34, 2)
    assert {f[:2] for f in forms.values()} == {("rows", 1), ("rows", 2), ("tiles", 16)}
    # the dispatch edge is where the restatement says it is, and nowhere else below it
    assert [form(B)[0] for B in (1, 256, 257, 512, 513)] == ["rows"] * 4 + ["tiles"]
    # a sample of the 513-batch in its prefixes: 256 is the lone sample of the ragged workgroup of 257, 255 the second of a pair
    assert form(257)[1:] == (2, 129, 1) and 256 // 2 == 128 and 255 % 2 == 1
    # containment: the poisoned sample and the neighbours named by the tests share a workgroup / a tile
    B, p, mates = POISONED["rows"]
    assert form(B)[:2] == ("rows", 2) and [m // 2 for m in mates] == [p // 2] and form(B)[3] == 2
    B, p, mates = POISONED["tiles"]
    assert form(B)[0] == "tiles" and len(mates) == 15 and {m // 16 for m in mates} == {p // 16}


def test_start_has_entries_outside_the_box():
    """the "random" start of test_pgd.py, at the label counts used here (n = 1 included), leaves the box on both sides"""
    for n in (1, 12, 270):
        y0 = _start("random", 257, n, 0)[1]
        assert y0.shape == (257, n) and (y0 < LO).any() and (y0 > 1.0).any()


@pytest.mark.parametrize("name", ["n8_box", "n16_box", "n17_box"])
def test_pgd_entry_refuses_the_box_specs(name):
    """as test_gd_entry_refuses_the_box_specs: refused before anything is launched (placeholder pointers), and by pgd.solve"""
    import ctypes as C
    from icnn_amd import _lib, pgd
    spec = SPECS[name]
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width, m.wpack = spec.alpha, 1, spec.ctx_width, 64
    fake = C.c_void_p(64)
    assert _lib.load().icnn_be_fc_pgd(C.byref(m), fake, fake, 37, 3, 0.1, LO, pgd_ref.HI, fake, None, None, fake, None) == -1

    class _M:
        pgd_entry = "icnn_be_fc_pgd"
    model = _M()
    model.spec, model.device = spec, torch.device("cpu")
    with pytest.raises(ValueError):
        pgd.solve(model, torch.zeros(3, spec.ctx_width), 0.5, 3, 0.1)


@pytest.mark.parametrize("K,lr", PGD_SCHEDULES)
@pytest.mark.parametrize("name", FAMILY)
def test_family_problems_pass_the_feed_screen_on_the_host(name, K, lr):
    """The screen of the GPU cases with the host mirror of the context at B = 37: a seed is found, and the case is a case -- at
    lr = 0.1 the restatement ends with entries on lo and on hi, at lr = 0.001 y moves by more than 0.01."""
    spec = FC_SPECS[name]
    for seed in range(20):
        params, x = _problem(spec, 37, seed, TAME.get(name))
        ctx = picnn.context(spec, params, torch.from_numpy(x)).numpy()
        fg = picnn_oracle.make_fg_chain(params, ctx, list(spec.szs), spec.alpha)
        ref, same = pgd_ref.screen_feeds(fg, _start("random", 37, spec.n_labels, seed)[1], K, lr)
        if same:
            break
    else:
        raise AssertionError("no screened seed")
    assert np.isfinite(ref["y"]).all() and np.isfinite(ref["obj"]).all() and np.isfinite(ref["obj_final"]).all()
    if lr == 0.1:
        assert (ref["y"] == LO).any() and (ref["y"] == pgd_ref.HI).any()
    else:
        assert np.abs(ref["y"] - ref["iterates"][0]).max() > 0.01


# ------------------------------------------------------------------------------------------------ problems


@functools.lru_cache(maxsize=None)
def _fc(name, B, seed):
    """(spec, model, ctx, fg): the model on the device, its context, and the MFMA-order oracle on that very context"""
    spec = FC_SPECS[name]
    params, x = _problem(spec, B, seed, TAME.get(name))
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    fg = picnn_oracle.make_fg_chain(params, ctx.cpu().numpy(), list(spec.szs), spec.alpha)
    return spec, model, ctx, fg


@functools.lru_cache(maxsize=None)
def _fc_screened(name, B, K, lr):
    """the first seed that pgd_ref.screen_feeds accepts: (seed, y0, the restatement's run)"""
    for seed in range(20):
        spec, model, ctx, fg = _fc(name, B, seed)
        y0 = _start("random", B, spec.n_labels, seed)[1]
        ref, same = pgd_ref.screen_feeds(fg, y0, K, lr)
        if same:
            return seed, y0, ref
    raise AssertionError("no screened seed")


def _conv_start(spec, B, seed, out_of_box):
    rng = np.random.RandomState(seed)
    y0 = np.repeat((0.2 + 0.6 * rng.rand(spec.n_labels))[None], B, axis=0)      # meanY-like start (test_gd_conv.py)
    if out_of_box:
        y0[:, ::97] = (-0.5, 0.0, 1.0, 2.0)[seed % 4]                           # as test_pgd_conv.py
    return y0


@functools.lru_cache(maxsize=None)
def _conv(H, W, B, seed):
    spec = picnn.ConvSpec(H, W)
    params = picnn.init_conv_params(spec, seed, "spread")
    x = np.random.RandomState(seed + 50).rand(B, H, W, 1).astype(np.float32)
    model = picnn.ConvModel(spec, params)
    ctx = model.context(torch.from_numpy(x).cuda())
    fg = picnn_conv_oracle.make_fg_chain(params, ctx.cpu().numpy(), H, W)
    return spec, model, ctx, fg


@functools.lru_cache(maxsize=None)
def _conv_screened(H, W, B, K, lr):
    for seed in range(20):
        spec, model, ctx, fg = _conv(H, W, B, seed)
        y0 = _conv_start(spec, B, seed, True)
        ref, same = pgd_ref.screen_feeds(fg, y0, K, lr)
        if same:
            return seed, y0, ref
    raise AssertionError("no screened seed")


def _check_pgd(what, ref, out, K, lr):
    """test_pgd._check_against, behind one line that names the case and gives the fraction of every bound it used"""
    y, obj, fin = out
    dy = np.abs(y.cpu().numpy() - ref["y"]).max() / pgd_ref.y_tolerance(K, lr)
    de = (np.abs(obj.cpu().numpy() - ref["obj"]) / (8 * ULP * ref["scale"])).max()
    df = (np.abs(fin.cpu().numpy() - ref["obj_final"]) / (8 * ULP * ref["scale_final"])).max()
    edge = (ref["y"] == LO) | (ref["y"] == pgd_ref.HI)
    print("FRACTIONS %s K=%d lr=%g: |dy| %.4f, e_k %.4f, e_K %.4f of their bounds; %.1f %% of y_K on lo, %.1f %% on hi; "
          "y moved by %.2e" % (what, K, lr, dy, de, df, 100 * (ref["y"] == LO).mean(), 100 * (ref["y"] == pgd_ref.HI).mean(),
                              np.abs(ref["y"] - ref["iterates"][0]).max()))
    assert y.dtype == obj.dtype == fin.dtype == torch.float64
    assert y.shape == ref["y"].shape and obj.shape == ref["obj"].shape and fin.shape == ref["obj_final"].shape
    _check_against(ref, y, obj, fin, K, lr)
    assert np.abs(ref["y"] - ref["iterates"][0]).max() > 1e-5                   # y did move
    return edge


def _check_gd(what, ref, out, y0):
    y_ref, traj_ref, E_ref = ref
    y, traj, E = (t.cpu().numpy() for t in out)
    assert y.dtype == traj.dtype == np.float64 and E.dtype == np.float32 and traj.shape == traj_ref.shape
    assert np.array_equal(traj, traj_ref), "%s trajectory: %s" % (what, _first_difference(traj, traj_ref))
    assert np.array_equal(y, y_ref.astype(np.float64)), "%s y_K: %s" % (what, _first_difference(y, y_ref.astype(np.float64)))
    assert np.array_equal(E, E_ref), "%s E(y_K): %s" % (what, _first_difference(E, E_ref))
    moved = float(np.abs(y_ref - np.asarray(y0).astype(np.float32)).max())
    assert moved > 1e-4                                                          # y did move
    return moved


# ------------------------------------------------------------------------------------------------ 2. FC, the edges


@pytest.mark.gpu
@pytest.mark.parametrize("B", EDGE_BATCHES)
@pytest.mark.parametrize("name", EDGE_SPECS)
def test_gd_at_the_dispatch_edges(name, B):
    """Trajectory, y_K and E(y_K) bit for bit at the ragged rows workgroup (257, 511), the last rows batch (512), the first
    tile batch with its one-row tile (513) and whole tiles (528).  The first seed whose y moves by more than 1e-4 is taken:
    seed 0 for every spec, n = 1 included."""
    from icnn_amd import gd
    _need_256_cus()
    for seed in range(20):
        spec, model, ctx, fg = _fc(name, B, seed)
        y0 = np.random.RandomState(seed + 32).rand(B, spec.n_labels)
        ref = gd_ref.unroll_f32(fg, y0, GD_K, GD_LR, GD_MU)
        if float(np.abs(ref[0] - y0.astype(np.float32)).max()) > 1e-4:
            break
    else:
        raise AssertionError("no seed on which y moves")
    out = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), GD_K, GD_LR, GD_MU, trajectory=True, energy=True)
    torch.cuda.synchronize()
    moved = _check_gd("%s B=%d" % (name, B), ref, out, y0)
    print("%s B=%d seed %d %s: GD bit-exact, y moved by up to %.2e" % (name, B, seed, form(B), moved))


@pytest.mark.gpu
@pytest.mark.parametrize("K,lr", PGD_SCHEDULES)
@pytest.mark.parametrize("B", EDGE_BATCHES)
@pytest.mark.parametrize("name", EDGE_SPECS)
def test_pgd_at_the_dispatch_edges(name, B, K, lr):
    from icnn_amd import pgd
    _need_256_cus()
    seed, y0, ref = _fc_screened(name, B, K, lr)
    spec, model, ctx, fg = _fc(name, B, seed)
    out = pgd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, final=True)
    torch.cuda.synchronize()
    _check_pgd("%s B=%d seed %d %s" % (name, B, seed, form(B)[0]), ref, out, K, lr)


def _per_sample(rule, out, idx):
    """the rows of `idx` in every output of a solve: obj of PGD is [K, B], everything else has the sample first"""
    y, a, b = out
    return y[idx], (a[:, idx] if rule == "pgd" else a[idx]), b[idx]


def _solve(rule, model, ctx, y0):
    from icnn_amd import gd, pgd
    if rule == "gd":
        return gd.solve(model, ctx, y0, GD_K, GD_LR, GD_MU, trajectory=True, energy=True)
    return pgd.solve(model, ctx, y0, 3, 0.1, final=True)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["gd", "pgd"])
@pytest.mark.parametrize("name", ["n270", "deep8"])
def test_a_sample_has_the_same_bits_in_every_form(name, rule):
    """Samples 0, 255, 256 and 512 of a 513-batch (tiles; 512 is the lone row of the last tile) alone, inside the first 257
    (rows: 256 is the lone sample of the ragged workgroup, 255 the second of a pair) and inside the first 512 (rows, whole):
    y and traj / E (GD) or e_k / e_K (PGD) bit for bit.  The context rows are slices of the 513-batch's context."""
    _need_256_cus()
    spec, model, ctx, fg = _fc(name, CROSS_BATCH, 3)
    n = spec.n_labels
    y0 = np.random.RandomState(35).rand(CROSS_BATCH, n) if rule == "gd" else _start("random", CROSS_BATCH, n, 3)[1]
    y0 = torch.from_numpy(y0).cuda()
    whole = _solve(rule, model, ctx, y0)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in whole)
    assert float((whole[0] - (y0 if rule == "gd" else y0.clamp(LO, pgd_ref.HI))).abs().max()) > 1e-4
    for i in CROSS_SAMPLES:
        for lo, hi in [(i, i + 1)] + [(0, p) for p in CROSS_PREFIXES if i < p]:
            part = _solve(rule, model, ctx[lo:hi].contiguous(), y0[lo:hi])
            torch.cuda.synchronize()
            for what, a, b in zip(("y", "traj / e_k", "E / e_K"), _per_sample(rule, part, i - lo), _per_sample(rule, whole, i)):
                assert torch.equal(a, b), "%s %s: sample %d in [%d, %d) differs from the batch of 513 in %s" % (name, rule, i, lo, hi, what)


# ------------------------------------------------------------------------------------------------ 3. FC, PGD on the family


@pytest.mark.gpu
@pytest.mark.parametrize("K,lr", PGD_SCHEDULES)
@pytest.mark.parametrize("B", FAMILY_BATCHES)
@pytest.mark.parametrize("name", FAMILY)
def test_pgd_on_the_architecture_family(name, B, K, lr):
    """n = 1 is one live lane, n = 270 five lane passes with a ragged tail behind npad = 272, eight layers the largest rows
    layout.  At lr = 0.1 a share of y_K sits on lo and on hi, where the device must agree bit for bit."""
    from icnn_amd import pgd
    _need_256_cus()
    seed, y0, ref = _fc_screened(name, B, K, lr)
    spec, model, ctx, fg = _fc(name, B, seed)
    out = pgd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, final=True)
    torch.cuda.synchronize()
    edge = _check_pgd("%s B=%d seed %d %s" % (name, B, seed, form(B)[0]), ref, out, K, lr)
    if lr == 0.1:
        assert edge.any()                                                      # the exact-edge assertion has entries to bite on


# ------------------------------------------------------------------------------------------------ 4. conv


@pytest.mark.gpu
@pytest.mark.parametrize("B", CONV_BATCHES)
@pytest.mark.parametrize("H,W", CONV_SIZES)
def test_conv_gd_at_other_sizes(H, W, B):
    from icnn_amd import gd
    K, lr, mu = CONV_GD
    spec, model, ctx, fg = _conv(H, W, B, 8)
    y0 = _conv_start(spec, B, 8, False)
    out = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True, energy=True)
    torch.cuda.synchronize()
    moved = _check_gd("conv %dx%d B=%d" % (H, W, B), gd_ref.unroll_f32(fg, y0, K, lr, mu), out, y0)
    print("conv %dx%d B=%d: GD bit-exact, y moved by up to %.2e" % (H, W, B, moved))


@pytest.mark.gpu
@pytest.mark.parametrize("K,lr", PGD_SCHEDULES)
@pytest.mark.parametrize("B", CONV_BATCHES)
@pytest.mark.parametrize("H,W", CONV_SIZES)
def test_conv_pgd_at_other_sizes(H, W, B, K, lr):
    """pgd_conv_update_kernel makes 4 (32 x 32, 16 x 64) and 12 (48 x 64) strided passes where the shipped image makes 8, and
    block_tree_sum meets n = 1024 and 3072"""
    from icnn_amd import pgd
    seed, y0, ref = _conv_screened(H, W, B, K, lr)
    spec, model, ctx, fg = _conv(H, W, B, seed)
    out = pgd.solve(model, ctx, torch.from_numpy(y0).cuda().reshape(B, H, W, 1), K, lr, final=True)
    torch.cuda.synchronize()
    edge = _check_pgd("conv %dx%d B=%d seed %d" % (H, W, B, seed), ref, out, K, lr)
    assert edge.any() or lr != 0.1


def _conv_small():
    spec, model, ctx, fg = _conv(32, 32, 17, 1)
    return spec, model, ctx, torch.from_numpy(_conv_start(spec, 17, 1, True)).cuda()


def _solve_conv(rule, model, ctx, y0, **kw):
    from icnn_amd import gd, pgd
    if rule == "gd":
        K, lr, mu = CONV_GD
        return gd.solve(model, ctx, y0, K, lr, mu, **(kw or dict(trajectory=True, energy=True)))
    return pgd.solve(model, ctx, y0, 3, 0.1, **(kw or dict(final=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["gd", "pgd"])
def test_conv_optional_outputs_do_not_change_y(rule):
    """conv_gd_rounds decides by null pointers what it records: all four combinations leave y and every present output alone"""
    spec, model, ctx, y0 = _conv_small()
    full = _solve_conv(rule, model, ctx, y0)
    first, second = ("trajectory", "energy") if rule == "gd" else ("trace", "final")
    for a in (True, False):
        for b in (True, False):
            y, oa, ob = _solve_conv(rule, model, ctx, y0, **{first: a, second: b})
            torch.cuda.synchronize()
            assert (oa is not None) == a and (ob is not None) == b
            assert torch.equal(y, full[0]), (rule, a, b)
            assert oa is None or torch.equal(oa, full[1]), (rule, a, b)
            assert ob is None or torch.equal(ob, full[2]), (rule, a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["gd", "pgd"])
def test_conv_sample_alone_and_scratch_regrowth(rule):
    """A sample alone equals the same sample inside B = 17; and one ConvModel solved at B = 3, at B = 17 (ConvModel.reserve
    regrows the scratch) and at B = 3 again gives the first result's bits."""
    spec, _, ctx, y0 = _conv_small()
    params = picnn.init_conv_params(spec, 1, "spread")
    model = picnn.ConvModel(spec, params)                                       # a fresh model: no scratch yet
    c3, s3 = ctx[:3].contiguous(), y0[:3]
    first = [t.clone() for t in _solve_conv(rule, model, c3, s3)]
    assert model.c_model.work_batch == 3
    whole = [t.clone() for t in _solve_conv(rule, model, ctx, y0)]
    assert model.c_model.work_batch == 17
    again = _solve_conv(rule, model, c3, s3)
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    for a, b in zip(first, _per_sample(rule, whole, torch.arange(3, device=ctx.device))):
        assert torch.equal(a, b)
    for i in (5, 16):
        alone = _solve_conv(rule, model, ctx[i:i + 1].contiguous(), y0[i:i + 1])
        torch.cuda.synchronize()
        for a, b in zip(_per_sample(rule, alone, 0), _per_sample(rule, whole, i)):
            assert torch.equal(a, b), (rule, i)


@pytest.mark.gpu
def test_conv_pgd_captured_replay_equals_eager():
    from icnn_amd import pgd
    spec, model, ctx, y0 = _conv_small()
    ctx, y0 = ctx[:3].contiguous(), y0[:3].contiguous()
    eager = [t.clone() for t in pgd.solve(model, ctx, y0, 3, 0.1, final=True)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = pgd.solve(model, ctx, y0, 3, 0.1, final=True)
    for t in out:
        t.fill_(0.123)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(eager, out):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("rule", ["gd", "pgd"])
def test_conv_start_forms_hold_the_same_bits(rule):
    """a scalar, an [n] row, [B, n] and images [B, H, W, 1] of the same values"""
    spec, model, ctx, y0 = _conv_small()
    B, n = y0.shape
    row = y0[0].clone()                                                         # with entries outside the box
    runs = [_solve_conv(rule, model, ctx, s) for s in (row, row.cpu().numpy(), row.expand(B, n), row.expand(B, n).cpu().numpy(),
                                                        row.expand(B, n).reshape(B, spec.H, spec.W, 1))]
    flat = [_solve_conv(rule, model, ctx, s) for s in (0.3, np.full(n, 0.3), torch.full((B, n), 0.3, dtype=torch.float64))]
    torch.cuda.synchronize()
    for group in (runs, flat):
        for other in group[1:]:
            for a, b in zip(group[0], other):
                assert torch.equal(a, b)
    assert not torch.equal(runs[0][0], flat[0][0])


# ------------------------------------------------------------------------------------------------ 5. containment


@functools.lru_cache(maxsize=None)
def _containment_problem(form_name, rule):
    """(model, ctx, y0, poisoned sample, named neighbours, the clean solve)"""
    if form_name == "conv":
        spec, model, ctx, y0 = _conv_small()
        (B, p), mates = CONV_POISONED, []
        assert B == ctx.shape[0]
    else:
        B, p, mates = POISONED[form_name]
        spec, model, ctx, fg = _fc("small", B, 4)
        y0 = torch.from_numpy(_start("random", B, spec.n_labels, 4)[1]).cuda()
    clean = [t.clone() for t in _run(form_name, rule, model, ctx, y0)]
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t).all()) for t in clean)
    return model, ctx, y0, p, mates, clean


def _run(form_name, rule, model, ctx, y0):
    return _solve_conv(rule, model, ctx, y0) if form_name == "conv" else _solve(rule, model, ctx, y0)


@pytest.mark.gpu
@pytest.mark.parametrize("poison", ["y0_nan", "ctx_nan", "ctx_inf"])
@pytest.mark.parametrize("rule", ["gd", "pgd"])
@pytest.mark.parametrize("form_name", ["rows", "tiles", "conv"])
def test_a_poisoned_sample_leaves_its_neighbours_alone(form_name, rule, poison):
    """One NaN start entry, one NaN context entry or one +Inf context entry in one sample: every other sample keeps its bits in
    every output -- by name the sample that shares the rows workgroup and the fifteen that share the MFMA tile.  Under PGD the
    start is clip(y0) = fmin(fmax(y0, lo), hi), which takes a NaN entry to lo: that run equals the run started at lo."""
    if form_name != "conv":
        _need_256_cus()
    model, ctx, y0, p, mates, clean = _containment_problem(form_name, rule)
    B = ctx.shape[0]
    ctx2, y02 = ctx.clone(), y0.clone()
    j = y0.shape[1] // 3
    if poison == "y0_nan":
        y02[p, j] = float("nan")
    else:
        ctx2[p, ctx.shape[1] // 3] = float("nan") if poison == "ctx_nan" else float("inf")
    out = _run(form_name, rule, model, ctx2, y02)
    torch.cuda.synchronize()
    hit = not all(bool(torch.isfinite(t).all()) for t in _per_sample(rule, out, p))
    print("%s %s %s: the poisoned sample's outputs are %s" % (form_name, rule, poison, "not finite" if hit else "finite"))
    for m in mates:
        for what, a, b in zip(("y", "traj / e_k", "E / e_K"), _per_sample(rule, out, m), _per_sample(rule, clean, m)):
            assert torch.equal(a, b), "sample %d beside the poisoned %d differs in %s" % (m, p, what)
    others = torch.tensor([u for u in range(B) if u != p], device=ctx.device)
    for what, a, b in zip(("y", "traj / e_k", "E / e_K"), _per_sample(rule, out, others), _per_sample(rule, clean, others)):
        assert torch.equal(a, b), "%s: a sample other than the poisoned %d differs" % (what, p)
    if rule == "pgd" and poison == "y0_nan":
        y03 = y0.clone()
        y03[p, j] = LO
        at_lo = _run(form_name, rule, model, ctx, y03)
        torch.cuda.synchronize()
        for a, b in zip(out, at_lo):
            assert torch.equal(a, b)
        assert bool(torch.isfinite(out[0]).all())
