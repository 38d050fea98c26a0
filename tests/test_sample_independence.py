"""A sample's solve does not depend on its batch, and a non-finite value stays in the sample it entered.

plan_fc_solve promises "Results are bit-identical whichever row runs"; the other identity tests hold the batch fixed and change
the flags.  Here the default dispatch (flags = 0) solves the same samples in other batches: as the contiguous shards of 2, 4
and 8 ranks (what dist.solve_sharded does with a context of the full batch), in another order, and alone.  The batch sizes
are the smallest at which the full batch and its shards run different kernels on 256 CUs (tests/test_solve_plan.py pins
them): MFMA tiles of 16 or 8 rows with a partial last tile against the per-sample kernel with 1 to 3 samples per workgroup,
lockstep rounds with four samples per wave against the same.  The context is computed once from the full batch and sliced, so
BatchNorm statistics are the same and any difference is the solve's.  Every comparison is np.array_equal on the eleven
output tensors.

Second half: ICNN_BE_ST_NONFINITE as the device itself sets it.  Context rows (fused solves) or the callback's values
(generic mode) are made NaN or +inf for a few samples: exactly those samples stop with the bit set, no other sample carries an
error bit or differs in any output from the clean solve, and raise_on_error names the first of them."""
import functools

import numpy as np
import pytest
import torch

import problems
from icnn_amd import _lib, dist, picnn

pytestmark = pytest.mark.gpu

OUTPUTS = ("y", "lam", "active", "count", "n_iters", "newton_iters", "G", "h", "ys", "finished", "status")
STATUS = OUTPUTS.index("status")
FINISHED = OUTPUTS.index("finished")

# name -> (spec, batch, nIter, variant); the full batch's kernel and the shards' in tests/test_solve_plan.py
CASES = {
    "bibtex_1043x10_dual": ("bibtex", 1043, 10, "dual"),         # TILE, 8 rows, last tile of 3 | ROWS 3, 2, 1
    "bibtex_1043x20_dual": ("bibtex", 1043, 20, "dual"),         # the 32-slot tile instance | ROWS
    "bibtex_2051x10_dual": ("bibtex", 2051, 10, "dual"),         # TILE, 16 rows | TILE 8, ROWS 3, 2, 1
    "bibtex_1043x10_pdipm": ("bibtex", 1043, 10, "pdipm"),       # TILE 8 | ROWS
    "halfcheetah_1043x5_rl": ("halfcheetah", 1043, 5, "rl"),     # lockstep rounds, four samples per wave | ROWS
}
WORLDS = (2, 4, 8)
PERMUTED = ("bibtex_1043x10_dual", "bibtex_1043x20_dual", "halfcheetah_1043x5_rl")


def _planned(model, res):
    """The plan icnn_be_solve_fc followed for this solve (tests/test_gpu_parity.py's idiom): asserts that the solve issued the
    rounds the plan says and returns (path, samples per workgroup, budget, rounds)."""
    plan = _lib.solve_plan(model.c_model, res.state.c_state)
    assert res.state.rounds == plan[3], (plan, res.state.rounds)
    return plan


def _all_outputs(res, B):
    return [t.cpu().numpy().copy() for t in (res.y, res.lam, res.active, res.count[:B], res.n_iters[:B], res.newton_iters[:B],
                                             res.state.G, res.state.h, res.state.ys, res.finished[:B], res.status[:B])]


def _frozen(outs):
    for a in outs:
        a.setflags(write=False)
    return outs


def _solve(model, ctx, n_iter, variant, fc=True):
    """one solve of the rows of ctx by the default dispatch, on a solver of its own: (outputs, plan)"""
    from icnn_amd import bundle_entropy
    B = ctx.shape[0]
    res = bundle_entropy.FusedSolver(model, B, n_iter, variant, flags=0).solve(ctx.contiguous(), 0.5)
    plan = _planned(model, res) if fc else None
    return _all_outputs(res, B), plan, res


def _assert_same(got, want, what, rows=None):
    for name, a, b in zip(OUTPUTS, got, want):
        if rows is not None:
            a, b = a[rows], b[rows]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, name)
        if not np.array_equal(a, b):
            diff = np.nonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0]
            raise AssertionError("%s: output %s differs on %d samples, first %s" % (what, name, len(diff), diff[:8]))


@functools.lru_cache(maxsize=None)
def _case(name):
    """(spec, model, params, context of the full batch, outputs of its one-launch solve, its plan), made once per case"""
    which, B, n_iter, variant = CASES[name]
    if which == "bibtex":
        spec = picnn.bibtex_spec()
        params = picnn.init_params(spec, 0, "spread")
        x = (np.random.RandomState(90).rand(B, spec.n_features) < 0.04).astype(np.float32)
    else:
        spec = picnn.halfcheetah_spec()
        params = picnn.init_params(spec, 0, "spread", yu_bias=1.0, gate_bias=1.0)
        x = np.random.RandomState(91).randn(B, spec.n_features).astype(np.float32)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x)).clone()
    outs, plan, _ = _solve(model, ctx, n_iter, variant)
    assert (outs[STATUS] == 0).all()
    return spec, model, params, ctx, _frozen(outs), plan


def _shards(model, ctx, n_iter, variant, world, fc=True):
    B = ctx.shape[0]
    pieces, plans = [], []
    for rank in range(world):
        lo, hi = dist.shard_bounds(B, world, rank)
        outs, plan, _ = _solve(model, ctx[lo:hi], n_iter, variant, fc)
        pieces.append(outs)
        plans.append(plan)
    return [np.concatenate(parts, axis=0) for parts in zip(*pieces)], plans


def _unpermuted(outs, perm):
    """outputs of a solve of rows perm[0], perm[1], ... mapped back to the batch's own order"""
    back = []
    for a in outs:
        b = np.empty_like(a)
        b[perm] = a
        back.append(b)
    return back


# ------------------------------------------------------------------------------------------------ 1. independence


@pytest.mark.parametrize("world", WORLDS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_stitched_shards_equal_the_one_launch_solve(name, world):
    _, B, n_iter, variant = CASES[name]
    _, model, _, ctx, full, plan = _case(name)
    stitched, plans = _shards(model, ctx, n_iter, variant, world)
    print("%s: full batch %s; world %d: %s" % (name, plan, world, sorted(set(plans))))
    assert any(p[:2] != plan[:2] for p in plans), (plan, plans)      # not a kernel against itself
    _assert_same(stitched, full, "%s in %d shards" % (name, world))
    assert full[OUTPUTS.index("count")].max() >= 2                  # bundles of several cuts: the subproblem solver ran


@pytest.mark.parametrize("order", ["shuffled", "reversed"])
@pytest.mark.parametrize("name", PERMUTED)
def test_a_permuted_batch_gives_every_sample_the_same_result(name, order):
    """reversed: the members of the partial last tile (or quad) sit in full tiles and the first rows form the partial one"""
    _, B, n_iter, variant = CASES[name]
    _, model, _, ctx, full, _ = _case(name)
    perm = np.random.RandomState(92).permutation(B) if order == "shuffled" else np.arange(B)[::-1].copy()
    outs, _, _ = _solve(model, ctx[torch.from_numpy(perm).to(ctx.device)], n_iter, variant)
    _assert_same(_unpermuted(outs, perm), full, "%s %s" % (name, order))


def test_one_sample_alone_equals_its_rows_of_the_full_batch():
    name = "bibtex_1043x10_dual"
    _, B, n_iter, variant = CASES[name]
    _, model, _, ctx, full, plan = _case(name)
    newton, count = full[OUTPUTS.index("newton_iters")], full[OUTPUTS.index("count")]
    # the first, the last (partial tile), the hardest two, and two inside a tile (rows 3 of tile 13 and 1 of the last one)
    picked = [0, B - 1, int(np.argmax(newton)), int(np.argmax(count)), 8 * 13 + 3, B - 2]
    for u in picked:
        outs, alone, _ = _solve(model, ctx[u:u + 1], n_iter, variant)
        assert alone[:2] != plan[:2], (alone, plan)
        _assert_same(outs, [a[u:u + 1] for a in full], "sample %d alone" % u)


@functools.lru_cache(maxsize=None)
def _conv_case():
    """The smallest accepted image size, 22 samples, the nIter of test_conv_fused_solve_at_other_sizes."""
    from test_architectures import _conv_problem
    spec = picnn.ConvSpec(32, 32)
    B, n_iter, variant = 22, 5, "dual"
    p = _conv_problem(spec, "spread", 31, False, B=B)
    model = picnn.ConvModel(spec, p["params"])
    ctx = model.context(torch.from_numpy(p["x"])).clone()
    outs, _, _ = _solve(model, ctx, n_iter, variant, fc=False)
    assert (outs[STATUS] == 0).all()
    return spec, model, p["params"], ctx, _frozen(outs), n_iter, variant


@pytest.mark.parametrize("how", ["world2", "world8", "shuffled"])
def test_conv_shards_and_a_permuted_batch_equal_the_one_launch_solve(how):
    spec, model, _, ctx, full, n_iter, variant = _conv_case()
    B = ctx.shape[0]
    if how == "shuffled":
        perm = np.random.RandomState(93).permutation(B)
        outs, _, _ = _solve(model, ctx[torch.from_numpy(perm).to(ctx.device)], n_iter, variant, fc=False)
        got = _unpermuted(outs, perm)
    else:
        got, _ = _shards(model, ctx, n_iter, variant, int(how[5:]), fc=False)
    _assert_same(got, full, "conv 32 x 32, %s" % how)


# ------------------------------------------------------------------------------------------------ 3. non-finite values

ERROR_BITS = _lib.ST_ERROR_MASK


def _poisoned_samples(name, B):
    """row 0 of a tile (of 16, 8 or 4 rows), a sample in the middle of one (row 5 of 16 and of 8, row 1 of a quad), the very
    last sample (partial tile or quad); HalfCheetah: also row 2 of a quad whose other three stay clean"""
    picked = [32, 53, B - 1]
    if name.startswith("halfcheetah"):
        picked.append(70)
    return sorted(picked)


def _assert_contained(clean, got, res, bad, what):
    B = clean[STATUS].shape[0]
    bad = np.asarray(bad)
    others = np.setdiff1d(np.arange(B), bad)
    status, finished = got[STATUS], got[FINISHED]
    print("%s: status of the poisoned samples %s, finished %s" % (what, status[bad], finished[bad]))
    assert ((status[bad] & _lib.ST_NONFINITE) != 0).all(), (what, status[bad])
    assert (finished[bad] == 1).all(), (what, finished[bad])
    assert ((status[others] & ERROR_BITS) == 0).all(), (what, others[(status[others] & ERROR_BITS) != 0][:8])
    _assert_same(got, clean, what, rows=others)
    with pytest.raises(FloatingPointError, match=r"sample %d$" % bad.min()):
        res.raise_on_error()


def _energy_is_nonfinite(spec, params, row):
    """CPU: the poisoned context row reaches the energy (a poison that the network masks would make the test vacuous)"""
    from oracle import picnn_oracle
    fg = picnn_oracle.make_fg_from_context(params, row[None], list(spec.szs), float(spec.alpha),
                                           "action" if spec.action_box else None)
    with np.errstate(all="ignore"):
        E, _ = fg(np.full((1, spec.n_labels), 0.5))
    return not np.isfinite(E).all()


@pytest.mark.parametrize("poison", [np.nan, np.inf], ids=["nan", "inf"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_poisoned_context_rows_stop_their_own_samples_only(name, poison):
    """the full batch and rank 0's shard of eight: both kernels of the case"""
    _, B, n_iter, variant = CASES[name]
    spec, model, params, ctx, full, plan = _case(name)
    lo, hi = dist.shard_bounds(B, 8, 0)
    row = np.full(spec.ctx_width, poison, dtype=np.float32)              # the whole row: no single entry is in every path to E
    assert _energy_is_nonfinite(spec, params, row)
    plans = []
    for what, rows, clean in (("full batch", slice(0, B), full), ("shard 0 of 8", slice(lo, hi), None)):
        part = ctx[rows].clone()
        if clean is None:
            clean, _, _ = _solve(model, part, n_iter, variant)
        bad = _poisoned_samples(name, part.shape[0])
        part[torch.tensor(bad, device=part.device)] = poison
        got, p, res = _solve(model, part, n_iter, variant)
        plans.append(p)
        _assert_contained(clean, got, res, bad, "%s, %s, %s" % (name, what, poison))
    assert plans[0][:2] != plans[1][:2] and plans[0] == plan, plans


def _generic(prob, n_iter, variant, fg, **kw):
    from icnn_amd import bundle_entropy
    res = bundle_entropy.solveBatch(fg, prob.y0(), nIter=n_iter, variant=variant, native=True, **kw)
    return _all_outputs(res, prob.B), res


GENERIC = {
    "lse_n33_dual": (lambda: problems.log_sum_exp(26, 37, 33, 8, 1.0), 10, "dual"),
    "lse_n13_rl": (lambda: problems.log_sum_exp(27, 37, 13, 6, 1.0), 5, "rl"),      # narrow rows: dual_step_small_kernel
}


@pytest.mark.parametrize("what", ["nan_energy", "inf_gradient"])
@pytest.mark.parametrize("case", sorted(GENERIC))
def test_generic_mode_nonfinite_callback_values_stop_their_own_sample_only(case, what):
    factory, n_iter, variant = GENERIC[case]
    prob = factory()
    clean, _ = _generic(prob, n_iter, variant, prob.fg, check=False)
    assert (clean[STATUS] == 0).all()
    calls = [0]

    def fg(y):
        f, g = prob.fg(y)
        f, g = f.copy(), g.copy()
        calls[0] += 1
        if what == "nan_energy":
            if calls[0] >= 2:                           # from the second evaluation on: the sample holds a clean cut already
                f[5] = np.nan
        else:
            g[36, prob.n // 2] = np.inf
        return f, g

    bad = [5] if what == "nan_energy" else [36]
    got, res = _generic(prob, n_iter, variant, fg, check=False)
    assert calls[0] >= 2
    _assert_contained(clean, got, res, bad, "%s, %s" % (case, what))
    calls[0] = 0
    with pytest.raises(FloatingPointError):
        _generic(prob, n_iter, variant, fg, check=True)


def test_conv_poisoned_context_row_stops_its_own_sample_only():
    from oracle import picnn_conv_oracle as co
    spec, model, params, ctx, full, n_iter, variant = _conv_case()
    bad = [9]
    row = np.full((1, spec.ctx_width), np.nan, dtype=np.float32)
    with np.errstate(all="ignore"):
        E, _ = co.make_fg_from_context(params, row, spec.H, spec.W)(np.full((1, spec.n_labels), 0.5))
    assert not np.isfinite(E).all()
    part = ctx.clone()
    part[bad[0]] = float("nan")
    got, _, res = _solve(model, part, n_iter, variant, fc=False)
    _assert_contained(full, got, res, bad, "conv 32 x 32, NaN context row")
