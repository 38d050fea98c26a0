"""icnn_be_adam_fc_each (be_adam.hip, the EACH instantiations of adam_fc_kernel and adam_rows_kernel): the inner Adam optimiser
with the stopping rule applied to every state on its own.  The contract is bits only: row u of act_best, f_best and iters is
what icnn_be_adam_fc returns for the batch that consists of row u alone, so every GPU case compares

  * with the device's own icnn_be_adam_fc at batch 1, row by row, torch.equal;
  * with oracle.adam_oracle.adam run on row u alone (tests/test_adam_architectures.py's _oracle_adam), np.array_equal; the
    batches beyond 64 states with `adam_each_ref`, the same loop for all rows at once, which the CPU tests pin to the row-by-row
    oracle first.

Problems as tests/test_adam_architectures.py builds them ("spread" weights; `scale` multiplies the observations of the last
states).  Every case is screened on the CPU (chain-order context rows) so that each state's smoothed displacement keeps 1e-9
from the threshold wherever its rule reads it, and -- where `spread` is set -- so that one workgroup holds states whose stop
iterations differ by a factor of two or more: a frozen state sits beside a running one for at least half of the loop.

  case            hidden    obs  n   B     launch on 256 CUs        oracle iters (chain-order rows)
  rows_n6_b1      (24, 16)  7    6   1     rows, 1 x 1              15
  rows_n6_b2      (24, 16)  7    6   2     rows, 1 x 2              15, 6
  rows_n6_b4      (24, 16)  7    6   4     rows, 1 x 4              15, 6, 6, 20
  rows_n6_b4_m10  the same at max_iter 10: states 0 and 3 never fire
  rows_n6_b5      (24, 16)  7    6   5     rows, 5 x 1              15, 6, 6, 20, 6
  rows_n6_b37     (24, 16)  7    6   37    rows, 37 x 1             6 .. 55
  rows_n6_b601    (24, 16)  7    6   601   rows, 201 x 3 (last: 1)  6 .. 60
  rows_n6_b1023   (24, 16)  7    6   1023  rows, 256 x 4 (last: 3)
  rows_n1_b4      (16,)     5    1   4     rows, 1 x 4              16, 8, 12, 14
  rows_n64_b2     (40, 24)  9    64  2     rows, 1 x 2              52, 141
  rows_n64_b4     (40, 24)  9    64  4     rows, 1 x 4
  tile_n70_b1     (32, 24)  9    70  1     tile, 1                  50
  tile_n70_b16    (32, 24)  9    70  16    tile, 1                  14 .. 186
  tile_n70_b16_m60  the same at max_iter 60: some fire, some never
  tile_n70_b17    (32, 24)  9    70  17    tile, 2 (16 + 1)         14 .. 186
  tile_n6_b1025   (24, 16)  7    6   1025  tile, 65 (last: 1)       n = 6 beyond the rows plan
"""
import ctypes as C
import dataclasses
import os
import types

import numpy as np
import pytest
import torch

import test_adam_architectures as arch
from icnn_amd import _lib, picnn
from oracle import adam_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, TILE = "ROWS", "TILE"
MAX_ITER = 400
ROWS_MAX, TM = 4, 16


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    widths: tuple
    n_obs: int
    n: int
    B: int
    seed: int
    plan: tuple                # (kernel, states per workgroup, workgroups) on a device of 256 CUs
    scale: tuple = None
    max_iter: int = MAX_ITER
    spread: bool = False       # some workgroup holds states whose oracle iters differ by a factor >= 2
    never: bool = False        # some state never fires within max_iter (and some state does)


N6, N1, N64, N70 = ((24, 16), 7, 6), ((16,), 5, 1), ((40, 24), 9, 64), ((32, 24), 9, 70)
CASES = [
    Case("rows_n6_b1", *N6, 1, 1, (ROWS, 1, 1)),
    Case("rows_n6_b2", *N6, 2, 1, (ROWS, 2, 1), spread=True),
    Case("rows_n6_b4", *N6, 4, 1, (ROWS, 4, 1), spread=True),
    Case("rows_n6_b4_m10", *N6, 4, 1, (ROWS, 4, 1), max_iter=10, never=True),
    Case("rows_n6_b5", *N6, 5, 1, (ROWS, 1, 5)),
    Case("rows_n6_b37", *N6, 37, 1, (ROWS, 1, 37), (12, 16.0)),
    Case("rows_n6_b601", *N6, 601, 1, (ROWS, 3, 201), (12, 16.0), spread=True),
    Case("rows_n6_b1023", *N6, 1023, 1, (ROWS, 4, 256), (12, 16.0), spread=True),
    Case("rows_n1_b4", *N1, 4, 3, (ROWS, 4, 1), spread=True),
    Case("rows_n64_b2", *N64, 2, 1, (ROWS, 2, 1), (1, 64.0), spread=True),
    Case("rows_n64_b4", *N64, 4, 1, (ROWS, 4, 1), (2, 64.0), spread=True),
    Case("tile_n70_b1", *N70, 1, 1, (TILE, 16, 1)),
    Case("tile_n70_b16", *N70, 16, 1, (TILE, 16, 1), (8, 64.0), spread=True),
    Case("tile_n70_b16_m60", *N70, 16, 1, (TILE, 16, 1), (8, 64.0), max_iter=60, never=True),
    Case("tile_n70_b17", *N70, 17, 1, (TILE, 16, 2), (9, 64.0), spread=True),
    Case("tile_n6_b1025", *N6, 1025, 1, (TILE, 16, 65), (12, 16.0), spread=True),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
ROW_BY_ROW = 64            # batches up to here: adam_oracle.adam on every row alone; beyond, adam_each_ref


def each_plan(n, B, cus, rows_fit=True, per_cu=1):
    """plan_adam(each = true) restated: dim(action) <= 64 and the batch at 1-4 states per resident workgroup -- as few states per
    workgroup as keep one round of workgroups resident -- is the rows path; 16-state tiles otherwise, any number of them."""
    if n <= 64 and rows_fit:
        per_wg = B if B <= ROWS_MAX else -(-B // (per_cu * cus))
        if 1 <= per_wg <= ROWS_MAX:
            return (ROWS, per_wg, -(-B // per_wg))
    return (TILE, TM, -(-B // TM))


def adam_each_ref(func, obs, n_act, max_iter):
    """adam_oracle.adam with the rule per state, all rows at once: -> (act_best, iters[B], f_best, closest |drift - 1e-3| any
    live state's rule saw).  The mean displacement of a batch of one is the state's own; a fired state is frozen."""
    B = obs.shape[0]
    x = np.zeros((B, n_act))
    mom1, mom2 = np.zeros_like(x), np.zeros_like(x)
    pow1 = pow2 = 1.
    live = np.ones(B, bool)
    iters = np.full(B, max_iter, np.int32)
    drift = np.full(B, np.nan)
    margin = np.inf
    best_x = best_f = None
    for it in range(max_iter):
        f, g = func(obs, x)
        if it == 0:
            best_x, best_f = x.copy(), f.copy()
        else:
            better = live & (f < best_f)
            moved = np.zeros(B)
            moved[better] = np.linalg.norm(x[better] - best_x[better], axis=1)
            best_x[better] = x[better]
            best_f[better] = f[better]
            drift = np.where(np.isnan(drift), moved, adam_oracle.SMOOTH * drift + (1. - adam_oracle.SMOOTH) * moved)
            if it > 5:
                margin = min(margin, float(np.min(np.abs(drift[live] - 1e-3))))
                fire = live & (drift < 1e-3)
                iters[fire] = it
                live = live & ~fire
                if not live.any():
                    break
        gl = g[live]
        mom1[live] = adam_oracle.B1 * mom1[live] + (1. - adam_oracle.B1) * gl
        mom2[live] = adam_oracle.B2 * mom2[live] + (1. - adam_oracle.B2) * (gl * gl)
        pow1 *= adam_oracle.B1
        pow2 *= adam_oracle.B2
        mhat = mom1[live] / (1. - pow1)
        x = x.copy()
        x[live] = np.clip(x[live] - adam_oracle.ALPHA * mhat / (np.sqrt(mom2[live]) + adam_oracle.EPS), -adam_oracle.BOX,
                          adam_oracle.BOX)
    return best_x, iters, best_f, margin


def _fg(spec, params, ctx):
    from oracle import picnn_oracle
    chain = picnn_oracle.make_fg_chain(params, ctx, list(spec.szs), spec.alpha, False)
    return adam_oracle.entropy_fg(lambda obs, act: chain(act))


def oracle_rows(spec, params, ctx, max_iter):
    """adam_oracle.adam on every row alone -> (act_best [B, n], iters [B], f_best [B], closest |drift - 1e-3|)"""
    best, its, fb, margin = [], [], [], np.inf
    for u in range(ctx.shape[0]):
        trace = []
        b, it, f = arch._oracle_adam(spec, params, ctx[u:u + 1], max_iter, drift_trace=trace)
        best.append(b[0]); its.append(it); fb.append(f[0])
        if it > 5:
            margin = min(margin, min(abs(d - 1e-3) for d in trace[5:it]))
    return np.array(best), np.array(its, np.int32), np.array(fb, np.float32), margin


def oracle_each(spec, params, ctx, max_iter):
    if ctx.shape[0] <= ROW_BY_ROW:
        return oracle_rows(spec, params, ctx, max_iter)
    return adam_each_ref(_fg(spec, params, ctx), ctx, spec.n_labels, max_iter)


def _workgroups(c, iters):
    per_wg = c.plan[1]
    return [iters[s:s + per_wg] for s in range(0, c.B, per_wg)]


def _has_spread(c, iters):
    return any(g.max() >= 2 * g.min() for g in _workgroups(c, iters))


# ------------------------------------------------------------------------------------------------ CPU


def test_cases_cover_what_the_contract_names():
    rows = [c for c in CASES if c.plan[0] == ROWS]
    tile = [c for c in CASES if c.plan[0] == TILE]
    assert {1, 2, 4, 5} <= {c.B for c in rows} and any(c.plan[2] > 4 for c in rows)
    assert {1, 6, 64} <= {c.n for c in rows}
    assert {1, 16, 17} <= {c.B for c in tile if c.n == 70}
    assert any(c.n == 6 and -(-c.B // 256) > ROWS_MAX for c in tile)
    assert any(c.B % c.plan[1] and c.plan[2] > 1 for c in rows) and any(c.B % TM and c.plan[2] > 1 for c in tile)
    assert {1, 3, 4} <= {c.plan[1] for c in rows if c.plan[2] > 1}
    assert {c.plan[0] for c in CASES if c.never} == {ROWS, TILE} == {c.plan[0] for c in CASES if c.spread}
    for c in CASES:
        assert each_plan(c.n, c.B, 256) == c.plan, c.name


def test_plan_rule_restated():
    """the rows path while ceil(B / resident workgroups) <= 4, tiles beyond and for n > 64: no residency limit on either"""
    assert each_plan(6, 4, 256) == (ROWS, 4, 1) and each_plan(6, 5, 256) == (ROWS, 1, 5)
    assert each_plan(6, 256, 256) == (ROWS, 1, 256) and each_plan(6, 257, 256) == (ROWS, 2, 129)
    assert each_plan(64, 1024, 256) == (ROWS, 4, 256) and each_plan(64, 1025, 256) == (TILE, 16, 65)
    assert each_plan(65, 1, 256) == (TILE, 16, 1) and each_plan(65, 1 << 20, 256) == (TILE, 16, 1 << 16)
    assert each_plan(6, 1 << 20, 256) == (TILE, 16, 1 << 16)            # beyond what a cooperative launch keeps resident
    assert each_plan(6, 9, 2) == (TILE, 16, 1) and each_plan(6, 8, 2) == (ROWS, 4, 2)


@pytest.mark.parametrize("name", IDS)
def test_each_state_fires_clear_of_the_threshold(name):
    """CPU screen on the chain-order context rows: every rule decision keeps 1e-9 from the threshold; the cases marked `spread`
    hold, in one workgroup, states whose stop iterations differ by a factor of two or more; the `never` cases hold a state
    that fires and one that runs to max_iter; every other case fires in every state."""
    c = BY_NAME[name]
    spec, params, obs = arch._case_problem(c)
    ctx = arch._chain_rows(spec, params, obs)
    best, iters, f_best, margin = oracle_each(spec, params, ctx, c.max_iter)
    groups = _workgroups(c, iters)
    print("%s: iters %d .. %d, closest |drift - 1e-3| %.2e, largest ratio inside a workgroup %.1f"
          % (name, iters.min(), iters.max(), margin, max(g.max() / g.min() for g in groups)))
    assert margin >= 1e-9 and iters.min() >= 6
    if c.never:
        assert iters.max() == c.max_iter and iters.min() < c.max_iter
        assert any(g.max() == c.max_iter and g.min() < c.max_iter for g in groups)      # in ONE workgroup
    else:
        assert iters.max() < c.max_iter
    if c.spread:
        assert _has_spread(c, iters)


@pytest.mark.parametrize("name", ["rows_n6_b37", "tile_n70_b17", "rows_n6_b4_m10"])
def test_all_rows_restatement_is_the_oracle_row_by_row(name):
    """adam_each_ref, which the large batches are compared with, against adam_oracle.adam on every row alone: bits"""
    c = BY_NAME[name]
    spec, params, obs = arch._case_problem(c)
    ctx = arch._chain_rows(spec, params, obs)
    rows = oracle_rows(spec, params, ctx, c.max_iter)
    ref = adam_each_ref(_fg(spec, params, ctx), ctx, spec.n_labels, c.max_iter)
    assert np.array_equal(rows[1], ref[1]) and len(set(ref[1].tolist())) > 1
    assert np.array_equal(rows[0], ref[0]) and np.array_equal(rows[2], ref[2])
    assert rows[3] == ref[3]


def test_each_entry_is_declared_and_refuses_what_the_batch_entry_refuses():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    for name in ("icnn_be_adam_fc_each", "icnn_be_debug_adam_each_plan"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in header
    spec = arch._spec(*N6)
    buf = (C.c_double * 64)()
    p = C.addressof(buf)

    def call(entry, model, ctx=p, batch=4, max_iter=10, act=p, f=p, iters=p, ws=p):
        return getattr(lib, entry)(C.byref(model) if model is not None else None, ctx, batch, max_iter, act, f, iters, ws, None)

    def model(**kw):
        m = arch._c_model(spec)
        m.wpack = p
        for k, v in kw.items():
            setattr(m, k, v)
        return m
    bad_shape = model()
    bad_shape.width[spec.n_layers - 1] = 2
    refused = [dict(model=None), dict(model=model(wpack=None)), dict(model=model(action_box=1)), dict(model=bad_shape),
               dict(model=model(ctx_width=7)), dict(model=model(), ctx=None), dict(model=model(), act=None),
               dict(model=model(), f=None), dict(model=model(), iters=None), dict(model=model(), ws=None),
               dict(model=model(), batch=-1), dict(model=model(), max_iter=0)]
    for kw in refused:
        rc = call("icnn_be_adam_fc", **kw)
        assert rc < 0 and call("icnn_be_adam_fc_each", **kw) == rc, kw
    out = (C.c_int * 2)()
    assert lib.icnn_be_debug_adam_each_plan(None, 4, C.byref(out)) == -1
    assert lib.icnn_be_debug_adam_each_plan(C.byref(model()), 0, C.byref(out)) == -1
    assert lib.icnn_be_debug_adam_each_plan(C.byref(model(action_box=1)), 4, C.byref(out)) == -1
    assert lib.icnn_be_debug_adam_each_plan(C.byref(model()), 4, None) == -1


def test_solver_shapes_on_the_host():
    """AdamSolver(stop=...): iters is [B] for "each", 0-d for "batch"; anything else is refused"""
    from icnn_amd import rl_adam
    stub = types.SimpleNamespace(spec=types.SimpleNamespace(action_box=False, n_labels=6), device=torch.device("cpu"))
    each = rl_adam.AdamSolver(stub, 5, 30, stop="each")
    assert each.iters.shape == (5,) and each.iters.dtype == torch.int32 and each.act_best.shape == (5, 6)
    assert each.solve_obs(torch.zeros(5, 3)) is None
    assert rl_adam.AdamSolver(stub, 5, 30).iters.shape == () and rl_adam.AdamSolver(stub, 5, 30, stop="batch").stop == "batch"
    with pytest.raises(ValueError):
        rl_adam.AdamSolver(stub, 5, 30, stop="state")


# ------------------------------------------------------------------------------------------------ GPU


def _device_problem(c):
    spec, params, obs = arch._case_problem(c)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(obs))[:c.B].contiguous()
    return spec, params, model, ctx


def _solve_each(model, ctx, max_iter):
    from icnn_amd import rl_adam
    res = rl_adam.AdamSolver(model, ctx.shape[0], max_iter, stop="each").solve(ctx)
    torch.cuda.synchronize()
    return res.act_best.clone(), res.f_best.clone(), res.iters.clone()


def _solve_alone(model, ctx, max_iter):
    """icnn_be_adam_fc on every row as a batch of one -> (act_best [B, n], f_best [B], iters [B])"""
    from icnn_amd import rl_adam
    one = rl_adam.AdamSolver(model, 1, max_iter)
    act, f, its = [], [], []
    for u in range(ctx.shape[0]):
        r = one.solve(ctx[u:u + 1])
        act.append(r.act_best.clone()); f.append(r.f_best.clone()); its.append(r.iters.clone().reshape(1))
    torch.cuda.synchronize()
    return torch.cat(act), torch.cat(f), torch.cat(its)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_each_row_is_the_batch_of_one(name):
    c = BY_NAME[name]
    spec, params, model, ctx = _device_problem(c)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    plan = _lib.adam_each_plan(model.c_model, c.B)
    print("%s: plan %s on %d CUs" % (name, plan, cus))
    assert plan == each_plan(c.n, c.B, cus) and (cus != 256 or plan == c.plan)
    act, f, its = _solve_each(model, ctx, c.max_iter)
    assert its.shape == (c.B,) and its.dtype == torch.int32
    # ---- the device's own batch rule on every row alone
    act1, f1, its1 = _solve_alone(model, ctx, c.max_iter)
    print("%s: against icnn_be_adam_fc at batch 1: %d iters, %d of %d actions, %d energies differ"
          % (name, int((its != its1).sum()), int((act != act1).sum()), act.numel(), int((f != f1).sum())))
    assert torch.equal(its, its1) and torch.equal(act, act1) and torch.equal(f, f1)
    # ---- the oracle on every row alone, on the context the device used
    best, iters, f_best, margin = oracle_each(spec, params, ctx.cpu().numpy(), c.max_iter)
    got, got_f, got_its = act.cpu().numpy(), f.cpu().numpy(), its.cpu().numpy()
    print("%s: oracle iters %d .. %d, closest |drift - 1e-3| %.2e; %d iters, %d of %d actions (max %.2e), %d energies differ"
          % (name, iters.min(), iters.max(), margin, int((got_its != iters).sum()), int((got != best).sum()), best.size,
             float(np.max(np.abs(got - best))), int((got_f != f_best).sum())))
    assert margin >= 1e-9
    if c.spread:
        assert _has_spread(c, iters)
    if c.never:
        assert iters.max() == c.max_iter > iters.min()
    assert np.array_equal(got_its, iters)
    assert np.array_equal(got, best)
    assert np.array_equal(got_f, f_best)
    assert np.all(np.abs(got) <= 1.0 - 1e-8)


@pytest.mark.gpu
def test_a_row_does_not_depend_on_its_batch():
    """rows 0-4 in a batch of 5 and in a batch of 37 (the other 32 states stop anywhere between 6 and 55): the same bits"""
    c = BY_NAME["rows_n6_b37"]
    spec, params, model, ctx = _device_problem(c)
    big = _solve_each(model, ctx, c.max_iter)
    small = _solve_each(model, ctx[:5].contiguous(), c.max_iter)
    assert len(set(big[2].tolist())) > 4
    for a, b in zip(small, big):
        assert torch.equal(a, b[:5])
    # and across the two kernels: the same rows inside 16-state tiles (n = 6 beyond the rows plan)
    t = BY_NAME["tile_n6_b1025"]
    _, _, tmodel, tctx = _device_problem(t)
    assert torch.equal(tctx[:5], ctx[:5])
    tiles = _solve_each(tmodel, tctx, t.max_iter)
    for a, b in zip(small, tiles):
        assert torch.equal(a, b[:5])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["rows_n6_b4", "rows_n6_b5", "tile_n70_b17"])
def test_a_nan_state_stays_alone(name):
    """A NaN context entry in state 2: the launch ends, and every other state keeps its bits"""
    c = BY_NAME[name]
    spec, params, model, ctx = _device_problem(c)
    clean = _solve_each(model, ctx, c.max_iter)
    bad = ctx.clone()
    bad[2, 0] = float("nan")
    got = _solve_each(model, bad, c.max_iter)            # synchronises: the launch has ended
    keep = torch.arange(c.B, device=ctx.device) != 2
    for a, b in zip(got, clean):
        assert torch.equal(a[keep], b[keep])
    assert 6 <= int(got[2][2]) <= c.max_iter
    assert bool(torch.all(got[0][2].abs() <= 1.0 - 1e-8))
