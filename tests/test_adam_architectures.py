"""The inner Adam kernels (be_adam.hip) off the agent's shape, the batch-wide stopping rule included.

tests/test_adam.py reaches the HalfCheetah network and two other architectures; on its large launches the rule
`drift < 1e-3 && it > 5` never fires before max_iter, so the one thing grid_sum (the exchange of one double per workgroup)
decides is never decided there.  Every case below is screened on the CPU so that the rule FIRES, with the smoothed
displacement at least 1e-9 away from 1e-3 at every iteration the rule looks at (the device sums at most a few thousand
non-negative float64 terms in another order than NumPy: a relative difference below 1e-12), and so that a sum which lost
the workgroups behind grid_sum's first pass of 64 -- or, where stated, only the ragged last workgroup -- would stop at
ANOTHER iteration.  Each case names the launch it is meant to get on the 256-CU device (icnn_be_debug_adam_plan:
kernel, states per workgroup, workgroups, cooperative); the GPU test asserts that plan first.

Specs as tests/test_adam.py builds them (halfcheetah_spec with action_box=False and other sizes, "spread" weights); max_iter
400.  `x16 last 12`: the observations of the last 12 states are multiplied by 16.  stop = the oracle's iteration count on
the chain-order context rows; -64 = the same with the workgroups 64.. left out of the sum, -last = with the last one left out.

  case          hidden        obs  n   B     launch                                 stop   -64   -last
  tile_n65_b1   (24,)          9   65  1     adam_fc_kernel, 1 tile, one real state   51
  tile_n65_b16  (32, 24)       9   65  16    adam_fc_kernel, 1 full tile             107
  tile_n65_b17  (32, 24)       9   65  17    adam_fc_kernel, 2 tiles (16 + 1)        108          107
  tile_b1025    (24, 16)       7   6   1025  adam_fc_kernel, 65 tiles (last: 1)       80    79     79    x64 last 1
  tile_b1100    (24, 16)       7   6   1100  adam_fc_kernel, 69 tiles (last: 12)      81    79     80    x64 last 12
  tile_b1104    (24, 16)       7   6   1104  adam_fc_kernel, 69 full tiles            83    77
  rows_n64_b3   (40, 24)       9   64  3     adam_rows_kernel, 1 workgroup of 3       79
  rows_n64_b17  (40, 24)       9   64  17    adam_rows_kernel, 17 x 1                 88
  rows_n1_six   (16,)          5   1   3     adam_rows_kernel, 1 workgroup of 3        6
  rows_n1       (16,)          5   1   3     adam_rows_kernel, 1 workgroup of 3       17
  rows_L1       (30,)          9   6   2     adam_rows_kernel, 1 workgroup of 2       54
  rows_deep8    (20,) x 7      9   20  40    adam_rows_kernel, 40 x 1                243                 x3 all
  rows_n49_b301 (30, 20)       9   49  301   adam_rows_kernel, 151 x 2 (last: 1)     132    90    130    x64 last 1
  rows_b700     (24, 16)       7   6   700   adam_rows_kernel, 234 x 3 (last: 1)      83    55     77    x16 last 1
  rows_b902     (24, 16)       7   6   902   adam_rows_kernel, 226 x 4 (last: 2)      83    59     83    x16 last 2
  rows_b1024    (24, 16)       7   6   1024  adam_rows_kernel, 256 x 4                83    54

rows_n1_six: no state ever improves on act = 0, every displacement is zero and the rule fires at iteration 6, the first it
allows (`it > 5`); rows_n1 is the same network on a seed where the actions do move.  rows_deep8 (ICNN_BE_MAX_LAYERS): 154
components of the oracle's best actions end ON the wall +-(1 - 1e-8), asserted on the oracle side.

Not reached: the ragged last workgroup of rows_b902 (two states of 902) does not move the stop iteration on any of the
seeds and scalings tried (seeds 1-8, x16 and x64); the two other ragged rows cases and the three ragged tile cases do
reach it.  No spec that fc_check_model accepts has n <= 64 and a four-row rows layout beyond 160 KB (the tile layout of
be_picnn_fc_dev.h bounds the sum of the padded widths at 2560 - 136 (L + 2) floats per row, which bounds rows_layout's row at
under 8000 floats: 125 KB for four), so n <= 64 reaches adam_fc_kernel through the batch size only
(test_no_accepted_spec_outgrows_the_rows_layout checks the widest accepted nets).

solve_obs (the in-kernel context producer rows_context_from_obs) off the shipped spec: OBS_SPECS / OBS_CASES below, and the
scratch guard `2 * wmax > ctx_off` at its boundary, from a restatement of rows_layout."""
import dataclasses

import numpy as np
import pytest
import torch

from icnn_amd import _lib, picnn
from oracle import adam_oracle, picnn_oracle

CUS = 256                   # the plans below are stated for the MI355X: one resident workgroup of either kernel per CU
MAX_ITER = 400
ROWS, TILE = "ROWS", "TILE"


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    widths: tuple
    n_obs: int
    n: int
    B: int
    seed: int
    plan: tuple               # (kernel, states per workgroup, workgroups, cooperative)
    stop: int                 # the oracle's iteration count on the chain-order context rows
    scale: tuple = None       # (how many of the last states, factor on their observations)
    stop_first_64: int = None     # ... with the workgroups 64.. left out of the batch sum
    stop_without_last: int = None  # ... with only the last workgroup left out (None: not claimed to differ)
    max_iter: int = MAX_ITER


CASES = [
    Case("tile_n65_b1", (24,), 9, 65, 1, 1, (TILE, 16, 1, False), 51),
    Case("tile_n65_b16", (32, 24), 9, 65, 16, 1, (TILE, 16, 1, False), 107),
    Case("tile_n65_b17", (32, 24), 9, 65, 17, 1, (TILE, 16, 2, True), 108, stop_without_last=107),
    Case("tile_b1025", (24, 16), 7, 6, 1025, 7, (TILE, 16, 65, True), 80, (1, 64.0), 79, 79),
    Case("tile_b1100", (24, 16), 7, 6, 1100, 5, (TILE, 16, 69, True), 81, (12, 64.0), 79, 80),
    Case("tile_b1104", (24, 16), 7, 6, 1104, 1, (TILE, 16, 69, True), 83, None, 77),
    Case("rows_n64_b3", (40, 24), 9, 64, 3, 1, (ROWS, 3, 1, False), 79),
    Case("rows_n64_b17", (40, 24), 9, 64, 17, 1, (ROWS, 1, 17, True), 88),
    Case("rows_n1_six", (16,), 5, 1, 3, 2, (ROWS, 3, 1, False), 6),
    Case("rows_n1", (16,), 5, 1, 3, 1, (ROWS, 3, 1, False), 17),
    Case("rows_L1", (30,), 9, 6, 2, 1, (ROWS, 2, 1, False), 54),
    Case("rows_deep8", (20,) * 7, 9, 20, 40, 1, (ROWS, 1, 40, True), 243, (40, 3.0)),
    Case("rows_n49_b301", (30, 20), 9, 49, 301, 4, (ROWS, 2, 151, True), 132, (1, 64.0), 90, 130),
    Case("rows_b700", (24, 16), 7, 6, 700, 1, (ROWS, 3, 234, True), 83, (1, 16.0), 55, 77),
    Case("rows_b902", (24, 16), 7, 6, 902, 1, (ROWS, 4, 226, True), 83, (2, 16.0), 59),
    Case("rows_b1024", (24, 16), 7, 6, 1024, 1, (ROWS, 4, 256, True), 83, None, 54),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
WALL_COMPONENTS = {"rows_deep8": 100}        # at least so many components of the oracle's best actions on the wall


def _spec(widths, n_obs, n, **kw):
    return dataclasses.replace(picnn.halfcheetah_spec(), action_box=False, szs=tuple(widths), n_features=n_obs, n_labels=n, **kw)


def _problem(widths, n_obs, n, B, seed, scale=None, **kw):
    """tests/test_adam.py's _negq_problem, with the observations of the last scale[0] states multiplied by scale[1]"""
    spec = _spec(widths, n_obs, n, **kw)
    params = picnn.init_params(spec, seed, "spread", yu_bias=1.0, gate_bias=1.0)
    obs = np.random.RandomState(100 + seed).randn(max(B, 1), n_obs).astype(np.float32)
    if scale is not None:
        obs[-scale[0]:] *= np.float32(scale[1])
    return spec, params, obs


def _case_problem(c):
    return _problem(c.widths, c.n_obs, c.n, c.B, c.seed, c.scale)


def _oracle_adam(spec, params, ctx_host, max_iter, **kw):
    chain = picnn_oracle.make_fg_chain(params, ctx_host, list(spec.szs), spec.alpha, False)
    func = adam_oracle.entropy_fg(lambda obs, act: chain(act))
    return adam_oracle.adam(func, ctx_host, spec.n_labels, max_iter, **kw)


def _chain_rows(spec, params, obs):
    return picnn_oracle.context_rows_chain(params, obs, list(spec.szs), picnn.stage_weights(spec, params))


def _workgroup_of(c):
    return np.arange(c.B) // c.plan[1]


def _need_256_cus():
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != CUS:
        print("skipped: the plans of this module are stated for %d CUs, the device has %d" % (CUS, cus))
        pytest.skip("the plans of this module are stated for %d CUs, the device has %d" % (CUS, cus))


# ------------------------------------------------------------------------------------------------ CPU: the table


def test_cases_cover_the_paths():
    plans = {c.plan for c in CASES}
    assert {1, 2} <= {p[2] for p in plans if p[0] == TILE} and any(p[0] == TILE and p[2] > 64 for p in plans)
    assert (TILE, 16, 1, False) in plans                                        # the single non-cooperative tile
    assert {1, 2, 3, 4} <= {p[1] for p in plans if p[0] == ROWS and p[2] > 1}   # states per workgroup over several workgroups
    assert (ROWS, 4, 256, True) in plans                                        # four states in every workgroup
    assert {1, 49, 64, 65} <= {c.n for c in CASES}
    assert {1, 7} <= {len(c.widths) for c in CASES} and _spec((20,) * 7, 9, 20).n_layers == _lib.MAX_LAYERS
    assert {c.n for c in CASES if c.plan[0] == TILE and c.plan[2] == 1} == {65}
    assert any(c.plan[0] == TILE and c.n <= 64 for c in CASES)
    for c in CASES:
        kernel, per_wg, wgs, coop = c.plan
        assert wgs == (c.B + per_wg - 1) // per_wg and coop == (wgs > 1), c.name
        assert (c.stop_first_64 is not None) == (wgs > 64), c.name              # every case past grid_sum's first pass claims it
        if kernel == ROWS:      # one resident workgroup per CU: as few states per workgroup as keep them all resident
            assert c.n <= 64 and per_wg == (c.B if c.B <= 4 else (c.B + CUS - 1) // CUS) <= 4, c.name
        else:
            assert per_wg == 16 and wgs <= CUS and (c.n > 64 or (c.B + CUS - 1) // CUS > 4), c.name
    ragged = [c for c in CASES if c.stop_without_last is not None]
    assert all(c.B % c.plan[1] for c in ragged) and {c.plan[0] for c in ragged} == {ROWS, TILE}
    # ragged last workgroups over several workgroups at 2, 3 and 4 states per workgroup
    assert {2, 3, 4} <= {c.plan[1] for c in CASES if c.plan[0] == ROWS and c.plan[2] > 1 and c.B % c.plan[1]}
    assert {2, 3} <= {c.plan[1] for c in ragged if c.plan[0] == ROWS}


@pytest.mark.parametrize("name", IDS)
def test_the_stopping_rule_fires_and_every_workgroup_counts(name):
    """CPU screen on the chain-order context rows: the rule fires (6 <= iters < max_iter, at the iteration the table
    states), the smoothed displacement keeps 1e-9 from the threshold wherever the rule reads it, and the stop iteration
    changes when the sum loses the workgroups a wrong grid_sum would lose."""
    c = BY_NAME[name]
    spec, params, obs = _case_problem(c)
    ctx = _chain_rows(spec, params, obs)
    trace = []
    best, iters, f_best = _oracle_adam(spec, params, ctx, c.max_iter, drift_trace=trace)
    margin = min(abs(d - 1e-3) for d in trace[5:iters])          # trace[it - 1] is iteration it's: iterations 6 .. the stop
    print("%s: the oracle stops at %d of %d, closest |drift - 1e-3| = %.2e" % (name, iters, c.max_iter, margin))
    assert 6 <= iters < c.max_iter and iters == c.stop
    assert len(trace) == iters and trace[iters - 1] < 1e-3
    assert margin >= 1e-9
    wg, wgs = _workgroup_of(c), c.plan[2]
    if wgs > 64:                # grid_sum polls and sums 64 workgroups per pass: the second pass must count
        _, lost, _ = _oracle_adam(spec, params, ctx, c.max_iter, moved_mask=wg < 64)
        print("%s: without workgroups 64..%d the rule fires at %d" % (name, wgs - 1, lost))
        assert lost == c.stop_first_64 != iters
    if c.stop_without_last is not None:
        _, lost, _ = _oracle_adam(spec, params, ctx, c.max_iter, moved_mask=wg < wgs - 1)
        print("%s: without the ragged last workgroup the rule fires at %d" % (name, lost))
        assert lost == c.stop_without_last != iters
    if name in WALL_COMPONENTS:
        on_wall = int((np.abs(best) == 1.0 - 1e-8).sum())
        print("%s: %d of %d components of the best actions on the wall" % (name, on_wall, best.size))
        assert on_wall >= WALL_COMPONENTS[name]
    if name == "rows_n1_six":
        assert max(trace) == 0.0 and not best.any()              # nothing ever improves on act = 0 (module docstring)
    else:
        assert np.abs(best).max() > 0.01


def test_oracle_diagnostics_leave_the_result_alone():
    """drift_trace and moved_mask are read-only taps: same iterates, and an all-True mask is no mask."""
    c = BY_NAME["rows_L1"]
    spec, params, obs = _case_problem(c)
    ctx = _chain_rows(spec, params, obs)
    plain = _oracle_adam(spec, params, ctx, c.max_iter)
    trace = []
    tapped = _oracle_adam(spec, params, ctx, c.max_iter, drift_trace=trace, moved_mask=np.ones(c.B, bool))
    assert plain[1] == tapped[1] == len(trace) and np.array_equal(plain[0], tapped[0]) and np.array_equal(plain[2], tapped[2])
    none = _oracle_adam(spec, params, ctx, c.max_iter, moved_mask=np.zeros(c.B, bool))
    assert none[1] == 6 < plain[1]                               # no displacement at all: the first iteration the rule allows


# ------------------------------------------------------------------------------------------------ the rows layout, restated


def _pad16(v):
    return (v + 15) & ~15


def _kblocks(k):
    return (_pad16(k) // 16 + 4) // 5 * 5


def rows_layout(spec, rows=4):
    """rows_layout (be_picnn_fc_rows_dev.h) restated: (ctx_off, floats of one state's row, LDS bytes of adam_rows_kernel).
    Before the context row: the L chained operands y * yu_i (padded k-blocks), ysc, g, g0, the L activations, delta and gw."""
    n, w, L = spec.n_labels, list(spec.szs), len(spec.szs)
    npad = _pad16(n)
    ctx_off = L * _kblocks(n) * 16 + 3 * npad + sum(_kblocks(v) * 16 for v in w) + _kblocks(w[-1]) * 16 + _pad16(w[-1])
    row = ctx_off + ((spec.ctx_width + 3) & ~3)
    return ctx_off, row, (rows * row + _pad16(w[-1]) + npad + 4) * 4 + (4 + 1) * 8


def _lds_pitch(width):
    p = _kblocks(width) * 16
    while p & 63 != 8:
        p += 4
    return p


def _tile_bytes(spec):
    """fill_args (be_picnn_fc_dev.h): the LDS of one 16-row tile; fc_check_model refuses a model beyond 160 KB"""
    L = len(spec.szs)
    return 4 * 16 * (_lds_pitch(spec.n_labels) * (L + 2) + sum(_lds_pitch(v) for v in spec.szs) + _lds_pitch(spec.szs[-1]))


def _c_model(spec):
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = spec.alpha, 0, spec.ctx_width
    return m


def test_no_accepted_spec_outgrows_the_rows_layout():
    """n <= 64: the widest nets fc_check_model accepts, at one, two and seven hidden layers, keep four rows within 160 KB, so
    the rows kernel is left through the batch size only (module docstring).  The tile restatement is checked against the
    library on both sides of its limit."""
    lib = _lib.load()
    import ctypes as C
    for L in (1, 2, 7):
        widest = 0
        for w in range(16, 4000, 16):
            spec = _spec((w,) * L, 9, 64)
            accepted = lib.icnn_be_fc_pack_floats(C.byref(_c_model(spec))) > 0
            assert accepted == (_tile_bytes(spec) <= 160 * 1024), (L, w)
            if not accepted:
                break
            widest = w
        assert widest >= 64
        spec = _spec((widest,) * L, 9, 64)
        print("L = %d: widest accepted hidden width %d, four rows take %d bytes" % (L, widest, rows_layout(spec)[2]))
        assert rows_layout(spec)[2] <= 160 * 1024
    for c in CASES:
        spec = _spec(c.widths, c.n_obs, c.n)
        assert _tile_bytes(spec) <= 160 * 1024 and (c.n > 64 or rows_layout(spec)[2] <= 160 * 1024), c.name


# ------------------------------------------------------------------------------------------------ GPU: one test per case


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_adam_kernel_matches_oracle_on_its_planned_launch(name):
    """The case's plan first; then AdamSolver.solve on model.context(obs) against the oracle on that same context, with the
    bars of tests/test_adam.py: equal iteration counts, |act_best - oracle| <= 1e-9, |f_best - oracle| <= 1e-6, the box."""
    from icnn_amd import rl_adam
    _need_256_cus()
    c = BY_NAME[name]
    spec, params, obs = _case_problem(c)
    model = picnn.FCModel(spec, params)
    plan = _lib.adam_plan(model.c_model, c.B)
    print("%s: plan %s" % (name, plan))
    assert plan == c.plan + (False,), plan
    ctx = model.context(torch.from_numpy(obs))[:c.B].contiguous()
    res = rl_adam.AdamSolver(model, c.B, c.max_iter).solve(ctx)
    torch.cuda.synchronize()
    trace = []
    best, iters, f_best = _oracle_adam(spec, params, ctx.cpu().numpy(), c.max_iter, drift_trace=trace)
    got, got_iters = res.act_best.cpu().numpy(), int(res.iters.item())
    margin = min(abs(d - 1e-3) for d in trace[5:iters]) if iters > 5 else float("nan")
    print("%s: %d iterations (oracle %d on this context, %d on the chain-order rows), closest |drift - 1e-3| %.2e, "
          "max |d act_best| %.3e, max |d f_best| %.3e" % (name, got_iters, iters, c.stop, margin, np.max(np.abs(got - best)),
                                                           np.max(np.abs(res.f_best.cpu().numpy() - f_best))))
    assert 6 <= iters < c.max_iter and margin >= 1e-9            # the screen, on the GEMM context
    assert got_iters == iters
    assert np.max(np.abs(got - best)) <= 1e-9
    assert np.max(np.abs(res.f_best.cpu().numpy() - f_best)) <= 1e-6
    assert np.all(np.abs(got) <= 1.0 - 1e-8)


# ------------------------------------------------------------------------------------------------ solve_obs


# (hidden widths, n_features, n): no BatchNorm, the last u-layer linear
OBS_SPECS = {
    "L1": ((30,), 9, 6),                      # one hidden layer: the only u-layer is the linear one
    "L3": ((48, 20, 33), 11, 20),             # uneven widths, two ReLU'd u-layers and the linear one
    "deep8": ((20,) * 7, 9, 20),              # ICNN_BE_MAX_LAYERS
    "f3": ((24, 16), 3, 6),                   # K = 3: the single-step loop alone
    "f45": ((24, 16), 45, 6),                 # K = 45 = 32 + 8 + 5
    "w300": ((300, 24), 17, 6),               # 606 columns in stage 0 (a second trip of col += 512), K = 300 in stage 1
}
# (spec, batch) -> (states per workgroup, workgroups): every spec at two batches, every batch of {1, 4, 5, 700} three times
OBS_CASES = [("L1", 1, (1, 1)), ("L1", 700, (3, 234)), ("L3", 4, (4, 1)), ("L3", 5, (1, 5)), ("deep8", 1, (1, 1)),
             ("deep8", 5, (1, 5)), ("f3", 4, (4, 1)), ("f3", 700, (3, 234)), ("f45", 1, (1, 1)), ("f45", 5, (1, 5)),
             ("w300", 4, (4, 1)), ("w300", 700, (3, 234))]
OBS_SEED = 3


def test_obs_cases_cover_the_producer():
    assert {len(w) for w, _, _ in OBS_SPECS.values()} >= {1, 3, 7}
    assert {f for _, f, _ in OBS_SPECS.values()} >= {3, 45} and {b for _, b, _ in OBS_CASES} == {1, 4, 5, 700}
    w, f, n = OBS_SPECS["w300"]
    assert w[0] + n + w[0] > 512 and 300 % 32 == 12                  # stage 0's columns; K = 300 = 9 * 32 + 8 + 4
    for name, B, (per_wg, wgs) in OBS_CASES:
        assert per_wg == (B if B <= 4 else (B + CUS - 1) // CUS) and wgs == (B + per_wg - 1) // per_wg
        w, f, n = OBS_SPECS[name]
        assert 2 * max(w + (f,)) <= rows_layout(_spec(w, f, n))[0], name      # inside the scratch guard


@pytest.mark.parametrize("name", list(OBS_SPECS))
def test_chain_context_restates_these_architectures(name):
    """CPU: oracle/picnn_chain.c's context rows against the float64 statement of the context, to the bar
    test_adam_from_observations_in_one_launch uses between the two device contexts (2e-5 of the largest entry)."""
    w, f, n = OBS_SPECS[name]
    spec, params, obs = _problem(w, f, n, 5, OBS_SEED)
    ref = picnn_oracle.flat_context(picnn_oracle.context(params, obs, list(spec.szs), False, dtype=np.float64), dtype=np.float64)
    got = _chain_rows(spec, params, obs)
    assert got.shape == ref.shape == (5, spec.ctx_width) and ref.dtype == np.float64
    err, scale = float(np.max(np.abs(got - ref))), float(np.abs(ref).max())
    print("%s: max|chain - float64| = %.2e, bound 2e-5 * %.2e" % (name, err, scale))
    assert err <= 2e-5 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name,B,launch", OBS_CASES, ids=["%s_%d" % c[:2] for c in OBS_CASES])
def test_adam_from_observations_off_the_shipped_spec(name, B, launch):
    """solve_obs against the oracle's Adam on the chain-order context rows: same iteration count, bit-identical actions."""
    from icnn_amd import rl_adam
    _need_256_cus()
    w, f, n = OBS_SPECS[name]
    spec, params, obs = _problem(w, f, n, B, OBS_SEED)
    model = picnn.FCModel(spec, params)
    plan = _lib.adam_plan(model.c_model, B, model.c_ctx)
    print("%s B=%d: plan %s" % (name, B, plan))
    assert plan == (ROWS,) + launch + (launch[1] > 1, True), plan
    res = rl_adam.AdamSolver(model, B, MAX_ITER).solve_obs(torch.from_numpy(obs))
    assert res is not None
    torch.cuda.synchronize()
    best, iters, f_best = _oracle_adam(spec, params, _chain_rows(spec, params, obs), MAX_ITER)
    got = res.act_best.cpu().numpy()
    print("%s B=%d: %d iterations (oracle %d), %d of %d actions differ" % (name, B, int(res.iters.item()), iters,
                                                                          int((got != best).sum()), best.size))
    assert int(res.iters.item()) == iters
    assert np.array_equal(got, best)
    assert np.array_equal(res.f_best.cpu().numpy(), f_best)


GUARD_SPECS = [((24, 16), 6), ((30,), 6)]         # (hidden widths, n): ctx_off 464 and 320


def test_scratch_guard_restatement():
    assert [rows_layout(_spec(w, 9, n))[0] for w, n in GUARD_SPECS] == [464, 320]
    # (24, 16), n = 6: two operands of 80 | ysc, g, g0 of 16 | z_0, z_1 of 80 | delta 80 | gw 16
    assert 2 * 80 + 3 * 16 + 2 * 80 + 80 + 16 == 464


@pytest.mark.gpu
def test_obs_scratch_guard_at_its_boundary():
    """The in-kernel producer keeps two vectors of wmax = max(n_features, hidden widths) floats in the row's operand
    region, [0, ctx_off): the launch accepts 2 * wmax <= ctx_off and nothing beyond.  With more features than hidden units
    the largest accepted n_features is ctx_off / 2 (ctx_off from the restated layout); there solve_obs must still equal
    the oracle bit for bit -- an off-by-one in the guard overwrites the first entries of the context row --, and one feature
    more is refused: solve_obs returns None and rl_adam.adam(one_launch=True) falls back to context + Adam."""
    from icnn_amd import rl_adam
    _need_256_cus()
    B = 3
    for widths, n in GUARD_SPECS:
        ctx_off = rows_layout(_spec(widths, 9, n))[0]
        accepted = {}
        for f in (ctx_off // 2 - 1, ctx_off // 2, ctx_off // 2 + 1, ctx_off // 2 + 2):
            spec, params, obs = _problem(widths, f, n, B, OBS_SEED)
            model = picnn.FCModel(spec, params)
            plan = _lib.adam_plan(model.c_model, B, model.c_ctx)
            assert plan[:4] == (ROWS, B, 1, False), plan
            accepted[f] = plan[4]
        print("hidden %s n=%d: ctx_off %d, obs form accepted %s" % (widths, n, ctx_off, accepted))
        assert max(f for f, ok in accepted.items() if ok) == ctx_off // 2 and accepted[ctx_off // 2 - 1]
        assert not accepted[ctx_off // 2 + 1] and not accepted[ctx_off // 2 + 2]
    widths, n = GUARD_SPECS[0]
    edge = rows_layout(_spec(widths, 9, n))[0] // 2
    # ---- the largest accepted width (232 = 7 * 32 + 8 features)
    spec, params, obs = _problem(widths, edge, n, B, OBS_SEED)
    model = picnn.FCModel(spec, params)
    res = rl_adam.AdamSolver(model, B, MAX_ITER).solve_obs(torch.from_numpy(obs))
    assert res is not None
    best, iters, _ = _oracle_adam(spec, params, _chain_rows(spec, params, obs), MAX_ITER)
    assert 6 <= iters < MAX_ITER and int(res.iters.item()) == iters
    assert np.array_equal(res.act_best.cpu().numpy(), best)
    # ---- one more: refused, and the wrapper falls back
    spec, params, obs = _problem(widths, edge + 1, n, B, OBS_SEED)
    model = picnn.FCModel(spec, params)
    assert rl_adam.AdamSolver(model, B, MAX_ITER).solve_obs(torch.from_numpy(obs)) is None
    act = rl_adam.adam(model, torch.from_numpy(obs), max_iter=MAX_ITER, one_launch=True)
    ctx = model.context(torch.from_numpy(obs)).cpu().numpy()
    best, iters, _ = _oracle_adam(spec, params, ctx, MAX_ITER)
    assert 6 <= iters < MAX_ITER
    assert np.max(np.abs(act.cpu().numpy() - best)) <= 1e-9


@pytest.mark.gpu
def test_one_launch_falls_back_for_a_relu_last_u_model():
    """A BatchNorm-free model whose last u-layer is ReLU'd (FCSpec.relu_last_u): the in-kernel producer keeps that layer
    linear and the library refuses the description (ICNN_BE_EINVAL, tests/test_synth_picnn.py, tests/test_host_and_abi.py),
    so solve_obs answers None before calling it and adam(one_launch=True) is context + Adam: identical to one_launch=False."""
    from icnn_amd import rl_adam
    spec, params, obs = _problem((24, 16), 7, 6, 3, OBS_SEED, relu_last_u=True)
    model = picnn.FCModel(spec, params)
    assert model.c_ctx.u_last_relu == 1
    assert rl_adam.AdamSolver(model, 3, MAX_ITER).solve_obs(torch.from_numpy(obs)) is None
    two = rl_adam.adam(model, torch.from_numpy(obs), max_iter=MAX_ITER, one_launch=False).clone()
    one = rl_adam.adam(model, torch.from_numpy(obs), max_iter=MAX_ITER, one_launch=True)
    assert torch.equal(one, two)
    # the ReLU is in what it computed: the linear-last-u twin of the same parameters gives other actions
    twin = picnn.FCModel(dataclasses.replace(spec, relu_last_u=False), params)
    assert not torch.equal(rl_adam.adam(twin, torch.from_numpy(obs), max_iter=MAX_ITER), two)
