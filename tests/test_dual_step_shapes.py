"""One round of the dual step (icnn_amd/csrc/be_dual_dev.h dual_step_body, be_dual_small_dev.h dual_step_quad_rl) at every kernel
instance choose_dual_step / launch_dual_step_small can pick, on both sides of every branch on the bundle size k and on the padded
row width, on states written by hand (tests/dual_step_ref.py) -- independent of any solve's trajectory.

CPU part: icnn_be_debug_dual_plan -- the launcher's own choice, without the launch -- puts every row of dual_step_ref.CASES on the
instance it names; together the rows reach all 29 instances and every threshold; and the comparison's preconditions hold on
exactly these inputs: the oracle re-run with h and f moved by a relative 1e-15 keeps its active set and finished flag, moves y by
at most 1e-11, stays two updates below its cap, keeps every surviving multiplier above 1e-6 (interior point: every pruned one
below 1e-10) and every pruned cut's reduced gradient above 1e-8.  Two further conditions keep the oracle a function of the
bundle: variant rl's Armijo test (:145-146) must not be decided by the rounding of the objective -- the oracle re-run with its
softplus terms moved by a relative 1e-15 keeps its multipliers to 1e-13 (dual_step_ref.objective_noise_runs; where it does not,
one more Newton update moves them by ~6e-11, inside the 1e-10 gradient tolerance) --, and no multiplier may be within 1e-12 of
zero when the clip at zero or the pivot's 1 - sum (:139, :142) decides it, where the order of a sum makes it exactly 0 (pruned)
or 1e-17 (kept) (dual_step_ref.newton_trace).  All of these are conditions on the inputs, not measurements of the kernel; a
sample that misses one is reseeded (dual_step_ref.RESEED), never exempted.

GPU part, one launch per row: discrete outputs equal to the oracle's round, y at tier A of DESIGN.md section 2, the new slot, the
multipliers within 10 x the oracle's own spread + 1e-12, optimality in longdouble independent of the algorithm, containment of
every write, determinism and the flag twins.

Which rows run where is the plan export's answer and, for the passes gated on the row width, dual_step_ref.sums_path's: variant
dual at n = 1040 with 31 slots stages 22 rows in LDS, so the <float, 32, 8> LDS instance runs at t = 20 and t = 30 is a
dual_step_wide_kernel row; the interior point's one-wave fallback at n = 2560 begins with 29 rows (28 rows: 163 200 bytes fit);
the eight-wave VALU pass and ipm_solve_waves reach 20 cuts only where 8 hv_pitch(20) = 1856 and 8 x 252 = 2016 fit the row, so
their 20 | 21 rows are at n = 2048; the interior point's unrolled passes reach 12 cuts for 103 <= n_pad <= 192 (n = 177) and
ipm_solve_wide_one_fn 20 cuts from n_pad = 252 (n = 255).

The rows at n = 159 are the width of the persistent tile kernel's fixed-shape instances; tests/test_dual_body_probe.py runs the
dual bodies that only that kernel contains on the same states.  Random cuts prune each other, so the `full` rows there hold cuts
of one strongly convex function around the round's solution (dual_step_ref.full_bundle): their bundles leave the round as full
as they entered it (test_full_rows_stay_full).
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dual_step_ref as R

TIER_A = 1e-9                   # same mathematics, float64 summation / elimination order only
H_TOL = 1e-13                   # x (1 + |h|): test_float64_energy_with_float32_gradient_keeps_its_precision
LAM_FLOOR, LAM_FACTOR = 1e-12, 10.0
# Largest norm of the reduced gradient over the surviving cuts that the ORACLE's own multipliers give over the table, evaluated
# in longdouble, per variant (test_oracle_optimality_over_the_table measures them: dual 8.62e-11 at f32_16_dual_n64, rl 9.37e-11
# at f64_small8_rl_n16 -- simplex_newton returns below its 1e-10 tolerance, :122).  The device's multipliers are held to ten
# times that.
ORACLE_WORST_REDUCED_GRAD = {"dual": 8.7e-11, "rl": 9.4e-11}
OPT_BOUND = {v: 10.0 * w for v, w in ORACLE_WORST_REDUCED_GRAD.items()}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(name):
    return R.CASES[R.CASE_IDS.index(name)]


def _c_state(case):
    """struct icnn_be_state of a table row with no buffer but `scratch`, set exactly where BundleState allocates it"""
    from icnn_amd import _lib
    name, plan, cut, slots, n, variant, flags, t, ks = case[:9]
    s = _lib.State()
    s.batch, s.n, s.slots = len(ks), n, slots
    s.iters = R.case_options(case).get("iters", 0)
    s.cut_dtype = _lib.CUT_F64 if cut == np.float64 else _lib.CUT_F32
    s.variant = _lib.VARIANT[variant]
    s.flags = flags
    s.scratch = 1 if int(_lib.load().icnn_be_scratch_bytes(C.byref(s))) else None
    return s


def _k_of(spec):
    return spec[1] if isinstance(spec, tuple) else spec


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_plan_export_is_declared_exported_and_bound():
    from icnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "icnn_be.h")).read()
    assert re.search(r"ICNN_BE_API\s+int\s+icnn_be_debug_dual_plan\s*\(const icnn_be_state \*st, int t, int out\[8\]\)", header)
    assert "icnn_be_debug_dual_plan" in _lib.EXPORTS and hasattr(_lib.load(), "icnn_be_debug_dual_plan")
    assert _lib.load().icnn_be_abi_version() == _lib.ABI_VERSION == 12
    for i, kernel in enumerate(_lib.DUAL_KERNELS):
        assert re.search(r"#define ICNN_BE_DUAL_PLAN_%s %d\b" % (kernel.upper(), i), header)


@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_plan_export_names_the_rows_instance(case):
    from icnn_amd import _lib
    name, plan, cut, slots, n, variant, flags, t, ks = case[:9]
    got = _lib.dual_plan(_c_state(case), t)
    assert got[:6] == plan, (name, got)
    lds, rows = got[6:]
    assert 0 <= lds <= 160 * 1024
    assert max(_k_of(k) for k in ks) <= rows <= min(t + 1, slots)            # no sample of the row overflows the staging
    if plan[4]:                                                             # staged: every row the round allows
        assert rows == min(t + 1, slots)
    if plan[5] == "small":
        assert lds == 0 and n <= 16 and variant == "rl"


def test_plan_export_refuses_what_the_launch_refuses():
    from icnn_amd import _lib
    lib = _lib.load()
    s = _c_state(_case("f32_16_dual_n48"))
    out = (C.c_int * 8)()
    assert lib.icnn_be_debug_dual_plan(C.byref(s), 0, C.byref(out)) == 0
    assert lib.icnn_be_debug_dual_plan(C.byref(s), 14, None) == -1
    assert lib.icnn_be_debug_dual_plan(None, 0, C.byref(out)) == -1
    assert lib.icnn_be_debug_dual_plan(C.byref(s), -1, C.byref(out)) == -1
    assert lib.icnn_be_debug_dual_plan(C.byref(s), 15, C.byref(out)) == -1          # t beyond the last iteration
    s.batch = 0
    assert lib.icnn_be_debug_dual_plan(C.byref(s), 0, C.byref(out)) == -1           # nothing is launched
    s.batch, s.slots = 4, 40
    assert lib.icnn_be_debug_dual_plan(C.byref(s), 0, C.byref(out)) == -2           # ICNN_BE_MAX_SLOTS
    # wide rows without a staging area keep the LDS instance at its capacity (samples beyond it overflow)
    s = _c_state(_case("f32_wide_n1536"))
    s.scratch = None
    got = _lib.dual_plan(s, 23)
    assert got[:6] == ("float", 32, 8, "dual", False, "body") and got[7] == lib.icnn_be_bundle_capacity(1536, 24, 0, 0) < 24


# the 29 instances of choose_dual_step / launch_dual_step_small (be_dual.hip, be_dual_small.hip)
LDS_INSTANCES = ({("float", kt, w, v, False, "body") for kt in (16, 32) for w, v in ((1, "dual"), (8, "dual"), (1, "pdipm"),
                                                                                      (8, "pdipm"), (1, "rl"))}
                 | {("double", kt, 1, v, False, "body") for kt in (16, 32) for v in ("dual", "pdipm", "rl")})
STAGED_INSTANCES = {("double", 32, 1, "dual", True, "body"), ("double", 32, 1, "pdipm", True, "body"),
                    ("float", 32, 1, "dual", True, "body"), ("float", 32, 8, "dual", True, "body"),
                    ("float", 32, 1, "pdipm", True, "body"), ("float", 32, 8, "pdipm", True, "body"),
                    ("float", 32, 8, "dual", True, "wide")}
SMALL_INSTANCES = {(ct, ks, 4, "rl", False, "small") for ct in ("float", "double") for ks in (5, 8, 16)}

# k on both sides of every threshold that depends on k alone, per family of rows (select: which rows belong to the family)
NEWTON_K = {4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 16, 17, 20, 21, 24, 25}      # newton_step / inertia_not_above: 4 6 8 10 12 16 20 24
FAMILIES = {
    # newton_step<KT>, inertia_not_above<KT>; the 8 x 8 MFMA tiling while k + 1 <= 8 (7 | 8)
    "one wave, float32, LDS, dual": (lambda p, n, v, fl: p[:5] == ("float", p[1], 1, "dual", False) and n >= 48 and n <= 192,
                                     NEWTON_K | {1, 2, 31}),
    "one wave, MFMA sweep only": (lambda p, n, v, fl: bool(fl & R.FLAG_MFMA_CONTRACTION), {7, 8, 9, 12, 13}),
    "float64 cuts, dual": (lambda p, n, v, fl: p[0] == "double" and v == "dual", NEWTON_K | {1, 2, 31}),
    "float64 cuts, rl": (lambda p, n, v, fl: p[0] == "double" and v == "rl" and p[5] == "body", NEWTON_K | {1, 2, 31}),
    "float32, rl": (lambda p, n, v, fl: p[0] == "float" and v == "rl" and p[5] == "body", NEWTON_K | {1, 2, 31}),
    "wide kernel, rows mirrored (WIDE_LR = 12) and not": (lambda p, n, v, fl: p[5] == "wide", {2, 12, 13, 20, 21, 24, 31}),
    "pdipm, float64 cuts": (lambda p, n, v, fl: v == "pdipm" and p[0] == "double", {1, 2, 12, 13, 20, 21, 31}),
    "pdipm, staged": (lambda p, n, v, fl: v == "pdipm" and p[4], {1, 2, 12, 13, 20, 21, 31}),
    "small kernel": (lambda p, n, v, fl: p[5] == "small", {1, 2, 4, 5, 6, 7, 8, 9, 12, 15}),
}
# The passes that are gated on the row width as well (dual_step_ref.sums_path restates the kernels' conditions): every instance
# size each routine is dispatched to, per wave count, and -- in ONE row, so at one width -- its last bundle size next to the
# first one that falls back to the MFMA sweep.
ROUTINE_INSTANCES = {
    ("valu", 1): {2, 4, 5, 6, 7, 8},                                  # hv_column_pass_k, one wave: up to HV_K1MAX = 8
    ("valu", 8): {2, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20},          # eight waves: up to HV_KMAX = 20, needs 8 hv_pitch(k) <= n_pad
    ("ipm_unrolled", 1): {2, 5, 7, 10, 12},                           # IPM_K_SWITCH: up to IPM_KMAX = 12, needs ipm_nv(K) <= n_pad <= 192
    ("ipm_weighted", 1): {6, 8},                                      # hv_weighted_pass where the unrolled pass does not fit the row
    ("ipm_wide_one", 1): {2, 12, 14, 18, 20},                         # IPM_K_SWITCH_WAVES on one wave, n_pad > 192
    ("ipm_waves", 8): {2, 12, 14, 20},                                # ... on eight: needs 8 (ipm_nv(K) + 3 & ~3) <= n_pad
}
ROUTINE_EDGES = {("valu", 1): 8, ("valu", 8): 20, ("ipm_unrolled", 1): 12, ("ipm_wide_one", 1): 20, ("ipm_waves", 8): 20}


def _row_paths(case):
    """[(k, routine, instance size)] of the live samples of a row, on the rows the plan export stages"""
    from icnn_amd import _lib
    rows = _lib.dual_plan(_c_state(case), case[7])[7]
    return [(_k_of(k),) + R.sums_path(case[1], case[4], _k_of(k), case[6], rows)
            for k, kind in zip(case[8], R.case_state(case[0]).kind) if kind == "live"]


def test_width_gated_passes_run_at_every_instance_and_on_both_sides_of_their_last():
    assert (R.hv_pitch(20), R.hv_pitch(14), R.ipm_nv(12), R.ipm_nv(20)) == (232, 120, 103, 251)
    seen, edges = {}, set()
    for c in R.CASES:
        paths = _row_paths(c)
        for k, routine, K in paths:
            seen.setdefault((routine, c[1][2]), set()).add(K)
        for key, last in ROUTINE_EDGES.items():
            if key[1] == c[1][2] and (last, key[0]) in {(k, r) for k, r, _ in paths} and (last + 1, "mfma") in {(k, r) for k, r, _ in paths}:
                edges.add(key)
    for key, need in ROUTINE_INSTANCES.items():
        assert seen.get(key, set()) & need == need, (key, sorted(need - seen.get(key, set())))
    assert edges == set(ROUTINE_EDGES)
    # and the widths that do NOT reach the last instance say so: at n = 1040 the eight-wave passes end at 14 and 12 cuts (the
    # interior point then runs the one-wave solve on wave 0, which at this width is ipm_solve_wide_one_fn)
    assert R.sums_path(("float", 32, 8, "dual", False, "body"), 1040, 15, 0, 21) == ("mfma", 0)
    assert R.sums_path(("float", 32, 8, "pdipm", False, "body"), 1040, 13, 0, 14) == ("ipm_wide_one", 14)
    assert R.sums_path(("float", 16, 1, "pdipm", False, "body"), 48, 8, 0, 15) == ("ipm_weighted", 8)


WIDTHS_ONE_WAVE = {1, 15, 16, 17, 63, 64, 65, 177, 192, 193, 255, 256, 257, 300, 1023}   # n_pad 192 | 208, 256 | 272, one wave < 1024
WIDTHS_EIGHT_WAVES = {1024, 1040}                                                        # ragged last column chunk at 1040


def test_table_reaches_every_instance_every_threshold_and_every_width_edge():
    plans = {c[1] for c in R.CASES}
    assert {p for p in plans if p[5] == "small"} == SMALL_INSTANCES
    assert {p for p in plans if p[4]} == STAGED_INSTANCES
    assert {p for p in plans if not p[4] and p[5] == "body"} == LDS_INSTANCES
    assert len(plans) == 29
    for family, (select, need) in FAMILIES.items():
        seen = set()
        for c in R.CASES:
            if select(c[1], c[4], c[5], c[6]):
                seen.update(_k_of(k) for k, kind in zip(c[8], R.case_state(c[0]).kind) if kind == "live")
        assert seen & need == need, (family, sorted(need - seen))
    one_wave = {c[4] for c in R.CASES if c[1][:6] == ("float", 16, 1, "dual", False, "body") and c[3] == 10}
    assert one_wave & WIDTHS_ONE_WAVE == WIDTHS_ONE_WAVE
    assert {c[4] for c in R.CASES if c[1][2] == 8 and c[3] == 15 and c[5] == "dual"} == WIDTHS_EIGHT_WAVES
    # at least three rows run at a smaller t (rows_cap < slots moves the carve-up), one recycles slots, one takes float64 energies
    assert sum(1 for c in R.CASES if c[7] < c[3] - 1 and not R.case_options(c).get("iters")) >= 3
    assert any(R.case_options(c).get("iters", 0) > c[3] for c in R.CASES)
    assert any(c[6] & R.FLAG_F64_ENERGY for c in R.CASES)
    # the special samples are in dual and pdipm rows of both cut dtypes
    for variant in ("dual", "pdipm"):
        for cut in (np.float32, np.float64):
            kinds = set()
            for c in R.CASES:
                if c[5] == variant and c[2] == cut:
                    kinds.update(R.case_state(c[0]).kind)
            assert kinds == {"live", "fin", "dup", "zero"}, (variant, cut)
    for c in R.CASES:
        if c[5] == "rl":
            assert set(R.case_state(c[0]).kind) == {"live"}


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_state_is_written_as_described(name):
    """NaN wherever the kernel must not read, slots in random order, the specials as announced, the oracle's round as expected
    of them."""
    s = R.case_state(name)
    ref, _ = R.case_reference(name)
    shuffled = False
    for u in range(s.B):
        cnt = s.count[u]
        own = s.active[u, :cnt]
        off = np.setdiff1d(np.arange(s.slots), own)
        assert len(set(own.tolist())) == cnt
        assert np.isnan(s.G[u, off]).all() and np.isnan(s.ys[u, off]).all() and np.isnan(s.h[u, off]).all()
        assert np.isfinite(s.G[u, own]).all() and np.isfinite(s.h[u, own]).all() and np.isnan(s.lam[u]).all()
        assert (s.active[u, cnt:] == off[-1]).all()
        shuffled |= cnt > 1 and not np.array_equal(own, np.sort(own))
        slot = R.new_slot(s, u)
        assert slot not in own and (slot == s.t or s.iters > s.slots)
        if s.kind[u] == "fin":
            assert ref["finished"][u] == 1 and ref["n_iters"][u] == s.n_iters[u] and np.array_equal(ref["y"][u], s.y[u])
        elif s.kind[u] in ("dup", "zero"):
            assert ref["finished"][u] == 1 and ref["n_iters"][u] == s.t - 1 and ref["count"][u] == cnt
            assert np.array_equal(ref["y"][u], s.y[u]) and ref["active"][u] == own.tolist()
            if s.kind[u] == "dup":
                assert any(np.array_equal(s.g[u], s.G[u, sl]) for sl in own)
            else:
                assert cnt == 0 and not s.g[u].any()
        elif s.n >= cnt + 1:
            assert ref["lam_full"][u] is not None, "a live sample with k <= n must reach the inner solve"
    assert shuffled or max(s.count) <= 1
    if s.iters > s.slots:
        assert any(R.new_slot(s, u) != s.t for u in range(s.B)) and s.t >= s.slots


@pytest.mark.parametrize("name", R.CASE_IDS)
def test_preconditions_of_the_comparison(name):
    bad, lam_spread, y_spread = R.precondition_failures(name)
    ref, _ = R.case_reference(name)
    print("%s: oracle under 1e-15: lam spread %.2e, y spread %.2e; updates <= %s; bundle sizes after pruning %s"
          % (name, lam_spread.max(), y_spread.max(), max([v for v in ref["newton"] if v is not None] or [0]), ref["count"].tolist()))
    assert not bad, bad


FULL_ROWS = [c[0] for c in R.CASES if "full" in R.case_options(c)]


@pytest.mark.parametrize("name", FULL_ROWS)
def test_full_rows_stay_full(name):
    """What the `full` rows are for, as a condition on the inputs: up to the cap of eight (HV_K1MAX, the round class of the tile
    kernel) every bundle size the row lists is the size of some sample's bundle AFTER the oracle's round -- that many multipliers
    stay positive --, and the 31-slot row keeps 16 and more cuts somewhere.  Reached through RESEED, never by exempting a
    sample."""
    case = _case(name)
    s = R.case_state(name)
    ref, _ = R.case_reference(name)
    assert set(s.kind) == {"live"} and len(FULL_ROWS) == 7
    after = set(ref["count"].tolist())
    for k in sorted({_k_of(k) for k in case[8]}):
        if k <= R.HV_K1MAX:
            assert k in after, (name, k, ref["count"].tolist())
    for u in range(s.B):                    # no rank-test exit, no pruned-to-one sample: every round here is a Newton solve
        assert ref["lam_full"][u] is not None and ref["newton"][u] >= 2 and ref["count"][u] >= 2
    if case[3] > 15:
        assert max(after) >= 16


def _oracle_optimality(name):
    s = R.case_state(name)
    ref, _ = R.case_reference(name)
    worst = 0.0
    for u in range(s.B):
        if s.variant == "pdipm" or ref["lam_full"][u] is None or len(ref["lam_full"][u]) < 2:
            continue
        norm, pruned = R.reduced_gradient(*R.bundle_of(s, ref, u), ref["lam_full"][u])
        assert (pruned > 0).all()
        worst = max(worst, norm)
    return worst


def test_oracle_optimality_over_the_table():
    for variant, bound in ORACLE_WORST_REDUCED_GRAD.items():
        worst = {c[0]: _oracle_optimality(c[0]) for c in R.CASES if c[5] == variant}
        top = max(worst, key=worst.get)
        print("%s: largest reduced-gradient norm of the oracle's own multipliers %.3e (%s)" % (variant, worst[top], top))
        assert 0.9 * bound <= worst[top] <= bound                  # the figure next to the bound is the measured one


# ---- GPU ------------------------------------------------------------------------------------------------------------------
STATE_TENSORS = ("y", "G", "h", "ys", "lam", "active", "fvals", "pending", "park") + R.CONTROL


def _snapshot(st):
    return {name: getattr(st, name).detach().cpu().numpy().copy() for name in STATE_TENSORS}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _launch(s, flags, plan=None, step=None):
    """(state before, state after) of one icnn_be_dual_step launch on the row's state; step(st, t, f, g): another entry's launch
    in its place (tests/test_dual_body_probe.py)"""
    import torch
    st, f, g = s.to_device(flags)
    if plan is not None:                 # the state that is launched gets the instance the row names
        from icnn_amd import _lib
        assert _lib.dual_plan(st.c_state, s.t)[:6] == plan
    before = _snapshot(st)
    if step is not None:
        step(st, s.t, f, g)
    else:
        st.step(s.t, f, g)
    torch.cuda.synchronize()
    return before, _snapshot(st)


def _assert_containment(s, ref, before, after):
    """Raw bits of every array before and after.  May differ: the new slot of G / h / ys / fvals, the sample's y row, lam and
    active up to the new count, the control words.  Further writes of the kernel:
      pending[t]   be_dual_dev.h dual_step_body `if (more) es.pending[round] = 1` (be_dual_small_dev.h: `if (more)
                   st.pending[round] = 1`): a sample with another iteration ahead says so
      skip_fg      a control word here (finished or last iteration: 1)
      park         written only when a budgeted launch parks a sample (`if (parked)`): icnn_be_dual_step has no budget, so not a bit
      scratch      the staging area itself (`As = GLB ? st.scratch + ...`): not state, not compared
    """
    B, T = s.B, s.slots
    assert _same_bits(before["park"], after["park"])
    full = s.iters if s.iters else T
    more = any(not s.finished[u] and not ref["finished"][u] and s.t + 1 < full for u in range(B))
    want_pending = before["pending"].copy()
    if more:
        want_pending[s.t] = 1
    assert np.array_equal(after["pending"], want_pending)
    for name in R.CONTROL:
        assert _same_bits(before[name][B:], after[name][B:])
    for u in range(B):
        if s.kind[u] == "fin":                                   # the finished sample is untouched everywhere
            for name in ("y", "G", "h", "ys", "lam", "active", "fvals"):
                assert _same_bits(before[name][u], after[name][u]), (u, name)
            for name in R.CONTROL:
                assert before[name][u] == after[name][u], (u, name)
            continue
        slot = ref["slot"][u]
        others = np.setdiff1d(np.arange(T), [slot])
        for name in ("G", "h", "ys", "fvals"):
            assert _same_bits(before[name][u][others], after[name][u][others]), (u, name)
        inactive = np.setdiff1d(others, s.active[u, :s.count[u]])
        for name in ("G", "h", "ys", "fvals"):                  # the NaNs of inactive slots are still NaN
            assert np.isnan(after[name][u][inactive]).all()
        cnt = int(after["count"][u])
        assert _same_bits(before["lam"][u, cnt:], after["lam"][u, cnt:]) and np.isnan(after["lam"][u, cnt:]).all(), u
        assert _same_bits(before["active"][u, cnt:], after["active"][u, cnt:]), u
        if ref["lam_full"][u] is None:                          # ended by the rank test: bundle and y as they were
            for name in ("y", "lam", "active"):
                assert _same_bits(before[name][u], after[name][u]), (u, name)
        else:
            assert np.isfinite(after["lam"][u, :cnt]).all() and np.isfinite(after["y"][u]).all()
        assert np.isfinite(after["h"][u, slot]) and np.isfinite(after["G"][u, slot]).all()


def _assert_round(s, ref, lam_spread, before, after, label):
    B, T = s.B, s.slots
    full = s.iters if s.iters else T
    worst = dict(y=0.0, lam=0.0, opt=0.0, h=0.0)
    assert (after["status"][:B] == 0).all(), after["status"][:B]
    assert np.array_equal(after["count"][:B], ref["count"])
    assert np.array_equal(after["finished"][:B], ref["finished"])
    assert np.array_equal(after["n_iters"][:B], ref["n_iters"])
    for u in range(B):
        if s.kind[u] == "fin":
            continue
        cnt = int(ref["count"][u])
        assert after["active"][u, :cnt].tolist() == ref["active"][u], u
        assert after["phase"][u] == 0
        slot = ref["slot"][u]
        assert np.array_equal(after["G"][u, slot], ref["G_new"][u]) and np.array_equal(after["ys"][u, slot], ref["ys_new"][u])
        assert after["fvals"][u, slot] == np.float64(s.f[u])
        dh = abs(after["h"][u, slot] - ref["h_new"][u]) / (1.0 + abs(ref["h_new"][u]))
        worst["h"] = max(worst["h"], dh)
        assert dh <= H_TOL, (u, dh)
        if ref["lam_full"][u] is None:                          # rank test: no step was taken
            assert after["t_next"][u] == s.t and after["skip_fg"][u] == 1
            continue
        live_on = not ref["finished"][u] and s.t + 1 < full
        assert after["t_next"][u] == s.t + 1 and after["skip_fg"][u] == (0 if live_on else 1)
        dy = float(np.max(np.abs(after["y"][u] - ref["y"][u])))
        worst["y"] = max(worst["y"], dy)
        assert dy <= TIER_A, (u, dy)
        dlam = float(np.max(np.abs(after["lam"][u, :cnt] - ref["lam"][u])))
        worst["lam"] = max(worst["lam"], dlam)
        assert dlam <= LAM_FACTOR * lam_spread[u] + LAM_FLOOR, (u, dlam, lam_spread[u])
        if s.variant != "pdipm":                                # on the simplex by construction (:142); pdipm_pc's z is not
            assert abs(after["lam"][u, :cnt].sum() - 1.0) <= 1e-12
        if s.variant != "pdipm" and len(ref["slots_full"][u]) > 1:
            # optimality, whatever the algorithm: at the DEVICE's multipliers, zeros where it pruned
            lam_dev = np.zeros(len(ref["slots_full"][u]))
            for sl, v in zip(after["active"][u, :cnt], after["lam"][u, :cnt]):
                lam_dev[ref["slots_full"][u].index(int(sl))] = v
            norm, pruned = R.reduced_gradient(*R.bundle_of(s, ref, u), lam_dev)
            worst["opt"] = max(worst["opt"], norm)
            assert norm <= OPT_BOUND[s.variant], (u, norm)
            assert (pruned > 0).all(), (u, pruned)               # the sign the bound rule asks of a cut at zero (:119)
    print("%s: device vs oracle y %.3e lam %.3e h %.3e; reduced gradient at the device's multipliers %.3e"
          % (label, worst["y"], worst["lam"], worst["h"], worst["opt"]))
    return worst


def _assert_twins(s, a, b, bitwise, label, loose=()):
    """two launches from the same state: the same bits, or (MFMA contraction against the VALU pass; the samples `loose`) the
    same discrete state with y inside the y bound"""
    for name in STATE_TENSORS:
        if name in ("pending", "park"):
            assert _same_bits(a[name], b[name]), (label, name)
            continue
        for u in range(s.B):
            if bitwise and u not in loose:
                assert _same_bits(a[name][u], b[name][u]), (label, name, u)
            elif name in ("y", "lam"):
                ok = np.isnan(a[name][u]) & np.isnan(b[name][u])
                assert np.all(ok | (np.abs(a[name][u] - b[name][u]) <= TIER_A)), (label, name, u)
            elif name == "h":
                ok = np.isnan(a[name][u]) & np.isnan(b[name][u])
                assert np.all(ok | (np.abs(a[name][u] - b[name][u]) <= H_TOL * (1 + np.abs(a[name][u])))), (label, name, u)
            elif name != "newton_iters":
                assert _same_bits(a[name][u], b[name][u]), (label, name, u)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=R.CASE_IDS)
def test_dual_step_row(case):
    from icnn_amd import _lib
    name, plan, cut, slots, n, variant, flags, t, ks = case[:9]
    opt = R.case_options(case)
    s = R.case_state(name)
    ref, _ = R.case_reference(name)
    _, lam_spread, _ = R.precondition_failures(opt.get("twin_of", name))
    before, after = _launch(s, flags, plan)
    label = "%s <%s,%d,%d waves,%s%s,%s>" % (name, plan[0], plan[1], plan[2], plan[3], ",staged" if plan[4] else "", plan[5])
    for nm in ("y", "G", "h", "ys", "lam", "active", "fvals") + R.CONTROL:      # the device holds the state as written
        host = getattr(s, nm)
        assert _same_bits(before[nm][:s.B], host), nm
    _assert_containment(s, ref, before, after)
    _assert_round(s, ref, lam_spread, before, after, label)
    # determinism: a second launch from the same state gives the same bits
    _, again = _launch(s, flags, plan)
    _assert_twins(s, after, again, True, label + " again")
    if "twin" in opt:                      # the same state under another flag: another kernel, the same bits
        assert _lib.dual_plan(_flagged(case, flags | opt["twin"]), t)[:6] != plan
        _, twin = _launch(s, flags | opt["twin"])
        _assert_twins(s, after, twin, True, label + " flag twin")
    if "twin_of" in opt:
        base = _case(opt["twin_of"])
        _, twin = _launch(s, base[6], base[1])
        # bit-identical wherever both launches form their sums by the same routine.  The staged bundle has no instance of the
        # interior point's unrolled / weighted passes (include/icnn_be.h ICNN_BE_FLAG_GLOBAL_BUNDLE, be_ipm_dev.h ipm_solve) and
        # ICNN_BE_FLAG_MFMA_CONTRACTION takes the fused VALU pass away: those samples agree to the y bound
        rows_a, rows_b = _lib.dual_plan(_c_state(case), t)[7], _lib.dual_plan(_c_state(base), t)[7]
        loose = tuple(u for u in range(s.B)
                      if R.sums_path(plan, n, int(s.count[u]) + 1, flags, rows_a)[0] != R.sums_path(base[1], n, int(s.count[u]) + 1, base[6], rows_b)[0])
        if variant == "dual" and not flags & R.FLAG_MFMA_CONTRACTION:
            assert not loose
        _assert_twins(s, after, twin, True, label + " vs " + base[0], loose)


def _flagged(case, flags):
    s = _c_state(case)
    s.flags = flags
    return s
