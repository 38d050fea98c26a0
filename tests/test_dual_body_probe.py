"""The dual bodies that only the persistent tile kernel contains -- dual_step_body<..., BibtexShape> of its 16- and 32-slot
Bibsonomy instances and the body capped at eight cuts that the 16-slot instance runs in rounds 0..7 (be_fused.hip) -- one round at
a time through icnn_be_debug_dual_step_body, on the hand-written states of tests/dual_step_ref.py at n = 159.

The identity tests of these bodies (tests/test_shape_instance.py, tests/test_round_classes.py) compare them with their siblings
on the trajectories of a solve, where bundles rarely fill their cap and a mistake in text that both twins share (be_dual_dev.h,
be_dual_valu_dev.h, be_dual_dpp_rows.h) changes both alike.  Here a probe launch is judged exactly as a launch of
icnn_be_dual_step is in tests/test_dual_step_shapes.py -- against the float64 oracle's round, optimality in longdouble,
containment of every write -- on bundles of exactly 2..8 cuts that stay full, on duplicate cuts that the rank test must end,
with rows_cap from the round (the ungrouped loop) and from each sample's own count (the grouped loop).  Against the public
launch of the same state it must agree bit for bit, newton_iters and status included: include/icnn_be.h promises the same
operations in the same order, and dual_step_ref.sums_path says for every sample that both sides form their sums by the same
routine.
"""
import ctypes as C

import numpy as np
import pytest

import dual_step_ref as R
import test_dual_step_shapes as T

N_BIBTEX = 159
ROUND_CLASS_CAP = R.HV_K1MAX                      # be_fused.hip
BODY = {1: "BibtexShape, KT 16", 2: "BibtexShape, KT 16, capped at %d cuts" % ROUND_CLASS_CAP, 3: "BibtexShape, KT 32"}
ROWS_MODE_1_TOO = ("f32_16_dual_n159_t7", "f32_16_dual_n159_full_t9")      # 16-slot rows that also run with rows_mode 1


def _combos(case):
    """every legal (which, rows_mode) of a row"""
    name, slots, t = case[0], case[3], case[7]
    if slots > 15:
        return [(3, 0), (3, 1)]
    combos = [(1, 0), (2, 0)] if t < ROUND_CLASS_CAP else [(1, 0)]
    return combos + ([(1, 1)] if name in ROWS_MODE_1_TOO else [])


PROBE_ROWS = [c for c in R.CASES if c[4] == N_BIBTEX]
PROBE_CASES = [(c[0], which, mode) for c in PROBE_ROWS for which, mode in _combos(c)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_probe_cases_cover_every_body_and_both_row_rules():
    assert len(PROBE_ROWS) == 14 and all(c[2] == np.float32 and c[5] == "dual" and c[6] == 0 for c in PROBE_ROWS)
    seen = {}
    for name, which, mode in PROBE_CASES:
        case = T._case(name)
        live = [T._k_of(k) for k, kind in zip(case[8], R.case_state(name).kind) if kind == "live"]
        seen.setdefault((which, mode), set()).update(live)
        seen.setdefault(("kinds", which, mode), set()).update(R.case_state(name).kind)
    # both sides of every branch on k: hv_column_pass_upto / newton_step_dpp_inl<4|6|8> / inertia_not_above_dpp_inl<4|6|8> of the
    # capped body, and those of the full body up to the VALU gate and beyond it
    assert seen[(2, 0)] >= set(range(1, ROUND_CLASS_CAP + 1))
    assert seen[(1, 0)] >= set(range(1, 11)) and seen[(1, 1)] >= set(range(1, 11))
    assert seen[(3, 0)] == seen[(3, 1)] >= {1, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 31}
    for which, mode in ((1, 0), (2, 0), (3, 0), (3, 1), (1, 1)):
        assert seen[("kinds", which, mode)] == {"live", "fin", "dup", "zero"}
    # rows_cap held by the slots instead of t + 1, for both 16-slot bodies
    assert {(w, m) for n, w, m in PROBE_CASES if n == "f32_16_dual_n159_s5_t4"} == {(1, 0), (2, 0)}


def _c_state(case, t=None, flags=None, **kw):
    """struct icnn_be_state of a row with made-up buffer addresses (no refusing path dereferences one) and batch 0, where an
    accepted call launches nothing"""
    from icnn_amd import _lib
    s = T._c_state(case)
    for i, (name, typ) in enumerate(_lib.State._fields_):
        if typ is C.c_void_p and name != "scratch":
            setattr(s, name, 0x100000 + 0x100 * i)
    s.batch = 0
    if flags is not None:
        s.flags = flags
    for name, v in kw.items():
        setattr(s, name, v)
    return s


def test_probe_entry_is_declared_exported_and_bound():
    import os
    import re
    from icnn_amd import _lib
    header = open(os.path.join(T.ROOT, "include", "icnn_be.h")).read()
    assert re.search(r"ICNN_BE_API\s+int\s+icnn_be_debug_dual_step_body\s*\(const icnn_be_state \*st, int t, const void \*f, "
                     r"const void \*g, int which,\s+int rows_mode, void \*stream\)", header)
    assert "icnn_be_debug_dual_step_body" in _lib.EXPORTS and hasattr(_lib.load(), "icnn_be_debug_dual_step_body")
    assert _lib.load().icnn_be_abi_version() == _lib.ABI_VERSION == 12


@pytest.mark.parametrize("name,which,mode", PROBE_CASES, ids=["%s-body%d-rows%d" % c for c in PROBE_CASES])
def test_probe_accepts_every_case_it_is_run_on(name, which, mode):
    """with an empty batch an accepted call returns 0 and launches nothing: every case of the GPU test is a legal one"""
    from icnn_amd import _lib
    case = T._case(name)
    assert _lib.load().icnn_be_debug_dual_step_body(C.byref(_c_state(case)), case[7], 0x1000, 0x2000, which, mode, None) == 0


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _rows_of(s, case, mode):
    """rows_cap of every sample: the plan's rows (rows_mode 0: min(t + 1, slots), what the public launch stages), or count + 1"""
    from icnn_amd import _lib
    if mode == 0:
        rows = _lib.dual_plan(T._c_state(case), s.t)[7]
        assert rows == min(s.t + 1, s.slots)
        return [rows] * s.B
    return [min(int(s.count[u]) + 1, s.slots) for u in range(s.B)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,which,mode", PROBE_CASES, ids=["%s-body%d-rows%d" % c for c in PROBE_CASES])
def test_dual_body_row(name, which, mode):
    case = T._case(name)
    plan, n, flags, t = case[1], case[4], case[6], case[7]
    s = R.case_state(name)
    ref, _ = R.case_reference(name)
    _, lam_spread, _ = R.precondition_failures(name)
    label = "%s <%s> rows_mode %d" % (name, BODY[which], mode)

    def step(st, t_, f, g):
        st.step_body(t_, f, g, which, mode)

    before, after = T._launch(s, flags, plan, step)
    # a probe launch is judged exactly as a public launch is
    T._assert_containment(s, ref, before, after)
    T._assert_round(s, ref, lam_spread, before, after, label)
    # the public launch of the same state: the same bits, wherever both form their sums by the same routine -- which is
    # everywhere, and the fused VALU pass for 2..8 cuts
    rows_public, rows_probe = _rows_of(s, case, 0), _rows_of(s, case, mode)
    for u in range(s.B):
        k = int(s.count[u]) + 1
        ours, theirs = R.sums_path(plan, n, k, flags, rows_probe[u]), R.sums_path(plan, n, k, flags, rows_public[u])
        assert ours == theirs, (u, k, ours, theirs)
        assert (ours[0] == "valu") == (2 <= k <= R.HV_K1MAX), (u, k, ours)
    _, public = T._launch(s, flags, plan)
    T._assert_twins(s, after, public, True, label + " vs icnn_be_dual_step")
    # determinism: a second probe launch gives the same bits
    _, again = T._launch(s, flags, plan, step)
    T._assert_twins(s, after, again, True, label + " again")


@pytest.mark.gpu
def test_capped_body_is_refused_past_its_rounds_on_a_device_state():
    """which 2 at t = 8 and under ICNN_BE_FLAG_MFMA_CONTRACTION: refused with real buffers too, and nothing is written"""
    import torch
    for name, t, flags in (("f32_16_dual_n159_t9", ROUND_CLASS_CAP, 0), ("f32_16_dual_n159_t7", 7, R.FLAG_MFMA_CONTRACTION)):
        st, f, g = R.case_state(name).to_device(flags)
        before = T._snapshot(st)
        args = (C.byref(st.c_state), t, f.data_ptr(), g.data_ptr())
        assert st.lib.icnn_be_debug_dual_step_body(*args, 2, 0, st.stream()) == -1
        assert st.lib.icnn_be_debug_dual_step_body(*args, 2, 1, st.stream()) == -1
        torch.cuda.synchronize()
        after = T._snapshot(st)
        for nm in T.STATE_TENSORS:
            assert T._same_bits(before[nm], after[nm]), (name, nm)
