"""The fused FC solves (be_fused.hip), the context producer (be_context.hip) and gd.solve (be_gd.hip) at architectures
other than the two shipped nets.  Every LDS layout of the persistent kernels is a function of the architecture and the
bundle size (fused_rows_layout, fused_tile_layout); Bibtex (n = 159) and HalfCheetah (n = 6) reach one point of it each.
The specs below reach the others: one and eight layers, label counts on every branch of NumPy's pairwise sum (n < 8, 8,
9, > 256), both sides of the narrow-row limit (16 / 17), staged bundles smaller and larger than phase A's buffers, the
grouped dual phase at fewer than 16 slots, and both narrow-row instances no other test launches
(fused_rows_solve_kernel<true, 16, 8> and <true, 16, 16>).

Every spec of the table was accepted by the library as written; none had to be replaced.

  1. CPU: every solve case names the icnn_be_debug_solve_plan result it is meant to run at 256 CUs, and the tile cases the
     layout branch (grouped or not, constant rows behind the bundles or behind phase A) by a restatement of the layout rule.
  2. GPU: the planned path against ICNN_BE_FLAG_TWO_KERNELS, every output bit for bit.
  3. GPU: against the float64 solver over the kernel-order float32 PICNN (oracle.solve_batch around make_fg_chain), on
     seeds screened on the CPU so that the oracle itself is clean and never runs a Newton solve into its cap.
  4. GPU: model.context against the float64 statement of oracle/picnn_oracle.py (and bn_ref.py in moving mode).
  5. GPU: gd.solve on gd_rows_kernel and gd_fc_kernel bit for bit against gd_ref.unroll_f32.

One-dimensional y (L1_n1): the rank test of variant dual ends every sample at its second cut (two cuts in one dimension
are never independent), so no Newton update is ever taken there; that case asserts exactly this instead of "some sample
took more than one update".  The interior-point variant keeps no Newton counter either (icnn_be_state.newton_iters is a
diagnostic of the projected Newton solves and stays 0): its cases assert instead that some sample ends with more than one
cut, i.e. that the interior point solved subproblems of several cuts."""
import ctypes as C
import functools
from unittest import mock

import numpy as np
import pytest
import torch

import bn_ref
import gd_ref
from gpu_util import compare_with_oracle, result_to_host
from icnn_amd import _lib, picnn
from oracle import bundle_entropy_oracle as oracle
from oracle import picnn_oracle
from test_architectures import CHAIN2, DEEP, _perturbed
from test_gpu_parity import _all_outputs, _planned
from test_solve_plan import CUS, plan

FC = picnn.FCSpec
SPECS = {
    "L1_n1": FC(12, 1, (16,), batchnorm=False),                                      # one hidden layer, n = 1
    "L1_n9": FC(12, 9, (40,), batchnorm=True),                                       # pairwise plan with a tail, tiny phase A
    "n8_box": FC(12, 8, (24, 16), alpha=0.01, batchnorm=False, action_box=True),     # narrow rows, eight accumulators, no tail
    "n16_box": FC(12, 16, (24, 16), alpha=0.01, batchnorm=False, action_box=True),   # last narrow width
    "n17_box": FC(12, 17, (24, 16), alpha=0.01, batchnorm=False, action_box=True),   # first width on the wave-per-sample path
    "n20_deep4": FC(12, 20, (70, 33, 18, 50), alpha=0.01, batchnorm=True),           # odd k-block counts
    "n33": FC(12, 33, (240, 100), batchnorm=True),                                   # phase A larger than the bundles
    "n70": FC(12, 70, (72, 40), batchnorm=True),                                     # bundles larger than phase A
    "n270": FC(12, 270, (300, 280), batchnorm=False),                                # n > 256: pairwise split
    "deep8": DEEP,                                                                   # ICNN_BE_MAX_LAYERS
}
PERS, SLICE, TWO, WPS = _lib.FLAG_PERSISTENT, _lib.FLAG_TIME_SLICE, _lib.FLAG_TWO_KERNELS, _lib.FLAG_WAVE_PER_SAMPLE
OUTPUTS = ["y", "lam", "active", "count", "n_iters", "newton_iters", "G", "h", "ys", "finished", "status"]   # _all_outputs


# ------------------------------------------------------------------------------------------------ the layout rule


def _a16(v):
    return (v + 15) & ~15


def _pw_leaves(n):
    """leaves of NumPy's pairwise sum of n elements (pw_build, be_common.h)"""
    if n <= 128:
        return 1
    n2 = n // 2
    n2 -= n2 % 8
    return _pw_leaves(n2) + _pw_leaves(n - n2)


def _row_pitch(n_pad):
    while n_pad % 32 != 2:
        n_pad += 1
    return n_pad


def _carve(KT, rows, n, rl, ipm, own_const_rows=False):
    """bytes of one sample's staging region: float32 cuts on one wave (carve, be_dual_cut.h)"""
    n_pad = _a16(n)
    o = _a16((rows + (2 if own_const_rows else 0)) * _row_pitch(n_pad) * 4) + 2 * _a16(n_pad * 8)
    o += _a16(n_pad * 8) * ((1 if rl or ipm else 0) + (2 if ipm else 0))
    o += _a16(max(rows * ((rows + 1) | 1) * 8, (KT * _pw_leaves(n) + 2 * KT) * 8))
    return o + _a16(KT * 4)


def _lds_pitch(width):
    p = (_a16(width) // 16 + 4) // 5 * 5 * 16
    while p & 63 != 8:
        p += 4
    return p


def tile_layout(spec, slots, variant):
    """The layout rule of fused_tile_layout (be_fused.hip), restated: phase B stages sixteen bundles from offset 0 over
    phase A's buffers and the constant rows sit behind whichever is larger; the dual phase is GROUPED when bundles and
    constant rows exceed 160 KB, or at more than 15 slots.  Returns (grouped, what the constant rows sit behind)."""
    n, L = spec.n_labels, len(spec.szs)
    sample = _a16(_carve(32 if slots > 15 else 16, slots, n, variant == "rl", variant == "pdipm"))
    phase_a = 4 * 16 * (_lds_pitch(n) * (L + 2) + sum(_lds_pitch(w) for w in spec.szs) + _lds_pitch(spec.szs[-1]))
    bundles = 16 * sample
    grouped = _a16(max(phase_a, bundles)) + _a16(2 * _row_pitch(_a16(n)) * 4) > 160 * 1024 or slots > 15
    return grouped, "bundles" if bundles > phase_a else "phase A"


def narrow_rows(spec, slots, variant):
    """dual_step_small_fits (be_dual_small.hip): the dual steps of a workgroup's samples on wave 0, bundles in registers"""
    return variant == "rl" and spec.n_labels <= 16 and slots <= 15


def kernel_instance(spec, slots, variant, path):
    """the template instance launch_fused_rows_solve / launch_fused_fc_solve pick (restated, for the printed plan line)"""
    rl, ipm, KT = variant == "rl", variant == "pdipm", 32 if slots > 15 else 16
    if path == "ROWS":
        if narrow_rows(spec, slots, variant):
            return "fused_rows_solve_kernel<true, 16, %d>" % (5 if slots <= 5 else 8 if slots <= 7 else 16)
        return "fused_rows_solve_kernel<%s, %d, 0, %s>" % (str(rl).lower(), KT, str(ipm).lower())
    return "fused_fc_solve_kernel<%s, %d, %s, %s>" % (str(rl).lower(), KT, str(ipm).lower(),
                                                      str(path == "TILE_BUDGETED_THEN_ROWS").lower())


# (spec, batch, nIter, variant, flags) -> (path, samples per workgroup) at 256 CUs; for the tile paths also (grouped, what
# the constant rows sit behind).  Grouping follows from tile_layout above: at n = 270 the bundles outgrow the LDS from
# seven slots on (16 x 13 KB), at n = 20 and 33 only the 32-slot instances group (slots > 15).
SOLVE_CASES = [
    # per-sample kernel, 1 / 2 / 3 / 4 samples per workgroup
    (("L1_n1", 1, 3, "dual", 0), ("ROWS", 1), None),
    (("L1_n1", 300, 10, "dual", 0), ("ROWS", 2), None),
    (("L1_n9", 37, 7, "dual", 0), ("ROWS", 1), None),
    (("L1_n9", 1000, 15, "dual", 0), ("ROWS", 4), None),
    (("n8_box", 37, 5, "rl", 0), ("ROWS", 1), None),                # narrow rows, 5 slots: KS = 5
    (("n16_box", 300, 7, "rl", 0), ("ROWS", 2), None),              # narrow rows, 7 slots: KS = 8
    (("n8_box", 1000, 8, "rl", 0), ("ROWS", 4), None),              # narrow rows, 8 slots: KS = 16
    (("n16_box", 600, 15, "rl", 0), ("ROWS", 3), None),             # narrow rows, 15 slots: KS = 16
    (("n16_box", 37, 16, "rl", 0), ("ROWS", 1), None),              # 16 slots: off the narrow path (32-row instance)
    (("n17_box", 300, 5, "rl", 0), ("ROWS", 2), None),              # n = 17: wave per sample
    (("n20_deep4", 37, 10, "pdipm", 0), ("ROWS", 1), None),
    (("n33", 600, 10, "dual", 0), ("ROWS", 3), None),
    (("n70", 300, 15, "dual", 0), ("ROWS", 2), None),
    (("n270", 1, 7, "dual", 0), ("ROWS", 1), None),
    (("n270", 300, 20, "pdipm", 0), ("ROWS", 2), None),
    (("deep8", 37, 20, "dual", 0), ("ROWS", 1), None),
    (("deep8", 1000, 10, "dual", 0), ("ROWS", 4), None),
    # persistent tiles, 4 rows (forced)
    (("L1_n1", 37, 7, "dual", PERS), ("TILE", 4), (False, "phase A")),
    (("n17_box", 37, 15, "rl", PERS), ("TILE", 4), (False, "bundles")),
    (("n270", 37, 3, "dual", PERS), ("TILE", 4), (False, "phase A")),
    # 8 rows
    (("L1_n9", 1100, 10, "dual", 0), ("TILE", 8), (False, "phase A")),
    (("n16_box", 1100, 10, "rl", PERS), ("TILE", 8), (False, "phase A")),
    (("n20_deep4", 1100, 7, "pdipm", 0), ("TILE", 8), (False, "phase A")),
    (("n70", 1100, 10, "pdipm", 0), ("TILE", 8), (False, "bundles")),          # ungrouped, constant rows behind the bundles
    (("n270", 1100, 10, "pdipm", 0), ("TILE", 8), (True, "bundles")),           # grouped at 10 slots
    (("n33", 1100, 36, "dual", 0), ("TILE", 8), (True, "bundles")),             # 31 slots, recycled
    (("n33", 1100, 20, "dual", PERS | SLICE), ("TILE_BUDGETED_THEN_ROWS", 8), (True, "bundles")),
    (("deep8", 1100, 15, "dual", 0), ("TILE", 8), (False, "phase A")),
    # 16 rows
    (("n8_box", 2100, 7, "rl", PERS), ("TILE", 16), (False, "phase A")),
    (("n20_deep4", 2100, 20, "pdipm", 0), ("TILE", 16), (True, "bundles")),
    (("n33", 2100, 10, "dual", 0), ("TILE", 16), (False, "phase A")),           # phase A larger than the bundles
    (("n70", 2100, 7, "dual", 0), ("TILE", 16), (False, "bundles")),
    (("n70", 2100, 10, "pdipm", 0), ("TILE", 16), (False, "bundles")),          # ... read by sixteen interior-point solves
    (("n270", 2100, 15, "dual", 0), ("TILE", 16), (True, "bundles")),           # grouped at 15 slots
    (("deep8", 2100, 3, "dual", 0), ("TILE", 16), (False, "phase A")),
]


def _case_id(args):
    return "%s_%d_%d_%s_%d" % args


def _slots(n_iter):
    return min(n_iter, _lib.MAX_SLOTS)


# ------------------------------------------------------------------------------------------------ CPU


@pytest.mark.parametrize("args,expected,layout", SOLVE_CASES, ids=[_case_id(c[0]) for c in SOLVE_CASES])
def test_every_case_names_its_path(args, expected, layout):
    name, B, n_iter, variant, flags = args
    spec = SPECS[name]
    got = plan(spec, B, n_iter, variant, flags, cus=CUS)
    assert got[:2] == expected, got
    assert plan(spec, B, n_iter, variant, TWO, cus=CUS)[0].startswith("ROUNDS")
    assert (layout is None) == (expected[0] == "ROWS")
    if layout is not None:
        assert tile_layout(spec, _slots(n_iter), variant) == layout


def test_cases_cover_the_paths_and_layouts():
    seen = {c[1] for c in SOLVE_CASES}
    assert {("ROWS", 1), ("ROWS", 2), ("ROWS", 4), ("TILE", 4), ("TILE", 8), ("TILE", 16)} <= seen
    assert any(c[1][0] == "TILE_BUDGETED_THEN_ROWS" for c in SOLVE_CASES)
    tiles = [c for c in SOLVE_CASES if c[2] is not None]
    assert any(c[2][0] and _slots(c[0][2]) <= 15 for c in tiles)               # grouped for another reason than slots > 15
    assert any(c[2] == (False, "bundles") for c in tiles) and any(c[2] == (False, "phase A") for c in tiles)
    rl_rows = {kernel_instance(SPECS[c[0][0]], _slots(c[0][2]), c[0][3], "ROWS") for c in SOLVE_CASES
               if c[1][0] == "ROWS" and c[0][3] == "rl"}
    assert {"fused_rows_solve_kernel<true, 16, 5>", "fused_rows_solve_kernel<true, 16, 8>",
            "fused_rows_solve_kernel<true, 16, 16>", "fused_rows_solve_kernel<true, 32, 0, false>",
            "fused_rows_solve_kernel<true, 16, 0, false>"} <= rl_rows
    assert {_slots(c[0][2]) for c in SOLVE_CASES if c[0][0] in ("n8_box", "n16_box") and c[1][0] == "ROWS"} == {5, 7, 8, 15, 16}
    assert {3, 7, 10, 15, 20, 36} <= {c[0][2] for c in SOLVE_CASES}


def test_layout_restatement_agrees_with_the_library():
    """_carve against icnn_be_dual_lds_bytes (the interior-point carve with its own constant rows) at every label count and
    slot count of the cases, and the specs against the model check: all accepted."""
    lib = _lib.load()
    for name, spec in SPECS.items():
        for slots in (1, 3, 5, 7, 8, 10, 15, 16, 20, 31):
            assert lib.icnn_be_dual_lds_bytes(spec.n_labels, slots, _lib.CUT_F32) == \
                _carve(32 if slots > 15 else 16, slots, spec.n_labels, False, True, True), (name, slots)
        assert plan(spec, 64, 10, "dual")[0] == "ROWS", name
    assert DEEP.n_layers == _lib.MAX_LAYERS
    assert [_pw_leaves(n) for n in (1, 8, 9, 128, 129, 270)] == [1, 1, 1, 1, 2, 3]


@pytest.mark.parametrize("name", ["n8_box", "n16_box", "n17_box"])
def test_gd_entry_refuses_the_box_specs(name):
    """icnn_be_fc_gd is not a model of the RL wrapper's box: refused before anything is launched (placeholder pointers)"""
    spec = SPECS[name]
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width, m.wpack = spec.alpha, 1, spec.ctx_width, 64
    fake = C.c_void_p(64)
    assert _lib.load().icnn_be_fc_gd(C.byref(m), fake, fake, 37, 4, 0.01, 0.3, fake, None, None, fake, None) == -1


# ------------------------------------------------------------------------------------------------ problems


# Sections 3 and 5: y-path scales (z*_yu/W, z*_zu_proj/W) that keep |dE/dy| at O(1).  At the "spread" scale the gradients of
# deep8 reach 200, y saturates, and the projected Newton solve of the float64 reference runs into its 100-update cap on
# half the samples (on 6 % at n33): no batch would pass the screen.  Section 5 uses them too (unscaled, deep8's y moves by
# thousands in nine steps); sections 2 and 4 use the unscaled models.
TAME = {"deep8": (0.5, 0.5), "n33": (0.4, 1.0)}


def _problem(spec, B, seed, tame=None, x_scale=1.0):
    kw = dict(yu_bias=1.0, gate_bias=1.0) if spec.action_box else {}
    params = _perturbed(picnn.init_params(spec, seed, "spread", **kw), np.random.RandomState(seed + 50))
    if tame is not None:
        for k in params:
            if k.endswith("_yu/W"):
                params[k] = params[k] * np.float32(tame[0])
            elif k.endswith("_zu_proj/W"):
                params[k] = params[k] * np.float32(tame[1])
    x = (x_scale * np.random.RandomState(seed + 100).randn(B, spec.n_features)).astype(np.float32)
    return params, x


def _need_256_cus():
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    if cus != CUS:
        print("skipped: the plans of this module are stated for %d CUs, the device has %d" % (CUS, cus))
        pytest.skip("the plans of this module are stated for %d CUs, the device has %d" % (CUS, cus))


def _first_difference(a, b):
    idx = np.argwhere(np.asarray(a != b).reshape(len(a), -1).any(axis=1)).ravel()
    return "%d samples differ, first %d" % (len(idx), idx[0])


# ------------------------------------------------------------------------------------------------ GPU: section 2


@pytest.mark.gpu
@pytest.mark.parametrize("args,expected,layout", SOLVE_CASES, ids=[_case_id(c[0]) for c in SOLVE_CASES])
def test_fused_solve_equals_launch_pairs(args, expected, layout):
    """The planned path against one launch per phase and round (ICNN_BE_FLAG_TWO_KERNELS): same device functions, every
    output bit-identical.  The narrow-row cases run a third time with ICNN_BE_FLAG_WAVE_PER_SAMPLE added, so the quad dual
    step inside the fused kernel also meets the wave-per-sample code.  nIter 36 keeps 31 slots and recycles them: equal
    `active` and `count` arrays are in particular equal active-set sizes."""
    from icnn_amd import bundle_entropy
    _need_256_cus()
    name, B, n_iter, variant, flags = args
    spec = SPECS[name]
    params, x = _problem(spec, B, 7)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    instance = kernel_instance(spec, _slots(n_iter), variant, expected[0])
    runs = [flags, TWO] + ([TWO | WPS] if narrow_rows(spec, _slots(n_iter), variant) else [])
    outs, plans = [], []
    for fl in runs:
        res = bundle_entropy.FusedSolver(model, B, n_iter, variant, flags=fl).solve(ctx, 0.5)
        plans.append(_planned(model, res))
        outs.append(_all_outputs(res, B))
        assert res.state.T == _slots(n_iter)
    newton, count = outs[0][5], outs[0][3]
    print("%s B=%d nIter=%d %s flags=%d: plan %s, %s%s; against %s; cuts held %s, most Newton updates of a sample %d"
          % (name, B, n_iter, variant, flags, plans[0], instance,
             "" if layout is None else ", %s, constant rows behind %s" % ("grouped" if layout[0] else "ungrouped", layout[1]),
             [p[0] for p in plans[1:]], np.bincount(count), newton.max()))
    assert plans[0][:2] == expected, plans
    assert all(p[0].startswith("ROUNDS") for p in plans[1:]), plans
    for other, p in zip(outs[1:], plans[1:]):
        for what, a, b in zip(OUTPUTS, outs[0], other):
            assert np.array_equal(a, b), "%s differs from %s: %s" % (what, p[0], _first_difference(a, b))
    if spec.n_labels == 1:
        assert newton.max() == 0 and (count == 1).all() and (outs[0][9] == 1).all()      # the rank test, module docstring
    elif variant == "pdipm":
        assert newton.max() == 0 and count.max() > 1                                     # no Newton counter, module docstring
    else:
        assert newton.max() > 1


# ------------------------------------------------------------------------------------------------ GPU: section 3


# architecture -> (batch, flags, first seed of the screen, (path, samples per workgroup)); nIter 10, 5 for variant rl
ORACLE_CASES = {
    "L1_n1": (64, 0, 1, ("ROWS", 1)),
    "L1_n9": (130, 0, 1, ("ROWS", 1)),
    "n8_box": (130, 0, 1, ("ROWS", 1)),
    "n16_box": (300, 0, 1, ("ROWS", 2)),
    "n17_box": (64, PERS, 1, ("TILE", 4)),
    "n20_deep4": (65, 0, 1, ("ROWS", 1)),
    "n33": (100, PERS, 1, ("TILE", 4)),
    "n70": (48, PERS, 1, ("TILE", 4)),
    "n270": (40, PERS, 1, ("TILE", 4)),
    "deep8": (64, 0, 1, ("ROWS", 1)),
}
VARIANT = {"n8_box": "rl", "n16_box": "rl", "n17_box": "rl", "n20_deep4": "pdipm", "n70": "pdipm", "n270": "pdipm"}


def _oracle_run(spec, params, flat_ctx, n_iter, variant):
    """(result, clean, most updates of one inner solve): clean = what the device calls status 0 -- no singular system (variant
    rl swallows it: counted at numpy.linalg.solve), no LinAlgError, every y finite"""
    fg = picnn_oracle.make_fg_chain(params, flat_ctx, list(spec.szs), spec.alpha, spec.action_box)
    singular, real = [0], np.linalg.solve

    def counting_solve(*a, **kw):
        try:
            return real(*a, **kw)
        except np.linalg.LinAlgError:
            singular[0] += 1
            raise
    try:
        with np.errstate(all="ignore"), mock.patch.object(np.linalg, "solve", counting_solve):
            ora = oracle.solve_batch(fg, np.full((len(flat_ctx), spec.n_labels), 0.5), n_iter, variant=variant)
    except np.linalg.LinAlgError:
        return None, False, 0
    return ora, singular[0] == 0 and bool(np.isfinite(ora.y).all()), max(ora.newton_counts or [0])


@functools.lru_cache(maxsize=None)
def _screened_problem(name):
    """The first seed on which the oracle ALONE (host context) is clean on every sample and no inner solve reaches its cap
    (100 Newton updates, 20 for rl and for the interior point): a capped solve stops on a limit cycle at its rounding floor,
    where the reference does not reproduce itself."""
    spec, (B, _, seed0, _) = SPECS[name], ORACLE_CASES[name]
    variant = VARIANT.get(name, "dual")
    n_iter = 5 if variant == "rl" else 10
    for seed in range(seed0, seed0 + 100):
        params, x = _problem(spec, B, seed, TAME.get(name))
        host_ctx = picnn.context(spec, params, torch.from_numpy(x)).numpy()
        ora, clean, most = _oracle_run(spec, params, host_ctx, n_iter, variant)
        if clean and most < oracle.VARIANTS[variant].newton_cap:
            return seed, params, x, variant, n_iter
    raise AssertionError("no screened seed")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_fused_solve_matches_chain_order_oracle(name):
    """test_fused_matches_chain_order_oracle at these architectures, on the whole batch: identical active sets and nIters,
    status 0 on both sides, max|dy| <= 1e-7 (dual, pdipm) / 1e-6 (rl)."""
    from icnn_amd import bundle_entropy
    _need_256_cus()
    spec, (B, flags, _, expected) = SPECS[name], ORACLE_CASES[name]
    seed, params, x, variant, n_iter = _screened_problem(name)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=np.full((B, spec.n_labels), 0.5), nIter=n_iter, variant=variant,
                                    native=True, check=False, flags=flags)
    got_plan = _planned(model, res)
    ora, clean, most = _oracle_run(spec, params, ctx.cpu().numpy(), n_iter, variant)
    host = result_to_host(res)
    assert ora is not None
    dy, discrete = compare_with_oracle(host, ora)
    tol = 1e-6 if variant == "rl" else 1e-7
    print("%s seed %d B=%d nIter=%d %s, plan %s: max|dy| = %.3e (bound %.0e), %d discrete differences, cuts %s, "
          "most updates of one inner solve: oracle %d" % (name, seed, B, n_iter, variant, got_plan, dy.max(), tol, len(discrete),
                                                         np.bincount([len(a) for a in host["active"]]), most))
    assert got_plan[:2] == expected, got_plan
    assert clean and (host["status"] == 0).all(), (clean, np.nonzero(host["status"])[0])
    assert not discrete, "samples with different active sets / nIters: %s" % discrete[:8]
    assert dy.max() <= tol, dy.max()


# ------------------------------------------------------------------------------------------------ section 4: context


CTX_SPECS = dict(SPECS, chain2=CHAIN2)
CTX_BATCHES = [1, 63, 65, 130]
MIN_VARIANCE = 1e-4


@functools.lru_cache(maxsize=None)
def _context_problem(name, B):
    """Seeded model and x; with chained BatchNorm, screened (float64, CPU) so that no normalised channel's batch variance is
    below 1e-4: a channel that is active on one or two samples is scaled by gamma / sqrt(var + 1e-5), and float32
    arithmetic itself then misses float64 by more than the kernels' bound (test_architectures._float32_restatement_error)."""
    spec = CTX_SPECS[name]
    for seed in range(11, 211):
        # x of scale 3: with twelve features and weights of 0.02 the first layer's pre-activations are otherwise smaller than
        # its perturbed biases, and some channel of every model is all but dead
        params, x = _problem(spec, B, seed, x_scale=3.0)
        ref64, stats = bn_ref.fc_context64(spec, params, x)
        low = min([float(var.min()) for _, var in stats.values()] + [np.inf])
        if low < MIN_VARIANCE:
            continue
        ref = picnn_oracle.flat_context(picnn_oracle.context(params, x, list(spec.szs), spec.batchnorm, dtype=np.float64),
                                        dtype=np.float64)
        assert ref.dtype == np.float64 and np.max(np.abs(ref - ref64)) <= 1e-12 * np.abs(ref).max()
        return seed, params, x, ref, low
    raise AssertionError("no screened seed")


def _context_cases():
    return [(name, B) for name in CTX_SPECS for B in CTX_BATCHES if B > 1 or not picnn.bn_layers(CTX_SPECS[name])]


@pytest.mark.parametrize("name", list(CTX_SPECS))
def test_context_problems_are_screened_and_the_host_mirror_agrees(name):
    """CPU: the screen finds a seed for every batch size, the lowest batch variance it leaves is at least 1e-4, and the torch
    host mirror picnn.context agrees with the float64 statement to the kernels' bound (2e-5 of its scale)."""
    spec = CTX_SPECS[name]
    for B in CTX_BATCHES:
        if (name, B) not in _context_cases():
            continue
        seed, params, x, ref, low = _context_problem(name, B)
        assert ref.shape == (B, spec.ctx_width) and low >= MIN_VARIANCE
        host = picnn.context(spec, params, torch.from_numpy(x)).numpy()
        err, scale = float(np.max(np.abs(host - ref))), float(np.abs(ref).max())
        print("%s B=%d seed %d: lowest batch variance %.2e, host mirror max err %.2e, bound 2e-5 * %.2e" % (name, B, seed, low, err, scale))
        assert err <= 2e-5 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name,B", _context_cases(), ids=["%s_%d" % c for c in _context_cases()])
def test_context_producer_matches_float64(name, B):
    spec = CTX_SPECS[name]
    seed, params, x, ref, low = _context_problem(name, B)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x)).cpu().numpy()
    assert ctx.shape == ref.shape
    err, scale = float(np.max(np.abs(ctx - ref))), float(np.abs(ref).max())
    host = picnn.context(spec, params, torch.from_numpy(x)).numpy()
    print("%s B=%d seed %d: max|ctx - ref| = %.2e, bound 2e-5 * %.2e (lowest batch variance %.2e); host mirror %.2e"
          % (name, B, seed, err, scale, low, np.max(np.abs(ctx - host))))
    assert err <= 2e-5 * scale
    assert np.max(np.abs(ctx - host)) <= 2e-5 * scale


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["deep8", "n20_deep4"])
@pytest.mark.parametrize("B", [1, 65])
def test_moving_mode_context_matches_float64(name, B):
    """bn="moving": every normalised layer with the model's moving statistics (valid at batch 1), against bn_ref.py"""
    spec = SPECS[name]
    params, x = _problem(spec, B, 21)
    stats = bn_ref.random_bn_stats(picnn.init_bn_stats(spec), 5)
    model = picnn.FCModel(spec, params)
    model.set_bn_stats(stats)
    ctx = model.context(torch.from_numpy(x), bn="moving").cpu().numpy()
    ref, _ = bn_ref.fc_context64(spec, params, x, stats)
    err, scale = float(np.max(np.abs(ctx - ref))), float(np.abs(ref).max())
    print("%s B=%d moving: max|ctx - ref| = %.2e, bound 2e-5 * %.2e" % (name, B, err, scale))
    assert err <= 2e-5 * scale


# ------------------------------------------------------------------------------------------------ GPU: section 5


@pytest.mark.gpu
@pytest.mark.parametrize("lr,mu", [(0.01, 0.3), (0.05, 0.9)])
@pytest.mark.parametrize("B", [37, 530])
@pytest.mark.parametrize("name", ["L1_n9", "n20_deep4", "n270", "deep8", "L1_n1", "n33", "n70"])
def test_gd_solve_bit_exact(name, B, lr, mu):
    """gd.solve with K = 4 and K = 9 against the float32 recurrence around the kernel-order oracle: trajectory, y_K and
    E(y_K) bit for bit.  Batch 37 takes gd_rows_kernel (at most two samples per CU), 530 gd_fc_kernel with a last tile of two
    rows.  One K = 9 reference serves both: its first four points are the K = 4 trajectory, its fifth is y_4."""
    from icnn_amd import gd
    _need_256_cus()
    spec = SPECS[name]
    params, x = _problem(spec, B, 31, TAME.get(name))
    y0 = np.random.RandomState(32).rand(B, spec.n_labels)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    flat = ctx.cpu().numpy()

    def fg(yy):
        return picnn_oracle.energy_and_grad_chain(params, flat, yy, list(spec.szs), spec.alpha)
    y9, traj9, E9 = gd_ref.unroll_f32(fg, y0, 9, lr, mu)
    E4, _ = fg(traj9[:, 4])
    refs = {9: (y9.astype(np.float64), traj9, E9), 4: (traj9[:, 4], traj9[:, :4], E4)}
    for K, (y_ref, traj_ref, E_ref) in refs.items():
        y, traj, E = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True, energy=True)
        torch.cuda.synchronize()
        assert traj.shape == (B, K, spec.n_labels) and y.dtype == torch.float64
        assert np.array_equal(traj.cpu().numpy(), traj_ref), "K=%d trajectory: %s" % (K, _first_difference(traj.cpu().numpy(), traj_ref))
        assert np.array_equal(y.cpu().numpy(), y_ref), "K=%d y_K: %s" % (K, _first_difference(y.cpu().numpy(), y_ref))
        assert np.array_equal(E.cpu().numpy(), E_ref), "K=%d E(y_K)" % K
        moved = float(np.abs(y_ref - y0.astype(np.float32)).max())
        assert moved > 1e-4                                                          # y did move
    print("%s B=%d lr=%g mu=%g: K = 4 and 9 bit-exact on %s, y moved by up to %.2e"
          % (name, B, lr, mu, "gd_rows_kernel" if (B + CUS - 1) // CUS <= 2 else "gd_fc_kernel", moved))
