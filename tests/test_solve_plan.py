"""CPU-only: the dispatch table of icnn_be_solve_fc (icnn_be_debug_solve_plan), pinned at 256 CUs (MI355X).  The plan is
host arithmetic over the model and state descriptors, so neither a GPU nor any buffer is needed (wpack and every state
pointer stay null).  The rows cover every BASELINE configuration, the shapes and flag sets of the GPU tests that compare
two dispatch paths (tests/test_gpu_parity.py), the full batches and shards of tests/test_sample_independence.py, and the
corners of the rule."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from icnn_amd import _lib, dist, picnn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
BIB, HC = picnn.bibtex_spec(), picnn.halfcheetah_spec()
PERS, SLICE, LOCK, TWO = _lib.FLAG_PERSISTENT, _lib.FLAG_TIME_SLICE, _lib.FLAG_LOCKSTEP, _lib.FLAG_TWO_KERNELS


def fc_model(spec):
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = float(spec.alpha), int(spec.action_box), spec.ctx_width
    return m


def fc_state(spec, B, n_iter, variant, flags=0, slots=None):
    """the descriptor bundle_entropy.BundleState fills, without its buffers"""
    s = _lib.State()
    slots = min(n_iter, _lib.MAX_SLOTS) if slots is None else slots
    s.batch, s.n, s.slots = B, spec.n_labels, slots
    s.iters = n_iter if n_iter > slots else 0
    s.variant, s.flags = _lib.VARIANT[variant], flags
    return s


def plan(spec, B, n_iter, variant, flags=0, slots=None, cus=CUS):
    return _lib.solve_plan(fc_model(spec), fc_state(spec, B, n_iter, variant, flags, slots), cus)


# (spec, batch, nIter, variant, flags, slots) -> (path, samples per workgroup, budget per round, value returned)
TABLE = [
    # BASELINE configurations (the FC ones; configs[3] is the 4096 x 30 batch, also per rank of its 8-way shard)
    ((BIB, 128, 10, "dual", 0, None), ("ROWS", 1, 0, 10)),                           # configs[1]
    ((BIB, 4096, 30, "dual", 0, None), ("TILE", 16, 0, 30)),                         # configs[3], one GPU
    ((BIB, 512, 30, "dual", 0, None), ("ROWS", 2, 0, 30)),                           # configs[3], one of eight shards
    ((HC, 8192, 5, "rl", 0, None), ("ROUNDS_LOCKSTEP", 0, 0, 5)),                    # configs[4]
    ((BIB, 4096, 10, "dual", 0, None), ("TILE", 16, 0, 10)),                         # the benchmark's headline
    ((BIB, 2048, 10, "dual", 0, None), ("TILE", 8, 0, 10)),                          # its shard on two GPUs
    ((BIB, 512, 10, "dual", 0, None), ("ROWS", 2, 0, 10)),                           # ... on eight
    ((BIB, 4096, 10, "pdipm", 0, None), ("TILE", 16, 0, 10)),
    # forced paths
    ((BIB, 4096, 10, "dual", PERS | SLICE, None), ("TILE_BUDGETED_THEN_ROWS", 16, 8, 11)),
    ((BIB, 4096, 30, "dual", SLICE, None), ("ROUNDS_SLICED_THEN_ROWS", 0, 8, 31)),
    ((BIB, 1100, 20, "dual", TWO, None), ("ROUNDS_SLICED_EXTRA", 0, 8, 40)),
    # variant RL: persistent tiles only when forced, in lockstep (T <= 15) and beyond
    ((HC, 210, 5, "rl", PERS, None), ("TILE", 4, 0, 5)),
    ((BIB, 1100, 20, "rl", PERS, None), ("TILE", 8, 0, 20)),
    ((BIB, 1100, 20, "rl", 0, None), ("ROUNDS_SLICED_THEN_ROWS", 0, 8, 21)),
    ((HC, 8192, 5, "rl", TWO, None), ("ROUNDS_LOCKSTEP", 0, 0, 5)),
    # pdipm: lockstep at any nIter, tiles at nIter > 15 too
    ((BIB, 1100, 20, "pdipm", 0, None), ("TILE", 8, 0, 20)),
    ((BIB, 1100, 20, "pdipm", TWO, None), ("ROUNDS_LOCKSTEP", 0, 0, 20)),
    ((BIB, 1100, 20, "pdipm", SLICE, None), ("TILE", 8, 0, 20)),
    ((BIB, 8193, 20, "pdipm", 0, None), ("ROUNDS_LOCKSTEP", 0, 0, 20)),
    ((BIB, 40, 31, "pdipm", 0, None), ("ROWS", 1, 0, 31)),
    # 4 * tiles >= cus (1009 samples: 64 tiles) and tiles <= 2 * cus (8192 samples: 512 tiles), where the per-sample kernel
    # is not taken (a forced flag, or more than four samples per CU)
    ((BIB, 1008, 10, "dual", LOCK, None), ("ROUNDS_LOCKSTEP", 0, 0, 10)),
    ((BIB, 1009, 10, "dual", LOCK, None), ("TILE", 4, 0, 10)),
    ((BIB, 1024, 10, "dual", 0, None), ("ROWS", 4, 0, 10)),
    ((BIB, 1025, 10, "dual", 0, None), ("TILE", 8, 0, 10)),
    ((BIB, 8192, 10, "dual", 0, None), ("TILE", 16, 0, 10)),
    ((BIB, 8193, 10, "dual", 0, None), ("ROUNDS_LOCKSTEP", 0, 0, 10)),
    ((BIB, 16384, 30, "dual", 0, None), ("TILE", 16, 0, 30)),                        # nIter > 15: no upper bound
    ((BIB, 1008, 30, "dual", SLICE | PERS, None), ("TILE_BUDGETED_THEN_ROWS", 4, 8, 31)),
    ((BIB, 1008, 30, "dual", LOCK, None), ("ROUNDS_LOCKSTEP", 0, 0, 30)),
    # tests/test_sample_independence.py: the smallest batches at which the default dispatch puts the full batch and its
    # contiguous shards (dist.shard_bounds, world 2, 4, 8) on different kernels; every path is the one the rule was expected to
    # give, no batch size had to move.  1043 = 130 tiles of 8 and one of 3, 260 quads and one of 3
    ((BIB, 1043, 10, "dual", 0, None), ("TILE", 8, 0, 10)),
    ((BIB, 522, 10, "dual", 0, None), ("ROWS", 3, 0, 10)),
    ((BIB, 521, 10, "dual", 0, None), ("ROWS", 3, 0, 10)),
    ((BIB, 261, 10, "dual", 0, None), ("ROWS", 2, 0, 10)),
    ((BIB, 260, 10, "dual", 0, None), ("ROWS", 2, 0, 10)),
    ((BIB, 131, 10, "dual", 0, None), ("ROWS", 1, 0, 10)),
    ((BIB, 130, 10, "dual", 0, None), ("ROWS", 1, 0, 10)),
    ((BIB, 1, 10, "dual", 0, None), ("ROWS", 1, 0, 10)),                             # one sample alone
    ((BIB, 1043, 20, "dual", 0, None), ("TILE", 8, 0, 20)),                          # nIter > 15: the 32-slot tile instance
    ((BIB, 522, 20, "dual", 0, None), ("ROWS", 3, 0, 20)),
    ((BIB, 261, 20, "dual", 0, None), ("ROWS", 2, 0, 20)),
    ((BIB, 131, 20, "dual", 0, None), ("ROWS", 1, 0, 20)),
    ((BIB, 2051, 10, "dual", 0, None), ("TILE", 16, 0, 10)),
    ((BIB, 1026, 10, "dual", 0, None), ("TILE", 8, 0, 10)),                          # 16-row against 8-row tiles
    ((BIB, 513, 10, "dual", 0, None), ("ROWS", 3, 0, 10)),
    ((BIB, 257, 10, "dual", 0, None), ("ROWS", 2, 0, 10)),
    ((BIB, 256, 10, "dual", 0, None), ("ROWS", 1, 0, 10)),
    ((BIB, 1043, 10, "pdipm", 0, None), ("TILE", 8, 0, 10)),
    ((BIB, 522, 10, "pdipm", 0, None), ("ROWS", 3, 0, 10)),
    ((BIB, 131, 10, "pdipm", 0, None), ("ROWS", 1, 0, 10)),
    ((HC, 1043, 5, "rl", 0, None), ("ROUNDS_LOCKSTEP", 0, 0, 5)),                    # the four-samples-per-wave dual step
    ((HC, 522, 5, "rl", 0, None), ("ROWS", 3, 0, 5)),
    ((HC, 261, 5, "rl", 0, None), ("ROWS", 2, 0, 5)),
    ((HC, 131, 5, "rl", 0, None), ("ROWS", 1, 0, 5)),
]

# the shapes and flag sets of the GPU tests that compare two dispatch paths: (test, spec, B, nIter, variant, slots, flags A,
# flags B); each pair must take two different paths
PAIRS = [("pdipm_persistent", BIB, B, T, "pdipm", None, 0, TWO)
         for B, T in [(100, 10), (300, 6), (1100, 10), (1100, 20), (40, 31)]] + \
        [("persistent_tile", BIB, B, T, "dual", None, PERS, TWO)
         for B, T in [(100, 10), (1100, 6), (16, 15), (1100, 12), (300, 14), (530, 24), (40, 31)]] + \
        [("per_sample", spec, B, T, v, None, 0, TWO)
         for spec, B, T, v in [(BIB, 100, 10, "dual"), (BIB, 1, 7, "dual"), (BIB, 256, 4, "dual"), (HC, 210, 5, "rl"),
                               (HC, 1, 5, "rl"), (BIB, 301, 6, "dual"), (BIB, 70, 30, "dual"), (BIB, 400, 22, "dual"),
                               (HC, 333, 17, "rl"), (BIB, 700, 5, "dual"), (BIB, 1001, 4, "dual"), (HC, 1024, 5, "rl")]] + \
        [("stragglers", BIB, 1100, 20, "dual", None, 0, TWO)] + \
        [("budgeted_tile", BIB, B, T, "dual", None, PERS, PERS | SLICE) for B, T in [(1100, 20), (700, 10), (4096, 30)]] + \
        [("tile_rl", HC, 210, 5, "rl", None, PERS, TWO)] + \
        [("valu_contraction", BIB, B, T, "dual", None, m, m | TWO) for B, T in [(100, 10), (1100, 10), (300, 14)]
         for m in (0, _lib.FLAG_MFMA_CONTRACTION)] + \
        [("recycled_slots", BIB, B, T, "dual", None, 0, TWO) for B, T in [(48, 40), (1100, 36), (20, 64)]] + \
        [("overflow", BIB, B, T, "dual", S, 0, TWO) for B, S, T in [(1100, 16, 40), (1100, 20, 36), (40, 16, 40)]] + \
        [("time_sliced", BIB, 1100, 30, "dual", None, SLICE, LOCK)]

# tests/test_sample_independence.py solves a full batch in one launch and again as the contiguous shards of `world` ranks:
# (spec, B, nIter, variant) x world; the full batch and at least one shard must differ in (path, samples per workgroup)
FULL_BATCHES = [(BIB, 1043, 10, "dual"), (BIB, 1043, 20, "dual"), (BIB, 2051, 10, "dual"), (BIB, 1043, 10, "pdipm"),
                (HC, 1043, 5, "rl")]
WORLDS = (2, 4, 8)
SHARDS = [full + (world,) for full in FULL_BATCHES for world in WORLDS]


@pytest.mark.parametrize("args,expected", TABLE, ids=["%d_%d_%s_%d" % (a[1], a[2], a[3], a[4]) for a, _ in TABLE])
def test_solve_plan_table(args, expected):
    assert plan(*args) == expected


@pytest.mark.parametrize("pair", PAIRS, ids=["%s_%d_%d_%s" % (p[0], p[2], p[3], p[4]) for p in PAIRS])
def test_dispatch_pairs_of_the_gpu_tests_take_different_paths(pair):
    _, spec, B, n_iter, variant, slots, fa, fb = pair
    a, b = plan(spec, B, n_iter, variant, fa, slots), plan(spec, B, n_iter, variant, fb, slots)
    assert a[0] != b[0], (a, b)


@pytest.mark.parametrize("case", SHARDS, ids=["%d_%d_%s_world%d" % c[1:] for c in SHARDS])
def test_shards_of_the_sample_independence_tests_leave_the_full_batchs_kernel(case):
    spec, B, n_iter, variant, world = case
    full = plan(spec, B, n_iter, variant)
    sizes = sorted({hi - lo for lo, hi in (dist.shard_bounds(B, world, r) for r in range(world))})
    shards = [plan(spec, size, n_iter, variant) for size in sizes]
    assert any(s[:2] != full[:2] for s in shards), (full, shards)


def test_profile_buffer_changes_no_path():
    """dual_step_small_fits (narrow rows, variant RL) depends on whether a dual-step profile buffer is set: that switches
    kernel instances inside a path (the quad dual step or the wave-per-sample one), never the path itself"""
    lib = _lib.load()
    cases = [(HC, 8192, 5, "rl", 0), (HC, 210, 5, "rl", 0), (HC, 8192, 5, "rl", PERS), (HC, 2048, 20, "rl", 0)]
    plain = [plan(*c) for c in cases]
    dummy = (C.c_longlong * 1)()
    lib.icnn_be_debug_profile(C.cast(dummy, C.POINTER(C.c_longlong)))
    try:
        profiled = [plan(*c) for c in cases]
    finally:
        lib.icnn_be_debug_profile(None)
    assert profiled == plain == [("ROUNDS_LOCKSTEP", 0, 0, 5), ("ROWS", 1, 0, 5), ("TILE", 16, 0, 5),
                                 ("ROUNDS_SLICED_THEN_ROWS", 0, 8, 21)]


def test_tile_budget_knob_is_read_once_and_passed_to_the_plan():
    """ICNN_BE_TILE_BUDGET (read once per process): nIter > 15 tiles with an update budget and a finishing launch; variant RL
    has no budgeted tile kernel and falls through to time-sliced launch pairs"""
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_solve_plan as t; "
            "print(t.plan(t.BIB, 4096, 30, 'dual'), t.plan(t.BIB, 1100, 20, 'rl', t.PERS), t.plan(t.BIB, 4096, 10, 'dual'))"
            % (REPO, os.path.join(REPO, "tests")))
    env = dict(os.environ, ICNN_BE_TILE_BUDGET="6")
    out = subprocess.run([sys.executable, "-s", "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout
    assert out.stdout.strip().splitlines()[-1] == str(("TILE_BUDGETED_THEN_ROWS", 16, 6, 31)) + " " + \
        str(("ROUNDS_SLICED_THEN_ROWS", 0, 8, 21)) + " " + str(("TILE", 16, 0, 10))


def test_solve_plan_validates_like_the_solve():
    lib = _lib.load()
    out = (C.c_int * 3)()
    m, s = fc_model(BIB), fc_state(BIB, 128, 10, "dual")
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, C.byref(out)) == 0
    s.batch = 0
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, C.byref(out)) == -1     # nothing to plan
    s.batch, s.flags = 128, _lib.FLAG_F64_ENERGY
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, C.byref(out)) == -1     # the fused energies are float32
    s.flags, s.cut_dtype = 0, _lib.CUT_F64
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, C.byref(out)) == -1
    s.cut_dtype, s.n = _lib.CUT_F32, 158
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, C.byref(out)) == -1     # state and model disagree on n
    s.n, m.ctx_width = 159, 7
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, C.byref(out)) == -1     # model rejected
    m.ctx_width = BIB.ctx_width
    assert lib.icnn_be_debug_solve_plan(None, C.byref(s), CUS, C.byref(out)) == -1
    assert lib.icnn_be_debug_solve_plan(C.byref(m), C.byref(s), CUS, None) == -1
