"""FC-PICNN networks whose 16-sample evaluation tile outgrows the LDS: narrow tiles of 8 or 4 rows
(icnn_be_fc_model.tile_rows, icnn_be_fc_tile_rows; DESIGN.md, "Narrow evaluation tiles").

The row count of the tile is a property of the model.  Nothing an output element is computed from depends on it -- every
element keeps its k-ordered fma chain --, so a narrow model agrees bit for bit with the order-matched oracle
(oracle/picnn_oracle.py, energy_and_grad_chain), with the 16-row tile of a network that also fits 16 rows, and with the
per-sample rows kernel.  The tests force narrow tiles on small networks that fit 16 rows (FCSpec.tile_rows), and run the
shapes of the reference's multi-label experiment that need them: bibtex with --layerSizes 600 600 (8 rows) and delicious
with --layerSizes 600 (4 rows).  The plans are stated for 256 CUs (tests/test_solve_plan.py, CUS).

pgd.solve has no bit-exact NumPy statement (its update takes device logarithms; tests/test_pgd.py bounds it instead), so
its tile form on narrow tiles is held bit for bit against its rows form -- the same samples in slices of at most two per
CU, on a kernel that shares no tile code -- and against the 16-row tile form."""
import ctypes as C
import dataclasses
import functools

import numpy as np
import pytest
import torch

import bn_ref
import gd_ref
from gpu_util import compare_with_oracle, result_to_host
from icnn_amd import _lib, picnn
from oracle import bundle_entropy_oracle as oracle
from oracle import picnn_oracle
from test_fc_solve_architectures import OUTPUTS, SPECS, _first_difference, _lds_pitch, _need_256_cus, _oracle_run, _problem
from test_gpu_parity import _all_outputs, _planned
from test_solve_plan import CUS, fc_state

TWO = _lib.FLAG_TWO_KERNELS
LDS_BYTES = 160 * 1024

# the table of the issue: (--dataset, --layerSizes) -> bytes of the tile at 16, 8, 4 rows (None: not stated) and the rows chosen
TABLE = [
    (picnn.bibtex_spec, (600,), (118272, None, None), 16),
    (picnn.bibtex_spec, (600, 600), (172544, 86272, None), 8),
    (picnn.bookmarks_spec, (600,), (142848, None, None), 16),
    (picnn.bookmarks_spec, (600, 600), (201216, 100608, None), 8),
    (picnn.delicious_spec, (600,), (462336, 231168, 115584), 4),
    (picnn.delicious_spec, (600, 600), (573952, 286976, 143488), 4),
]
BIB2 = picnn.bibtex_spec((600, 600))          # the default architecture of the reference's ebundle-vs-gd.py: 8 rows
DELI = picnn.delicious_spec((600,))           # 983 labels: 4 rows


def tile_bytes(spec, R):
    """4 R (pitch(n) (L + 2) + sum pitch(szs) + pitch(szs[-1])): fc_geom, be_picnn_fc_dev.h, restated"""
    L = len(spec.szs)
    return 4 * R * (_lds_pitch(spec.n_labels) * (L + 2) + sum(_lds_pitch(w) for w in spec.szs) + _lds_pitch(spec.szs[-1]))


def c_model(spec, tile_rows=0):
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width, m.tile_rows = float(spec.alpha), int(spec.action_box), spec.ctx_width, tile_rows
    return m


# ------------------------------------------------------------------------------------------------ CPU


def test_specs_of_the_three_datasets():
    assert picnn.bibtex_spec() == picnn.FCSpec(1836, 159, (600, 159)) and picnn.bibtex_spec().tile_rows is None
    assert picnn.bibtex_spec((600, 600)).szs == (600, 600, 159)
    assert (picnn.bookmarks_spec().n_features, picnn.bookmarks_spec().n_labels, picnn.bookmarks_spec().szs) == (2150, 208, (600, 208))
    assert (picnn.delicious_spec().n_features, picnn.delicious_spec().n_labels, picnn.delicious_spec().szs) == (500, 983, (600, 983))
    assert picnn.delicious_spec((600, 600)).szs == (600, 600, 983)


@pytest.mark.parametrize("make,szs,stated,rows", TABLE, ids=["%s_%s" % (t[0].__name__[:-5], "_".join(map(str, t[1]))) for t in TABLE])
def test_tile_rows_of_the_six_shapes(make, szs, stated, rows):
    lib = _lib.load()
    spec = make(szs)
    for R, want in zip((16, 8, 4), stated):
        assert want is None or tile_bytes(spec, R) == want, (R, tile_bytes(spec, R))
    assert rows == max(R for R in (16, 8, 4) if tile_bytes(spec, R) <= LDS_BYTES)
    for given in (0, 16, 8, 4, 5, -1):                              # shape->tile_rows is ignored
        assert lib.icnn_be_fc_tile_rows(C.byref(c_model(spec, given))) == rows
    # the struct field: 0 and 16 are the 16-row tile with its refusal, 8 and 4 fit or not by their own bytes
    for given in (0, 16, 8, 4):
        fits = tile_bytes(spec, given or 16) <= LDS_BYTES
        assert (lib.icnn_be_fc_pack_floats(C.byref(c_model(spec, given))) > 0) == fits, given


def test_tile_rows_refuses_what_is_not_a_network():
    lib = _lib.load()
    assert lib.icnn_be_fc_tile_rows(None) == _lib.EINVAL
    m = c_model(BIB2)
    m.width[BIB2.n_layers - 1] = 2                                  # last layer not scalar
    assert lib.icnn_be_fc_tile_rows(C.byref(m)) == _lib.EINVAL
    m = c_model(BIB2)
    m.n_layers = 1
    assert lib.icnn_be_fc_tile_rows(C.byref(m)) == _lib.EINVAL
    wide = picnn.FCSpec(12, 983, (4000, 983))                       # not even four rows
    assert tile_bytes(wide, 4) > LDS_BYTES
    assert lib.icnn_be_fc_tile_rows(C.byref(c_model(wide))) == _lib.ELIMIT


def test_pack_floats_and_the_struct_size():
    lib = _lib.load()
    assert lib.icnn_be_fc_pack_floats(C.byref(c_model(BIB2, 0))) == 0
    assert lib.icnn_be_fc_pack_floats(C.byref(c_model(BIB2, 16))) == 0
    assert lib.icnn_be_fc_pack_floats(C.byref(c_model(BIB2, 8))) > 0
    bib = picnn.bibtex_spec()
    counts = {lib.icnn_be_fc_pack_floats(C.byref(c_model(bib, R))) for R in (0, 16, 8, 4)}
    assert len(counts) == 1 and counts.pop() > 0
    assert lib.icnn_be_fc_pack_floats(C.byref(c_model(bib, 5))) == 0
    assert lib.icnn_be_fc_pack_floats(C.byref(c_model(bib, -1))) == 0
    assert C.sizeof(_lib.FcModel) == lib.icnn_be_struct_size(1) == 64
    assert _lib.FcModel.tile_rows.offset == _lib.FcModel.ctx_width.offset + 4 and _lib.ABI_VERSION == 12


def test_the_pack_does_not_depend_on_the_tile_rows():
    lib = _lib.load()
    spec = SPECS["n20_deep4"]
    params = picnn.init_params(spec, 3, "spread")
    L1 = spec.n_layers
    yu = (C.c_void_p * L1)(*[params["z%d_yu/W" % i].ctypes.data for i in range(L1)])
    zu = (C.c_void_p * L1)(*([None] + [params["z%d_zu_proj/W" % i].ctypes.data for i in range(1, L1)]))
    packs = []
    for R in (16, 8, 4):
        m = c_model(spec, R)
        host = np.full(lib.icnn_be_fc_pack_floats(C.byref(m)), np.nan, dtype=np.float32)
        assert lib.icnn_be_fc_pack(C.byref(m), yu, zu, host.ctypes.data) == 0
        packs.append(host)
    assert np.array_equal(packs[0], packs[1]) and np.array_equal(packs[0], packs[2]) and np.isfinite(packs[0]).all()
    assert lib.icnn_be_fc_pack(C.byref(c_model(spec, 5)), yu, zu, packs[0].ctypes.data) == _lib.EINVAL


@pytest.mark.parametrize("spec,rows", [(DELI, 4), (BIB2, 8)], ids=["delicious_600", "bibtex_600_600"])
@pytest.mark.parametrize("n_iter", [10, 30])
@pytest.mark.parametrize("B", [40, 1100, 4096])
def test_a_narrow_model_has_a_plan_at_every_batch(spec, rows, B, n_iter):
    """the per-sample kernel up to four samples per CU where its layout fits, launch pairs beyond: never the persistent tiles"""
    m = c_model(spec, rows)
    for variant in ("dual", "pdipm"):
        for flags in (0, TWO, _lib.FLAG_PERSISTENT):
            out = (C.c_int * 3)()
            rc = _lib.load().icnn_be_debug_solve_plan(C.byref(m), C.byref(fc_state(spec, B, n_iter, variant, flags)), CUS, C.byref(out))
            assert rc >= 0, (variant, flags, rc)
            path = _lib.PATHS[rc]
            assert path == "ROWS" or path.startswith("ROUNDS"), path
            if flags == 0 and B == 40 and (n_iter == 10 or spec is BIB2):     # (30 bundle rows of 983 floats and the rows
                assert (path, out[0]) == ("ROWS", 1)                          #  layout outgrow the LDS: launch pairs)
    # ... and the same shape with the 16-row tile stays refused
    out = (C.c_int * 3)()
    assert _lib.load().icnn_be_debug_solve_plan(C.byref(c_model(spec, 0)), C.byref(fc_state(spec, B, n_iter, "dual")), CUS,
                                                C.byref(out)) == _lib.ELIMIT


def test_a_narrow_model_never_matches_the_fixed_instance():
    bib = picnn.bibtex_spec()
    st = fc_state(bib, 4096, 10, "dual")
    lib = _lib.load()
    assert _lib.SHAPE_INSTANCES[lib.icnn_be_debug_shape_instance(C.byref(c_model(bib, 0)), C.byref(st))] != "generic"
    assert lib.icnn_be_debug_shape_instance(C.byref(c_model(bib, 8)), C.byref(st)) == 0
    assert lib.icnn_be_debug_shape_instance(C.byref(c_model(bib, 4)), C.byref(st)) == 0
    assert _lib.SHAPE_INSTANCES[0] == "generic"


def test_the_rl_entries_refuse_narrow_models():
    """icnn_be_adam_fc*, their plans and icnn_be_rl_bundle_solve own 16-row layouts: ICNN_BE_ELIMIT before any launch
    (placeholder pointers)"""
    lib = _lib.load()
    spec = dataclasses.replace(picnn.halfcheetah_spec(), action_box=False)
    fake = C.c_void_p(64)
    out = (C.c_int * 4)()
    for R in (8, 4):
        m = c_model(spec, R)
        m.wpack = 64
        assert lib.icnn_be_adam_fc(C.byref(m), fake, 4, 10, fake, fake, fake, fake, None) == _lib.ELIMIT
        assert lib.icnn_be_adam_fc_each(C.byref(m), fake, 4, 10, fake, fake, fake, fake, None) == _lib.ELIMIT
        assert lib.icnn_be_debug_adam_each_plan(C.byref(m), 4, C.byref((C.c_int * 2)())) == _lib.ELIMIT
        assert lib.icnn_be_debug_adam_plan(C.byref(m), None, 4, C.byref(out)) == _lib.ELIMIT
    assert lib.icnn_be_debug_adam_each_plan(C.byref(c_model(spec, 16)), 4, C.byref((C.c_int * 2)())) >= 0


# ------------------------------------------------------------------------------------------------ problems


def _sparse_problem(spec, B, seed, tame=None):
    """the multi-label inputs of the other tests: 'spread' weights, 4 % of the binary features set; tame: factors on the
    y-path weights (z*_yu/W, z*_zu_proj/W), as test_fc_solve_architectures.TAME"""
    params = picnn.init_params(spec, seed, "spread")
    if tame is not None:
        for k in params:
            if k.endswith("_yu/W"):
                params[k] = params[k] * np.float32(tame[0])
            elif k.endswith("_zu_proj/W"):
                params[k] = params[k] * np.float32(tame[1])
    x = (np.random.RandomState(seed + 100).rand(B, spec.n_features) < 0.04).astype(np.float32)
    return params, x


def _with_rows(spec, R):
    return dataclasses.replace(spec, tile_rows=R)


@functools.lru_cache(maxsize=None)
def _forced(name):
    """a small network that fits 16 rows: models with 16, 8 and 4 rows on the same weights, a context of 530 rows, y, and the
    oracle's E and dE/dy of those rows (computed once; read-only)"""
    spec = SPECS[name]
    params, x = _problem(spec, 530, 7)
    models = {R: picnn.FCModel(_with_rows(spec, R), params) for R in (16, 8, 4)}
    ctx = models[16].context(torch.from_numpy(x))
    y = np.random.RandomState(8).rand(530, spec.n_labels)
    E, g = picnn_oracle.energy_and_grad_chain(params, ctx.cpu().numpy(), y, list(spec.szs), spec.alpha)
    E, g = np.asarray(E, np.float32), np.asarray(g, np.float32)
    E.setflags(write=False)
    g.setflags(write=False)
    return spec, models, ctx, y, E, g


@functools.lru_cache(maxsize=None)
def _real(which, B, seed=11):
    spec = {"bib2": BIB2, "deli": DELI, "bib": picnn.bibtex_spec()}[which]
    params, x = _sparse_problem(spec, B, seed)
    model = picnn.FCModel(spec, params)
    ctx = model.context(torch.from_numpy(x))
    return spec, params, model, ctx


def _fg(model, ctx, y):
    f, g = model.fg(ctx, torch.from_numpy(np.ascontiguousarray(y)).cuda())
    torch.cuda.synchronize()
    return f.cpu().numpy(), g.cpu().numpy()


# ------------------------------------------------------------------------------------------------ GPU: E and dE/dy


@pytest.mark.gpu
@pytest.mark.parametrize("B", ["lt", "eq", 513, 530])
@pytest.mark.parametrize("R", [8, 4])
@pytest.mark.parametrize("name", ["n20_deep4", "n270"])
def test_forced_narrow_tiles_are_bit_exact(name, R, B):
    """B < R and B = R (the rows kernel: at most two samples per CU), 513 and 530 (the tile kernel, last tiles of one and
    two rows) against the oracle and against the 16-row model"""
    _need_256_cus()
    spec, models, ctx, y, E, g = _forced(name)
    B = {"lt": 3, "eq": R}.get(B, B)
    assert models[R].tile_rows == R and models[16].tile_rows == 16
    f_n, g_n = _fg(models[R], ctx[:B].contiguous(), y[:B])
    f_16, g_16 = _fg(models[16], ctx[:B].contiguous(), y[:B])
    assert np.array_equal(f_n, E[:B]), "E: %s" % _first_difference(f_n, E[:B])
    assert np.array_equal(g_n, g[:B]), "dE/dy: %s" % _first_difference(g_n, g[:B])
    assert np.array_equal(f_n, f_16) and np.array_equal(g_n, g_16)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [8, 4])
def test_finished_rows_keep_their_f_and_g(R):
    """tile 1 finished as a whole, tile 2 half finished.  The kernel skips TILES -- a workgroup whose samples have all left the
    loop returns before its first barrier --, as the 16-row tile does: the rows of tile 1 keep what was there, and a tile with
    a live sample is evaluated as a whole, its finished rows included (their f and g are the oracle's; no caller reads them)."""
    _need_256_cus()
    spec, models, ctx, y, E, g = _forced("n270")
    B, n = 530, spec.n_labels
    fin = np.zeros(B, np.int32)
    fin[R:2 * R] = 1
    fin[2 * R:2 * R + R // 2] = 1
    f = torch.full((B,), 123.0, dtype=torch.float32, device="cuda")
    gd_ = torch.full((B, n), -7.0, dtype=torch.float32, device="cuda")
    yd, find = torch.from_numpy(y).cuda(), torch.from_numpy(fin).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().icnn_be_fc_fg(C.byref(models[R].c_model), ctx.data_ptr(), yd.data_ptr(), B, f.data_ptr(), gd_.data_ptr(),
                                         find.data_ptr(), C.c_void_p(stream)), "icnn_be_fc_fg")
    torch.cuda.synchronize()
    f, gd_ = f.cpu().numpy(), gd_.cpu().numpy()
    skip = np.zeros(B, bool)
    skip[R:2 * R] = True
    assert (fin != 0).sum() == R + R // 2
    assert (f[skip] == 123.0).all() and (gd_[skip] == -7.0).all()
    assert np.array_equal(f[~skip], E[~skip]) and np.array_equal(gd_[~skip], g[~skip])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [100, 530])
def test_bibtex_600_600_is_bit_exact(B):
    """B = 100: the rows kernel; B = 530: tiles of 8 rows, the last one holding two"""
    _need_256_cus()
    spec, params, model, ctx = _real("bib2", B)
    assert model.tile_rows == 8
    y = np.random.RandomState(B).rand(B, spec.n_labels)
    E, g = picnn_oracle.energy_and_grad_chain(params, ctx.cpu().numpy(), y, list(spec.szs), spec.alpha)
    f_d, g_d = _fg(model, ctx, y)
    assert np.array_equal(f_d, np.asarray(E, np.float32)), "E: %s" % _first_difference(f_d, np.asarray(E, np.float32))
    assert np.array_equal(g_d, np.asarray(g, np.float32)), "dE/dy: %s" % _first_difference(g_d, np.asarray(g, np.float32))
    assert np.isfinite(f_d).all() and float(np.abs(g_d).max()) > 0


@pytest.mark.gpu
def test_delicious_600_is_bit_exact():
    """B = 515: tiles of 4 rows, the last one holding three (983 labels: 62 tiles of dE/dy, every unit at home).  The oracle on
    the first 20 and the last 7 rows; every row against the same model in slices of 256 rows, i.e. on the rows kernel."""
    _need_256_cus()
    B = 515
    spec, params, model, ctx = _real("deli", B)
    assert model.tile_rows == 4
    y = np.random.RandomState(5).rand(B, spec.n_labels)
    f_d, g_d = _fg(model, ctx, y)
    flat = ctx.cpu().numpy()
    for rows in (slice(0, 20), slice(B - 7, B)):
        E, g = picnn_oracle.energy_and_grad_chain(params, flat[rows], y[rows], list(spec.szs), spec.alpha)
        assert np.array_equal(f_d[rows], np.asarray(E, np.float32)) and np.array_equal(g_d[rows], np.asarray(g, np.float32)), rows
    for lo in range(0, B, 256):
        f_s, g_s = _fg(model, ctx[lo:lo + 256].contiguous(), y[lo:lo + 256])
        assert np.array_equal(f_s, f_d[lo:lo + 256]) and np.array_equal(g_s, g_d[lo:lo + 256]), lo
    assert np.isfinite(f_d).all() and float(np.abs(g_d).max()) > 0


# ------------------------------------------------------------------------------------------------ GPU: solve


def _solve(model, ctx, B, n_iter, variant, flags):
    from icnn_amd import bundle_entropy
    res = bundle_entropy.FusedSolver(model, B, n_iter, variant, flags=flags).solve(ctx, 0.5)
    return _all_outputs(res, B), _planned(model, res)


def _assert_same_outputs(a, b, what):
    for name, x, y in zip(OUTPUTS, a, b):
        assert np.array_equal(x, y), "%s differs (%s): %s" % (name, what, _first_difference(x, y))


@pytest.mark.gpu
@pytest.mark.parametrize("B,n_iter,path", [(40, 10, "ROWS"), (1100, 5, "ROUNDS_LOCKSTEP")])
def test_bibtex_600_600_solve_equals_launch_pairs(B, n_iter, path):
    _need_256_cus()
    spec, params, model, ctx = _real("bib2", B)
    default, plan = _solve(model, ctx, B, n_iter, "dual", 0)
    pairs, plan2 = _solve(model, ctx, B, n_iter, "dual", TWO)
    print("bibtex 600 600 B=%d nIter=%d: plan %s against %s; cuts held %s, most Newton updates %d"
          % (B, n_iter, plan, plan2, np.bincount(default[3]), default[5].max()))
    assert plan[0] == path and plan2[0].startswith("ROUNDS")
    _assert_same_outputs(default, pairs, plan2[0])
    assert default[5].max() > 1 and (default[10] == 0).all()


# The oracle comparison keeps |dE/dy| at O(1), as test_fc_solve_architectures.TAME does for its deep networks: at the "spread"
# scale the gradients of the three-layer network reach 300, y saturates, and the float64 reference's projected Newton solve
# runs into its 100-update cap on every seed (none of forty passed the screen).  The bit-exact tests use the unscaled models.
TAME_BIB2 = (0.2, 0.3)


@functools.lru_cache(maxsize=None)
def _screened_bib2(B=40, n_iter=10):
    """The first seed on which the oracle alone (host context) is clean and runs no Newton solve into its cap
    (test_fc_solve_architectures._screened_problem)."""
    for seed in range(1, 41):
        params, x = _sparse_problem(BIB2, B, seed, TAME_BIB2)
        host_ctx = picnn.context(BIB2, params, torch.from_numpy(x)).numpy()
        ora, clean, most = _oracle_run(BIB2, params, host_ctx, n_iter, "dual")
        if clean and most < oracle.VARIANTS["dual"].newton_cap:
            return seed, params, x
    raise AssertionError("no screened seed")


def test_a_screened_seed_exists_for_the_oracle_comparison():
    seed, params, x = _screened_bib2()
    assert x.shape == (40, 1836)


@pytest.mark.gpu
def test_bibtex_600_600_solve_matches_chain_order_oracle():
    """test_fused_solve_matches_chain_order_oracle at this architecture: identical active sets and nIters, status 0 on both
    sides, max|dy| <= 1e-7"""
    from icnn_amd import bundle_entropy
    _need_256_cus()
    B, n_iter = 40, 10
    seed, params, x = _screened_bib2()
    model = picnn.FCModel(BIB2, params)
    ctx = model.context(torch.from_numpy(x))
    res = bundle_entropy.solveBatch(f=model, ctx=ctx, y0=np.full((B, BIB2.n_labels), 0.5), nIter=n_iter, variant="dual",
                                    native=True, check=False)
    plan = _planned(model, res)
    ora, clean, most = _oracle_run(BIB2, params, ctx.cpu().numpy(), n_iter, "dual")
    host = result_to_host(res)
    assert ora is not None
    dy, discrete = compare_with_oracle(host, ora)
    print("bibtex 600 600 seed %d, plan %s: max|dy| = %.3e (bound 1e-7), %d discrete differences, most updates of one inner "
          "solve: oracle %d" % (seed, plan, dy.max(), len(discrete), most))
    assert plan[:2] == ("ROWS", 1)
    assert clean and most < oracle.VARIANTS["dual"].newton_cap and (host["status"] == 0).all()
    assert not discrete, "samples with different active sets / nIters: %s" % discrete[:8]
    assert dy.max() <= 1e-7, dy.max()


@pytest.mark.gpu
@pytest.mark.parametrize("R", [8, 4])
def test_forced_narrow_solve_equals_the_16_row_solve(R):
    """bibtex_spec() at B = 1100, nIter 5: the 16-row model runs the persistent tiles (the fixed-shape instance), the narrow one
    launch pairs of the narrow fc_fg_kernel and the dual step"""
    _need_256_cus()
    B, n_iter = 1100, 5
    spec, params, wide, ctx = _real("bib", B)
    narrow = picnn.FCModel(_with_rows(spec, R), params)
    a, plan_a = _solve(wide, ctx, B, n_iter, "dual", 0)
    b, plan_b = _solve(narrow, ctx, B, n_iter, "dual", 0)
    print("bibtex B=%d nIter=%d: %s (16 rows) against %s (%d rows)" % (B, n_iter, plan_a, plan_b, R))
    assert plan_a[0] == "TILE" and plan_b[0] == "ROUNDS_LOCKSTEP"
    _assert_same_outputs(a, b, "tile_rows %d against 16" % R)
    assert a[5].max() > 1


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["dual", "pdipm"])
def test_delicious_600_solve_equals_launch_pairs(variant):
    _need_256_cus()
    B, n_iter = 9, 5
    spec, params, model, ctx = _real("deli", B)
    default, plan = _solve(model, ctx, B, n_iter, variant, 0)
    pairs, plan2 = _solve(model, ctx, B, n_iter, variant, TWO)
    print("delicious 600 B=%d nIter=%d %s: plan %s against %s; cuts held %s" % (B, n_iter, variant, plan, plan2, np.bincount(default[3])))
    assert plan[:2] == ("ROWS", 1) and plan2[0].startswith("ROUNDS")
    _assert_same_outputs(default, pairs, plan2[0])
    assert np.isfinite(default[0]).all() and default[3].max() > 1


# ------------------------------------------------------------------------------------------------ GPU: gd / pgd


@pytest.mark.gpu
@pytest.mark.parametrize("B", [40, 530])
def test_gd_on_bibtex_600_600_is_bit_exact(B):
    """gd.solve, K = 3, against the float32 recurrence around the kernel-order oracle: 40 takes gd_rows_kernel, 530
    gd_fc_kernel on tiles of 8 rows (the last one holds two)"""
    from icnn_amd import gd
    _need_256_cus()
    spec, params, model, ctx = _real("bib2", B)
    flat = ctx.cpu().numpy()
    y0 = np.random.RandomState(32).rand(B, spec.n_labels)
    K, lr, mu = 3, 0.01, 0.3

    def fg(yy):
        return picnn_oracle.energy_and_grad_chain(params, flat, yy, list(spec.szs), spec.alpha)
    y_ref, traj_ref, E_ref = gd_ref.unroll_f32(fg, y0, K, lr, mu)
    y, traj, E = gd.solve(model, ctx, torch.from_numpy(y0).cuda(), K, lr, mu, trajectory=True, energy=True)
    torch.cuda.synchronize()
    assert np.array_equal(traj.cpu().numpy(), traj_ref), "trajectory: %s" % _first_difference(traj.cpu().numpy(), traj_ref)
    assert np.array_equal(y.cpu().numpy(), y_ref.astype(np.float64)), "y_K: %s" % _first_difference(y.cpu().numpy(), y_ref)
    assert np.array_equal(E.cpu().numpy(), E_ref)
    assert float(np.abs(y_ref - y0.astype(np.float32)).max()) > 1e-4


def _pgd(model, ctx, y0, K=4, lr=0.1):
    from icnn_amd import pgd
    out = pgd.solve(model, ctx.contiguous(), y0, K, lr, final=True)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


@pytest.mark.gpu
def test_pgd_on_bibtex_600_600_tiles_equal_rows():
    """pgd.solve at B = 530 (pgd_fc_kernel on tiles of 8 rows) against the same samples at B = 40 and in slices of 256
    (pgd_rows_kernel), bit for bit in y, e_k and e_K (module docstring)"""
    _need_256_cus()
    B = 530
    spec, params, model, ctx = _real("bib2", B)
    y0 = torch.from_numpy(np.random.RandomState(33).rand(B, spec.n_labels) * 1.2 - 0.1).cuda()
    y, obj, fin = _pgd(model, ctx, y0)
    assert np.isfinite(y).all() and np.isfinite(obj).all() and np.isfinite(fin).all() and obj.shape == (4, B)
    for lo, hi in ((0, 40), (0, 256), (256, 512), (512, 530)):
        ys, objs, fins = _pgd(model, ctx[lo:hi], y0[lo:hi])
        assert np.array_equal(ys, y[lo:hi]) and np.array_equal(objs, obj[:, lo:hi]) and np.array_equal(fins, fin[lo:hi]), (lo, hi)
    assert float(np.abs(y - np.clip(y0.cpu().numpy(), 1e-6, 1 - 1e-6)).max()) > 1e-4


@pytest.mark.gpu
def test_gd_and_pgd_forced_4_rows_equal_16_rows():
    """bibtex_spec() at B = 530: gd_fc_kernel and pgd_fc_kernel on tiles of 4 rows against tiles of 16"""
    from icnn_amd import gd
    _need_256_cus()
    B = 530
    spec, params, wide, ctx = _real("bib", B)
    narrow = picnn.FCModel(_with_rows(spec, 4), params)
    y0 = torch.from_numpy(np.random.RandomState(34).rand(B, spec.n_labels)).cuda()
    outs = []
    for model in (wide, narrow):
        y, traj, E = gd.solve(model, ctx, y0, 4, 0.01, 0.3, trajectory=True, energy=True)
        torch.cuda.synchronize()
        outs.append([y.cpu().numpy(), traj.cpu().numpy(), E.cpu().numpy()] + _pgd(model, ctx, y0))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert float(np.abs(outs[0][0] - y0.cpu().numpy()).max()) > 1e-4


# ------------------------------------------------------------------------------------------------ GPU: context, training


@functools.lru_cache(maxsize=None)
def _delicious_context_problem(B=9):
    """seeded model and x at the delicious shape, screened as test_fc_solve_architectures._context_problem screens: no
    normalised channel with a batch variance below 1e-4"""
    for seed in range(11, 211):
        params, x = _problem(DELI, B, seed, x_scale=3.0)
        ref64, stats = bn_ref.fc_context64(DELI, params, x)
        if min([float(var.min()) for _, var in stats.values()] + [np.inf]) < 1e-4:
            continue
        ref = picnn_oracle.flat_context(picnn_oracle.context(params, x, list(DELI.szs), DELI.batchnorm, dtype=np.float64),
                                        dtype=np.float64)
        return seed, params, x, ref
    raise AssertionError("no screened seed")


def test_the_delicious_context_problem_is_screened():
    assert picnn.bn_layers(DELI) and DELI.n_features == 500
    seed, params, x, ref = _delicious_context_problem()
    assert ref.shape == (9, DELI.ctx_width) and ref.dtype == np.float64


@pytest.mark.gpu
def test_context_at_the_delicious_shape_matches_float64():
    seed, params, x, ref = _delicious_context_problem()
    model = picnn.FCModel(DELI, params)
    ctx = model.context(torch.from_numpy(x)).cpu().numpy()
    err, scale = float(np.max(np.abs(ctx - ref))), float(np.abs(ref).max())
    print("delicious B=9 seed %d: max|ctx - ref| = %.2e, bound 2e-5 * %.2e" % (seed, err, scale))
    assert ctx.shape == ref.shape and err <= 2e-5 * scale


@functools.lru_cache(maxsize=None)
def _small_feed_bib2():
    """tests/test_train_grad.py::_small_problem at this architecture: 6 samples with 1-4 rows each, screened there"""
    import test_train_grad
    return test_train_grad._small_problem(BIB2, 0, True)


def test_a_screened_small_feed_exists():
    p = _small_feed_bib2()
    assert len(p["samp"]) >= 6 and set(p["g64"]) == set(picnn.init_params(BIB2).keys())


@pytest.mark.gpu
def test_surrogate_grad_on_bibtex_600_600_against_float64():
    """test_train_grad.py::test_small_every_variable_matches_float64_double_backward on bibtex 600 600: every variable within
    1e-4 of its scale (+ 1e-7) of the float64 double backward, F within 1e-5"""
    from icnn_amd import bundle_entropy, train
    p = _small_feed_bib2()
    model = picnn.FCModel(BIB2, p["params"], "cuda")
    assert model.tile_rows == 8
    dev = model.device
    y, v, c = (torch.from_numpy(p[k]).to(dev) for k in ("y", "v", "c"))
    F = torch.empty(len(p["samp"]), dtype=torch.float32, device=dev)
    feed = bundle_entropy.ImplicitFeed(torch.from_numpy(p["samp"].astype(np.int32)).to(dev), y, v, c)
    g = train.surrogate_grad(model, torch.from_numpy(p["x"]), feed, F_rows=F)
    torch.cuda.synchronize()
    worst = []
    for k, ref in p["g64"].items():
        got = g[k].double().cpu().numpy()
        assert got.shape == ref.shape, k
        err, scale = float(np.max(np.abs(got - ref))), float(np.max(np.abs(ref)))
        worst.append((err / max(scale, 1e-30), k))
        assert err <= 1e-4 * scale + 1e-7, (k, err, scale)
    assert np.max(np.abs(F.double().cpu().numpy() - p["F64"])) <= 1e-5 * np.max(np.abs(p["F64"]))
    print("bibtex 600 600, %d rows: worst relative error %.2e (%s)" % ((len(p["samp"]),) + max(worst)))


def _trainer_step(kind, model, x, labels):
    from icnn_amd import train
    B = x.shape[0]
    if kind == "bundle":
        tr = train.BundleTrainer(model, B, n_iter=5, loss="xent", variant="pdipm")
        tr.step(torch.from_numpy(x).cuda(), torch.from_numpy(labels.astype(np.float64)).cuda())
    else:
        tr = train.GDTrainer(model, B, n_iter=3, lr=0.01, momentum=0.3)
        tr.step(torch.from_numpy(x).cuda(), torch.from_numpy(labels.astype(np.float32)).cuda())
    torch.cuda.synchronize()
    return tr


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bundle", "gd"])
def test_a_training_step_does_not_depend_on_the_tile_rows(kind):
    """one BundleTrainer / GDTrainer step on bibtex_spec() at B = 528: the parameters after it, 8 rows against 16"""
    _need_256_cus()
    B = 528
    spec = picnn.bibtex_spec()
    params, x = _sparse_problem(spec, B, 0)
    labels = np.random.RandomState(1).rand(B, spec.n_labels) < 0.05
    thetas = []
    for R in (16, 8):
        model = picnn.FCModel(_with_rows(spec, R), {k: v.copy() for k, v in params.items()})
        tr = _trainer_step(kind, model, x, labels)
        assert model.tile_rows == R
        thetas.append((tr.opt.theta.cpu().numpy(), tr.grad.cpu().numpy()))
        del tr
    assert np.array_equal(thetas[0][0], thetas[1][0]) and np.array_equal(thetas[0][1], thetas[1][1])
    assert np.isfinite(thetas[0][0]).all() and float(np.abs(thetas[0][1]).max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["bundle", "gd"])
def test_a_training_step_on_delicious_600(kind):
    B = 16
    params, x = _sparse_problem(DELI, B, 2)
    labels = np.random.RandomState(3).rand(B, DELI.n_labels) < 0.02
    model = picnn.FCModel(DELI, params)
    tr = _trainer_step(kind, model, x, labels)
    theta = tr.opt.theta.cpu().numpy()
    assert model.tile_rows == 4
    assert np.isfinite(theta).all() and np.isfinite(tr.grad.cpu().numpy()).all() and np.isfinite(float(tr.loss.item()))
    assert float(tr.grad.abs().max()) > 0
