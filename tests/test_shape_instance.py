"""The instances of the persistent tile kernel compiled for the Bibsonomy network's shape (be_fused.hip, FixedShape): which
launches take them (icnn_be_debug_shape_instance: the launcher's own choice), and that they compute, bit for bit, what the
generic kernel computes (ICNN_BE_FLAG_GENERIC_SHAPE) -- same operations in the same order, only the shape is a constant.

The launcher takes a fixed instance only where every constant of its policy equals what fill_args, pack_offsets and
make_dual_args produce for the model and state at hand (shape_matches, be_fused.hip), so a non-zero answer of the query is
also the check that the policy's derivation and the launcher's agree.

Batches of 16, 17 and 40 samples get 4-row tiles on a device of more than ten CUs (tests/test_solve_plan.py): 4, 5 and 10
workgroups, the last one of B = 17 with a single real row.  8- and 16-row tiles are reached by batches of 8 and 8 + samples
per CU; the 16-row case ends in a ragged tile of three rows."""
import ctypes as C

import numpy as np
import pytest
import torch

from icnn_amd import _lib, picnn

PERS, TWO, GENERIC = _lib.FLAG_PERSISTENT, _lib.FLAG_TWO_KERNELS, _lib.FLAG_GENERIC_SHAPE
BIB = picnn.bibtex_spec()
N158 = picnn.FCSpec(BIB.n_features, 158, BIB.szs)                       # the same net with n = 158
W160 = picnn.FCSpec(BIB.n_features, BIB.n_labels, (BIB.szs[0], 160))    # ... with widths 600 / 160 / 1
FIELDS = ("y", "G", "ys", "h", "lam", "active", "count", "n_iters", "newton_iters", "status")


# ---- host arithmetic: no GPU, no buffers (the descriptors of tests/test_solve_plan.py) ------------------------------------

def fc_model(spec):
    m = _lib.FcModel()
    m.n, m.n_layers = spec.n_labels, spec.n_layers
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    m.alpha, m.action_box, m.ctx_width = float(spec.alpha), int(spec.action_box), spec.ctx_width
    return m


def fc_state(spec, B, n_iter, variant, flags=0, cut=_lib.CUT_F32):
    s = _lib.State()
    slots = min(n_iter, _lib.MAX_SLOTS)
    s.batch, s.n, s.slots = B, spec.n_labels, slots
    s.iters = n_iter if n_iter > slots else 0
    s.variant, s.flags, s.cut_dtype = _lib.VARIANT[variant], flags, cut
    return s


def instance(spec, B, n_iter, variant="dual", flags=0, cut=_lib.CUT_F32):
    return _lib.shape_instance(fc_model(spec), fc_state(spec, B, n_iter, variant, flags, cut))


def test_only_the_bibsonomy_net_has_an_instance():
    assert instance(BIB, 4096, 10) == "bibtex_kt16"
    assert instance(picnn.halfcheetah_spec(), 4096, 10) == "generic"
    assert instance(picnn.halfcheetah_spec(), 4096, 5, "rl", PERS) == "generic"
    assert instance(picnn.synthetic_spec(), 4096, 10) == "generic"


def test_instance_follows_tile_rows_slots_and_layout():
    """tile_rows is a run-time argument of the instances; the layout decision is not"""
    assert [instance(BIB, B, 10) for B in (1025, 2048, 2051, 8192)] == ["bibtex_kt16"] * 4       # 8-, 8-, 16-, 16-row tiles
    assert [instance(BIB, B, 10, flags=PERS) for B in (16, 17, 40)] == ["bibtex_kt16"] * 3      # 4-row tiles
    assert instance(BIB, 4096, 5) == instance(BIB, 4096, 3) == "bibtex_kt16"
    assert instance(BIB, 4096, 30) == instance(BIB, 40, 17, flags=PERS) == "bibtex_kt32_grouped"
    # 11..15 slots: the 16-slot kernel with the dual phase in groups -- no instance was compiled for that pair
    assert instance(BIB, 1100, 12, flags=PERS) == "generic"
    # not the tile kernel at all: per-sample kernel, launch pairs
    assert instance(BIB, 128, 10) == instance(BIB, 4096, 10, flags=TWO) == instance(BIB, 8193, 10) == "generic"


def test_near_misses_and_the_flag_stay_generic():
    assert instance(BIB, 4096, 10, flags=GENERIC) == instance(BIB, 4096, 30, flags=GENERIC) == "generic"
    assert instance(N158, 4096, 10) == instance(W160, 4096, 10) == "generic"
    assert instance(picnn.FCSpec(BIB.n_features, BIB.n_labels, (BIB.szs[0],)), 4096, 10) == "generic"      # one layer fewer
    assert instance(BIB, 4096, 10, "pdipm") == instance(BIB, 4096, 10, "rl", PERS) == "generic"
    assert instance(BIB, 4096, 10, flags=PERS | _lib.FLAG_TIME_SLICE) == "generic"                          # an update budget
    assert instance(BIB, 4096, 10, cut=_lib.CUT_F64) == "generic"


def test_query_validates_like_the_plan():
    lib = _lib.load()
    m, s = fc_model(BIB), fc_state(BIB, 4096, 10, "dual")
    assert lib.icnn_be_debug_shape_instance(C.byref(m), C.byref(s)) == 1
    assert lib.icnn_be_debug_shape_instance(None, C.byref(s)) == -1
    assert lib.icnn_be_debug_shape_instance(C.byref(m), None) == -1
    s.batch = 0
    assert lib.icnn_be_debug_shape_instance(C.byref(m), C.byref(s)) == -1
    s.batch, s.n = 4096, 158
    assert lib.icnn_be_debug_shape_instance(C.byref(m), C.byref(s)) == -1       # state and model disagree on n
    s.n, m.ctx_width = 159, 7
    assert lib.icnn_be_debug_shape_instance(C.byref(m), C.byref(s)) == -1       # model rejected


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def nets():
    """spec name -> (model, context rows); built once, never written by a test"""
    made = {}

    def get(name, rows):
        spec = {"bib": BIB, "n158": N158, "w160": W160}[name]
        if name not in made or made[name][1].shape[0] < rows:
            model = picnn.FCModel(spec, picnn.init_params(spec, 0, "spread"))
            x = (np.random.RandomState(1000).rand(rows, spec.n_features) < 0.04).astype(np.float32)
            made[name] = (model, model.context(torch.from_numpy(x)))
        return made[name]
    return get


def run(model, ctx_all, B, n_iter, variant, flags, start):
    """one fused solve; (instance name, plan, the result tensors as clones)"""
    from icnn_amd import bundle_entropy
    ctx = ctx_all[:B].contiguous()
    y0 = 0.5
    if start == "tensor":
        y0 = torch.from_numpy(0.1 + 0.8 * np.random.RandomState(5).rand(B, model.spec.n_labels))
    fs = bundle_entropy.FusedSolver(model, B, n_iter, variant, flags=flags)
    res = fs.solve(ctx, y0)
    torch.cuda.synchronize()
    st = res.state
    out = {"y": res.y, "G": st.G, "ys": st.ys, "h": st.h, "lam": res.lam, "active": res.active, "count": res.count[:B],
           "n_iters": res.n_iters[:B], "newton_iters": res.newton_iters[:B], "status": res.status[:B]}
    return (_lib.shape_instance(model.c_model, st.c_state), _lib.solve_plan(model.c_model, st.c_state),
            {k: v.clone() for k, v in out.items()})


def assert_same(a, b):
    for k in FIELDS:
        assert torch.equal(a[k], b[k]), k
    assert int(a["count"].max()) >= 1


SMALL = [(B, T, start) for B in (16, 17, 40) for T in (3, 10) for start in ("scalar", "tensor")]


@pytest.mark.gpu
@pytest.mark.parametrize("B,n_iter,start", SMALL, ids=["%d_%d_%s" % c for c in SMALL])
def test_fixed_instance_equals_generic_kernel(nets, B, n_iter, start):
    model, ctx = nets("bib", 64)
    fixed, generic = (run(model, ctx, B, n_iter, "dual", PERS | f, start) for f in (0, GENERIC))
    assert (fixed[0], generic[0]) == ("bibtex_kt16", "generic")
    assert fixed[1] == generic[1] and fixed[1][0] == "TILE"
    assert_same(fixed[2], generic[2])
    if n_iter == 10:
        assert int(fixed[2]["count"].max()) >= 2, "a bundle of one cut never enters the Newton loop"


@pytest.mark.gpu
@pytest.mark.parametrize("rows,extra,start", [(8, 0, "scalar"), (8, 0, "tensor"), (8, 3, "tensor")], ids=["8_rows", "8_rows_y0", "16_rows_ragged"])
def test_fixed_instance_equals_generic_kernel_on_wider_tiles(nets, rows, extra, start):
    """default dispatch: eight samples per CU are 8-row tiles (2048 on 256 CUs), three more 16-row tiles whose last holds 3"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = rows * cus + extra
    model, ctx = nets("bib", B)
    fixed, generic = (run(model, ctx, B, 10, "dual", f, start) for f in (0, GENERIC))
    assert (fixed[0], generic[0]) == ("bibtex_kt16", "generic")
    assert fixed[1] == generic[1] == ("TILE", 16 if extra else 8, 0, 10)
    assert_same(fixed[2], generic[2])


@pytest.mark.gpu
@pytest.mark.parametrize("n_iter,start", [(17, "scalar"), (24, "tensor")])
def test_grouped_fixed_instance_equals_generic_kernel(nets, n_iter, start):
    """more than 15 slots: the 32-slot instance, the dual phase in groups"""
    model, ctx = nets("bib", 64)
    fixed, generic = (run(model, ctx, 40, n_iter, "dual", PERS | f, start) for f in (0, GENERIC))
    assert (fixed[0], generic[0]) == ("bibtex_kt32_grouped", "generic")
    assert fixed[1] == generic[1] and fixed[1][0] == "TILE"
    assert_same(fixed[2], generic[2])


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", [("n158", "dual"), ("w160", "dual"), ("bib", "pdipm")])
def test_near_misses_run_the_generic_kernel(nets, name, variant):
    model, ctx = nets(name, 64)
    tile, pairs = (run(model, ctx, 40, 5, variant, f, "scalar") for f in (PERS, TWO))
    assert tile[0] == pairs[0] == "generic"
    assert tile[1][0] == "TILE" and pairs[1][0] != "TILE"
    assert_same(tile[2], pairs[2])


@pytest.mark.gpu
def test_float64_cuts_have_no_fused_solve_and_no_instance(nets):
    """icnn_be_solve_fc takes float32 cuts only (its energies are float32): with a float64 cut dtype the query answers
    generic and the solve is refused alike whatever the dispatch flags -- there is nothing the two could differ in"""
    from icnn_amd import bundle_entropy
    model, ctx_all = nets("bib", 64)
    ctx = ctx_all[:40].contiguous()
    for flags in (PERS, TWO):
        fs = bundle_entropy.FusedSolver(model, 40, 5, "dual", flags=flags)
        st = fs.state
        st.c_state.cut_dtype = _lib.CUT_F64
        assert _lib.shape_instance(model.c_model, st.c_state) == "generic"
        rc = st.lib.icnn_be_solve_fc_reset(C.byref(model.c_model), ctx.data_ptr(), C.byref(st.c_state), fs.f_work.data_ptr(),
                                           fs.g_work.data_ptr(), None, 0.5, st.stream())
        assert rc == -1
