"""icnn_be_solve_fc_reset: the reset of a solve inside its first launch.

The entry must equal, bit for bit, the three calls it replaces -- `st->y <- y0; icnn_be_state_init; icnn_be_solve_fc` -- on
every plan, and it must do so on a DIRTY state: before every comparison the solver runs once on another context from another
start point, and its control words are then overwritten with values that would stop a kernel which did not reset them
(finished = skip_fg = 1, t_next = nIter, phase = 1, status = 7, a count, Newton and iteration counters).  The reference is a
fresh BundleState driven through fill_/copy_ + icnn_be_state_init + icnn_be_solve_fc.

What is compared: y, count, n_iters, newton_iters, status, finished whole; `active` over its first count[u] entries, and lam, h,
G, ys over the active slots in the bundle's order (bench.py's outputs()).  Neither path resets the slot arrays or the tail of
`active` behind count[u] (icnn_be_state_init does not either), so a reused state keeps its earlier solve's values there and
only a fresh one holds zeros.

Batches.  With one sample per CU up to 256 samples, B = 1, 3, 5 all run the per-sample kernel at ONE sample per workgroup; two
and four samples per workgroup with a ragged last workgroup are B = 257 and B = 770, added here (for variant rl that is the
narrow-row phase whose wave 0 reads the control words the other waves reset).  B = 2050 is the 16-row tile kernel with a
two-row last tile, the headline's instance.

Last in the file: phase A's tile loops (gemm_tiles, be_picnn_fc_dev.h) at operands of one, two and five real k-blocks --
widths 16, 30, 70 -- in one and three hidden layers, bit for bit against oracle/picnn_chain.c."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from icnn_amd import _lib, picnn
from oracle import picnn_oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERS, SLICE, TWO = _lib.FLAG_PERSISTENT, _lib.FLAG_TIME_SLICE, _lib.FLAG_TWO_KERNELS
ENTRY = "icnn_be_solve_fc_reset"


# ------------------------------------------------------------------------------------------------ CPU


def test_entry_is_declared_listed_and_exported():
    from icnn_amd import build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    assert re.search(r"ICNN_BE_API\s+int\s+%s\s*\(" % ENTRY, header)
    assert ENTRY in _lib.EXPORTS and hasattr(lib, ENTRY)
    assert lib.icnn_be_abi_version() == 12                  # additive: the ABI number stays
    assert lib.icnn_be_solve_fc_reset.argtypes[:6] == lib.icnn_be_solve_fc.argtypes[:5] + [C.c_void_p]
    assert lib.icnn_be_solve_fc_reset.argtypes[6:] == [C.c_double, C.c_void_p]


def _host_descriptors(batch, cut_dtype=_lib.CUT_F32):
    """a Bibsonomy-shaped model and a state whose buffers are non-null: enough for every check made before a launch"""
    m = _lib.FcModel()
    m.n, m.n_layers = 159, 3
    m.width[0], m.width[1], m.width[2] = 600, 159, 1
    m.ctx_width = picnn.bibtex_spec().ctx_width
    m.wpack = 64
    st = _lib.State()
    st.batch, st.n, st.slots, st.cut_dtype, st.variant = batch, 159, 10, cut_dtype, 0
    for name, _ in _lib.State._fields_[6:22]:
        setattr(st, name, 64)
    return m, st


def test_invalid_arguments_get_the_codes_of_solve_fc():
    lib = _lib.load()
    fake = C.c_void_p(64)

    def both(model, ctx, st, f_work=fake, g_work=fake):
        old = lib.icnn_be_solve_fc(model, ctx, st, f_work, g_work, None)
        new = [lib.icnn_be_solve_fc_reset(model, ctx, st, f_work, g_work, y0, 0.5, None) for y0 in (None, fake)]
        assert new == [old, old], (old, new)
        return old

    m, st = _host_descriptors(4)
    assert both(C.byref(m), fake, None) == -1                               # null state
    assert both(None, fake, C.byref(st)) == -1                              # null model
    assert both(C.byref(m), None, C.byref(st)) == -1                        # null context
    assert both(C.byref(m), fake, C.byref(st), g_work=None) == -1           # null work array
    m64, st64 = _host_descriptors(4, _lib.CUT_F64)
    assert both(C.byref(m64), fake, C.byref(st64)) == -1                    # float64 cuts
    st.flags = _lib.FLAG_F64_ENERGY
    assert both(C.byref(m), fake, C.byref(st)) == -1                        # float64 energies
    st.flags, st.n = 0, 158
    assert both(C.byref(m), fake, C.byref(st)) == -1                        # state and model disagree on n
    st.n, st.slots = 159, 40
    assert both(C.byref(m), fake, C.byref(st)) == -2                        # more slots than ICNN_BE_MAX_SLOTS
    st.slots, st.count = 10, None
    assert both(C.byref(m), fake, C.byref(st)) == -1                        # a null buffer
    m0, st0 = _host_descriptors(0)
    assert both(C.byref(m0), fake, C.byref(st0)) == 0                       # empty batch: nothing enqueued


# ------------------------------------------------------------------------------------------------ GPU: the reset


SPECS = {"bib": picnn.bibtex_spec, "hc": picnn.halfcheetah_spec}


@functools.lru_cache(maxsize=None)
def _model(which):
    spec = SPECS[which]()
    kw = dict(yu_bias=1.0, gate_bias=1.0) if spec.action_box else {}
    return spec, picnn.FCModel(spec, picnn.init_params(spec, 3, "spread", **kw))


@functools.lru_cache(maxsize=None)
def _contexts(which, B):
    """(the context of the compared solve, another one for the solve that dirties the state)"""
    spec, model = _model(which)
    out = []
    for seed in (11, 12):
        rng = np.random.RandomState(seed)
        x = (rng.rand(B, spec.n_features) < 0.04) if spec.n_features > 100 else rng.randn(B, spec.n_features)
        out.append(model.context(torch.from_numpy(x.astype(np.float32))))
    return tuple(out)


def _start(kind, B, n, seed=21):
    if kind == "scalar":
        return 0.5
    return torch.from_numpy(0.2 + 0.6 * np.random.RandomState(seed).rand(B, n)).cuda()


def _outputs(st, B):
    """every compared array, the slot arrays gathered in the bundle's order and zero behind each sample's count"""
    h = {k: getattr(st, k)[:B].cpu().numpy() for k in ("y", "count", "n_iters", "newton_iters", "status", "finished", "active",
                                                       "lam", "h", "G", "ys")}
    cnt, T = h["count"].astype(np.int64), h["active"].shape[1]
    assert (cnt >= 0).all() and (cnt <= T).all()
    live = np.arange(T)[None, :] < cnt[:, None]
    slot = np.clip(np.where(live, h["active"], 0), 0, T - 1).astype(np.int64)
    out = {k: h[k] for k in ("y", "count", "n_iters", "newton_iters", "status", "finished")}
    out["active"] = np.where(live, h["active"], 0)
    out["lam"] = np.where(live, h["lam"], 0.0)                     # lam is stored in the bundle's order already
    out["h"] = np.where(live, np.take_along_axis(h["h"], slot, 1), 0.0)
    for k in ("G", "ys"):
        out[k] = np.where(live[:, :, None], np.take_along_axis(h[k], slot[:, :, None], 1), 0)
    return out


def _three_calls(model, ctx, B, n_iter, variant, flags, y0):
    """the path the entry replaces, on a fresh state"""
    from icnn_amd import bundle_entropy
    n = model.spec.n_labels
    y = torch.empty(B, n, dtype=torch.float64, device="cuda")
    st = bundle_entropy.BundleState(y, n_iter, variant, torch.float32, flags)
    if torch.is_tensor(y0):
        y.copy_(y0)
    else:
        y.fill_(y0)
    st.init()
    f_work = torch.empty(B, dtype=torch.float32, device="cuda")
    g_work = torch.empty(B, n, dtype=torch.float32, device="cuda")
    rounds = st.lib.icnn_be_solve_fc(C.byref(model.c_model), ctx.data_ptr(), C.byref(st.c_state), f_work.data_ptr(),
                                     g_work.data_ptr(), st.stream())
    assert rounds > 0, rounds
    torch.cuda.synchronize()
    return _outputs(st, B), rounds


def _dirty(solver, other_ctx):
    """one solve on other inputs, then control words that stop any kernel that does not reset them"""
    st, B = solver.state, solver.batch
    solver.solve(other_ctx, _start("tensor", B, st.n, seed=22))
    torch.cuda.synchronize()
    assert int(st.count[:B].max()) > 0 and int(st.t_next[:B].max()) > 0
    st.finished.fill_(1)
    st.skip_fg.fill_(1)
    st.t_next.fill_(st.n_iter)
    st.phase.fill_(1)
    st.status.fill_(7)
    st.count.fill_(min(st.T, 2))
    st.n_iters.fill_(-5)
    st.newton_iters.fill_(99)
    st.y.fill_(0.123)


def _assert_same(got, want, what):
    for k in want:
        assert np.array_equal(got[k], want[k]), "%s: %s differs on %d samples" % (
            what, k, int(np.asarray(got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1).sum()))


# (spec, variant, batch, nIter, flags, the plan's path at 256 CUs)
CASES = []
for _variant in ("dual", "pdipm"):
    CASES += [("bib", _variant, B, 3, 0, "ROWS") for B in (1, 3, 5)]
    CASES += [("bib", _variant, B, 3, PERS, "TILE") for B in (20, 33)]
    CASES += [("bib", _variant, 40, 18, PERS, "TILE"),                         # the grouped 32-slot instance
              ("bib", _variant, 20, 3, TWO, "ROUNDS_LOCKSTEP")]                # reset enqueued by the entry
CASES += [("bib", "dual", 33, 18, PERS | SLICE, "TILE_BUDGETED_THEN_ROWS"),     # budgeted tiles + the finishing launch
          ("bib", "dual", 257, 3, 0, "ROWS"), ("bib", "dual", 770, 3, 0, "ROWS"),       # 2 and 4 samples per workgroup, ragged
          ("bib", "pdipm", 770, 3, 0, "ROWS"),
          ("bib", "dual", 2050, 3, 0, "TILE"),                                  # sixteen rows per tile, two in the last
          ("bib", "dual", 5, 12, 0, "ROWS"), ("bib", "dual", 33, 12, PERS, "TILE")]
CASES += [("hc", "rl", B, n_iter, 0, "ROWS") for B in (3, 40) for n_iter in (3, 12)]    # narrow rows: the dual steps of a workgroup on wave 0
CASES += [("hc", "rl", 770, 3, 0, "ROWS"),                                      # four samples per wave, ragged last workgroup
          ("hc", "rl", 40, 3, PERS, "TILE"), ("hc", "rl", 40, 3, TWO, "ROUNDS_LOCKSTEP")]


def _case_id(c):
    return "%s-%s-B%d-T%d-f%d" % c[:5]


@pytest.mark.gpu
@pytest.mark.parametrize("start", ["scalar", "tensor"])
@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_reset_entry_on_a_dirty_state_equals_three_calls_on_a_fresh_one(case, start):
    from icnn_amd import bundle_entropy
    which, variant, B, n_iter, flags, path = case
    spec, model = _model(which)
    ctx, other = _contexts(which, B)
    y0 = _start(start, B, spec.n_labels)
    want, rounds = _three_calls(model, ctx, B, n_iter, variant, flags, y0)
    solver = bundle_entropy.FusedSolver(model, B, n_iter, variant, flags=flags)
    plan = _lib.solve_plan(model.c_model, solver.state.c_state)
    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    print("%s: plan %s on %d CUs, cuts held %s" % (_case_id(case), plan, cus, np.bincount(want["count"])))
    if cus == 256 or flags & (TWO | SLICE):
        assert plan[0] == path, plan
    _dirty(solver, other)
    res = solver.solve(ctx, y0)
    torch.cuda.synchronize()
    assert res.state.rounds == rounds == plan[3]
    _assert_same(_outputs(solver.state, B), want, "first solve on the dirty state")
    assert want["count"].max() > 0
    _dirty(solver, other)                                   # and again: the state the entry itself left behind
    solver.solve(ctx, y0)
    torch.cuda.synchronize()
    _assert_same(_outputs(solver.state, B), want, "second solve")


@pytest.mark.gpu
@pytest.mark.parametrize("case", [("bib", "dual", 33, 3, PERS), ("bib", "dual", 5, 3, 0), ("hc", "rl", 770, 3, 0),
                                  ("bib", "dual", 20, 3, TWO)], ids=["tile", "rows", "narrow_rows", "launch_pairs"])
@pytest.mark.parametrize("start", ["scalar", "tensor"])
def test_reset_entry_replays_from_a_graph_on_a_dirtied_state(case, start):
    """One solve captured, replayed twice with the state dirtied in front of each replay: both equal the eager result."""
    from icnn_amd import bundle_entropy
    which, variant, B, n_iter, flags = case
    spec, model = _model(which)
    ctx, other = _contexts(which, B)
    y0 = _start(start, B, spec.n_labels)
    solver = bundle_entropy.FusedSolver(model, B, n_iter, variant, flags=flags)
    solver.solve(ctx, y0)
    torch.cuda.synchronize()
    eager = _outputs(solver.state, B)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        solver.solve(ctx, y0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        solver.solve(ctx, y0)
    for replay in (1, 2):
        _dirty(solver, other)
        graph.replay()
        torch.cuda.synchronize()
        _assert_same(_outputs(solver.state, B), eager, "replay %d" % replay)


# ------------------------------------------------------------------------------------------------ GPU: phase A's unit starts


# every GEMM operand of these nets has 1 (K = 16), 2 (K = 30) or 5 (K = 70) real k-blocks: the tile loop's ring prologue alone,
# one turn of the loop, and two turns plus the odd k-block behind it
TILE_NETS = {"L1_n16_w70": (16, (70,)), "L1_n30_w16": (30, (16,)), "L1_n70_w30": (70, (30,)),
             "L3_n16": (16, (70, 30, 16)), "L3_n30": (30, (16, 70, 30)), "L3_n70": (70, (30, 16, 70))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TILE_NETS))
def test_tile_loops_at_one_two_and_five_k_blocks_equal_the_chain_oracle(name):
    from icnn_amd import bundle_entropy
    n, szs = TILE_NETS[name]
    spec = picnn.FCSpec(12, n, szs, alpha=0.01, batchnorm=False)
    params = picnn.init_params(spec, 5, "spread", yu_bias=1.0, gate_bias=1.0)
    model = picnn.FCModel(spec, params)
    for B in (20, 600):                                     # icnn_be_fc_fg: the per-sample kernel, and the 16-row MFMA tiles
        x = np.random.RandomState(8).randn(B, 12).astype(np.float32)
        ctx = model.context(torch.from_numpy(x))
        y = np.random.RandomState(9).rand(B, n)
        f, g = model.fg(ctx, torch.from_numpy(y).cuda())
        f_ref, g_ref = picnn_oracle.energy_and_grad_chain(params, ctx.cpu().numpy(), y, list(szs), spec.alpha, False)
        assert np.array_equal(f.cpu().numpy(), f_ref), (B, np.abs(f.cpu().numpy() - f_ref).max())
        assert np.array_equal(g.cpu().numpy(), g_ref), (B, np.abs(g.cpu().numpy() - g_ref).max())
    # the fused solve on the tile kernel (B = 20, four rows per tile): every cut it took is the chain's energy and gradient at
    # the point it was taken at
    B, n_iter = 20, 4
    x = np.random.RandomState(8).randn(B, 12).astype(np.float32)
    ctx = model.context(torch.from_numpy(x))
    solver = bundle_entropy.FusedSolver(model, B, n_iter, "dual", flags=PERS)
    assert _lib.solve_plan(model.c_model, solver.state.c_state)[0] == "TILE"
    st = solver.solve(ctx, 0.5).state
    torch.cuda.synchronize()
    t_next = st.t_next[:B].cpu().numpy()
    ys, G, fv = st.ys.cpu().numpy(), st.G.cpu().numpy(), st.fvals[:B].cpu().numpy()
    fg = picnn_oracle.make_fg_chain(params, ctx.cpu().numpy(), list(szs), spec.alpha, False)
    checked = 0
    for t in range(n_iter):
        f_ref, g_ref = fg(ys[:, t])
        took = t_next > t                                   # slot t holds the cut of iteration t of every sample that completed it
        assert took.any() or t > 0
        assert np.array_equal(G[took, t], g_ref[took]), (t, np.abs(G[took, t] - g_ref[took]).max())
        assert np.array_equal(fv[took, t], f_ref[took].astype(np.float64)), t
        checked += int(took.sum())
    assert checked > B
