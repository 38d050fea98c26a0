"""The deal of a tile evaluation (fc_deal, be_picnn_fc_dev.h; icnn_be_debug_fc_deal): the dE/dy GEMMs run an interval late on
the waves without a delta chain, the last of them ends behind the closing barrier and stores g itself, and the energy rows ride
in the last backward interval on the shortest chains.

On the host: the deal is complete and keeps the order every accumulator and every element of the gradient buffer relies on.
On the GPU: the evaluation stays bit-exact against the kernel-order oracle (oracle/picnn_chain.c, untouched by the deal) at
shapes that take every branch of the deal, and the persistent tile kernel -- 4-, 8- and 16-row tiles -- equals launch pairs."""
import ctypes as C

import numpy as np
import pytest
import torch

from icnn_amd import _lib, picnn
from test_architectures import DEEP
from test_shape_instance import fc_model

FC = picnn.FCSpec
SPECS = {
    "L1": FC(12, 9, (40,)),                                     # one hidden layer: nothing to move
    "narrow_next": FC(12, 33, (304, 33)),                       # 19 + 3 tiles: three dE/dy tiles beside 19 delta tiles
    "odd_kblocks": FC(12, 20, (70, 33, 18, 50)),                # 5 / 3 / 2 / 4 k-blocks, four intervals each way
    "wide_next": FC(12, 40, (40, 300)),                         # 19 tiles in the second layer, three in the first
    "n270": FC(12, 270, (300, 280)),                            # 17 dE/dy tiles: no wave without one, no backward move
    "box": FC(17, 6, (200, 200), alpha=0.01, action_box=True),
    "deep": DEEP,
}
SHIPPED = {"bibtex": picnn.bibtex_spec(), "halfcheetah": picnn.halfcheetah_spec()}
NWAVE = 16


def tiles(width):
    return (width + 15) // 16


# ---- host arithmetic ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(SHIPPED) + sorted(SPECS))
def test_deal_is_complete_and_ordered(name):
    spec = {**SHIPPED, **SPECS}[name]
    deal = _lib.fc_deal(fc_model(spec))
    L, n, w = spec.n_layers - 1, spec.n_labels, spec.widths
    want = [("fwd_y", i, t) for i in range(L) for t in range(tiles(w[i]))]
    want += [("fwd_z", i, t) for i in range(1, L) for t in range(tiles(w[i]))]
    want += [("delta", i, t) for i in range(1, L) for t in range(tiles(w[i - 1]))]
    want += [("dedy", i, t) for i in range(L) for t in range(tiles(n))]
    want += [("e", L, r) for r in range(16)]
    assert sorted(u[:3] for u in deal) == sorted(want)                  # every (GEMM, tile) unit exactly once
    site = {u[:3]: u[3:] for u in deal}
    assert all(0 <= s[1] < NWAVE and 0 <= s[0] <= s[2] <= 2 * L for s in site.values())
    for i in range(L):
        for t in range(tiles(w[i])):
            y = site["fwd_y", i, t]
            if i > 0:                                                   # the y and z parts on one wave, in that order
                z = site["fwd_z", i, t]
                assert z[1] == y[1] and y[0] <= z[0] == i, (i, t)
            assert y[2] == i                                            # the epilogue writes z_i in the layer's own interval
    for i in range(1, L):                                               # delta_{i-1} is ready when its readers start
        for t in range(tiles(w[i - 1])):
            assert site["delta", i, t][0] == site["delta", i, t][2] == 2 * L - 1 - i
    for t in range(tiles(n)):
        # the gradient buffer of a tile sees layers L-1 .. 0 in that order: in different intervals, or the later one is
        # the unit that crosses the last barrier; delta_i is at least an interval old when dE/dy_i reads it
        writes = [site["dedy", i, t][2] for i in range(L - 1, -1, -1)]
        assert writes == sorted(set(writes)), (t, writes)
        for i in range(L):
            assert site["dedy", i, t][0] >= 2 * L - 1 - i
            assert site["dedy", i, t][2] in (site["dedy", i, t][0], 2 * L)
        if writes[-1] == 2 * L:                                         # ... which holds one accumulator per wave
            assert tiles(n) <= NWAVE and site["dedy", 0, t][1] not in {site["dedy", 0, s][1] for s in range(t)}
    assert {site["e", L, r][0] for r in range(16)} <= set(range(L, 2 * L))


def test_the_bibsonomy_deal():
    """ten dE/dy_1 units on the six waves without a dE/dy_0 chain, ten dE/dy_0 units that end behind the last barrier, E beside
    the dE/dy_1 units"""
    site = {u[:3]: u[3:] for u in _lib.fc_deal(fc_model(SHIPPED["bibtex"]))}
    assert sorted({site["dedy", 1, t][1] for t in range(10)}) == list(range(10, 16))
    assert {site["dedy", 1, t][0] for t in range(10)} == {3} and {site["dedy", 0, t][2] for t in range(10)} == {4}
    assert {site["e", 2, r][:2] for r in range(16)} <= {(3, w) for w in range(10, 16)}


def test_deal_query_validates():
    lib = _lib.load()
    m = fc_model(SHIPPED["bibtex"])
    assert lib.icnn_be_debug_fc_deal(None, None, 0) == -1
    assert lib.icnn_be_debug_fc_deal(C.byref(m), None, 4) == -1
    assert lib.icnn_be_debug_fc_deal(C.byref(m), None, 0) == len(_lib.fc_deal(m))
    m.width[2] = 2
    assert lib.icnn_be_debug_fc_deal(C.byref(m), None, 0) == -1         # not a network: the final width is 1


# ---- on the GPU -----------------------------------------------------------------------------------------------------------

BATCHES = (1, 16, 17, 37)
SENTINEL = -7.0


@pytest.fixture(scope="module")
def nets():
    """name -> (model, parameters, context of 37 rows, y of 37 rows, oracle E and g of the 37 rows); built once, read only"""
    from oracle import picnn_oracle
    made = {}

    def get(name):
        if name not in made:
            spec = SPECS[name]
            rng = np.random.RandomState(len(name))
            params = picnn.init_params(spec, 3, "spread")
            model = picnn.FCModel(spec, params, "cuda")
            x = rng.randn(37, spec.n_features).astype(np.float32)
            ctx = model.context(torch.from_numpy(x)).contiguous()
            y = rng.rand(37, spec.n_labels)
            fg = picnn_oracle.make_fg_chain(params, ctx.cpu().numpy(), list(spec.szs), spec.alpha, spec.action_box)
            E, g = fg(y)
            E, g = np.asarray(E, np.float32).copy(), np.asarray(g, np.float32).copy()
            E.setflags(write=False)
            g.setflags(write=False)
            made[name] = (model, ctx, torch.from_numpy(y).cuda(), E, g)
        return made[name]
    return get


def _fg_raw(model, ctx, y, finished):
    """icnn_be_fc_fg into buffers filled with a sentinel: what a skipped tile must leave alone"""
    B = y.shape[0]
    f = torch.full((B,), SENTINEL, dtype=torch.float32, device="cuda")
    g = torch.full((B, model.spec.n_labels), SENTINEL, dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(_lib.load().icnn_be_fc_fg(C.byref(model.c_model), ctx.data_ptr(), y.data_ptr(), B, f.data_ptr(), g.data_ptr(),
                                         None if finished is None else finished.data_ptr(), C.c_void_p(stream)), "icnn_be_fc_fg")
    torch.cuda.synchronize()
    return f.cpu().numpy(), g.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("name", sorted(SPECS))
def test_fg_equals_the_chain_oracle(nets, name, B):
    """Once by the default dispatch (FCModel.fg) and once with the 16-row tile kernel, which batches this small otherwise leave to
    the per-sample kernel: the launcher takes the tile kernel whenever a phase-profile buffer is registered (the production
    kernels never touch the buffer).  Masks: none, one tile fully finished, every other sample finished."""
    model, ctx_all, y_all, E, g = nets(name)
    ctx, y = ctx_all[:B].contiguous(), y_all[:B].contiguous()
    lib = _lib.load()
    prof = torch.zeros(((B + 15) // 16) * 16 * 16, dtype=torch.int64, device="cuda")
    whole = np.zeros(B, np.int32)
    whole[:16] = 1
    masks = {"none": None, "tile": whole, "partly": (np.arange(B) % 2).astype(np.int32)}
    for tile_kernel in (False, True):
        lib.icnn_be_debug_profile_fc(C.c_void_p(prof.data_ptr()) if tile_kernel else None)
        try:
            f0, g0 = model.fg(ctx, y)
            torch.cuda.synchronize()
            assert np.array_equal(f0.cpu().numpy(), E[:B]) and np.array_equal(g0.cpu().numpy(), g[:B]), (tile_kernel, "fg")
            for what, fin in masks.items():
                fin_t = None if fin is None else torch.from_numpy(fin).cuda()
                fa, ga = _fg_raw(model, ctx, y, fin_t)
                for r in range(B):
                    same = fa[r] == E[r] and np.array_equal(ga[r], g[r])
                    untouched = fa[r] == SENTINEL and (ga[r] == SENTINEL).all()
                    if fin is None or not fin[r]:
                        assert same, (tile_kernel, what, r)
                    elif tile_kernel:                # a tile is skipped as a whole and only when all its samples are finished
                        skipped = fin[r // 16 * 16:r // 16 * 16 + 16].all()
                        assert untouched if skipped else same, (tile_kernel, what, r)
                    else:
                        assert same or untouched, (tile_kernel, what, r)
        finally:
            lib.icnn_be_debug_profile_fc(None)


def _solve_outputs(model, ctx, B, variant, flags):
    from icnn_amd import bundle_entropy
    res = bundle_entropy.FusedSolver(model, B, 3, variant, flags=flags).solve(ctx, 0.5)
    torch.cuda.synchronize()
    outs = [t.clone() for t in (res.y, res.lam, res.active, res.count[:B], res.n_iters[:B], res.newton_iters[:B], res.state.G,
                                res.state.h, res.state.ys, res.finished[:B], res.status[:B])]
    return outs, _lib.solve_plan(model.c_model, res.state.c_state)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", (4, 8, 16))
@pytest.mark.parametrize("name", sorted(SPECS))
def test_persistent_tile_kernel_equals_launch_pairs(nets, name, rows):
    """nIter 3 through the persistent tile kernel (the deal inside its round loop; tile rows as the plan sets them for the batch:
    4 rows at 37 samples, 8 rows at eight samples per CU, 16 rows beyond) against one launch per phase and round."""
    model, ctx_all, _, _, _ = nets(name)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = {4: 37, 8: 8 * cus, 16: 8 * cus + 19}[rows]
    ctx = ctx_all[torch.arange(B, device="cuda") % 37].contiguous()
    variant = "rl" if model.spec.action_box else "dual"
    tile, plan = _solve_outputs(model, ctx, B, variant, _lib.FLAG_PERSISTENT)
    pairs, plan2 = _solve_outputs(model, ctx, B, variant, _lib.FLAG_TWO_KERNELS)
    assert plan[:2] == ("TILE", rows) and plan2[0] != "TILE", (plan, plan2)
    for k, (a, b) in enumerate(zip(tile, pairs)):
        assert torch.equal(a, b), "output %d" % k
