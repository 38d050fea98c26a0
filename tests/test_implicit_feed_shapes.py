"""implicit_feed_kernel (icnn_amd/csrc/be_dual.hip) at every instance launch_implicit_feed can pick, every branch on the bundle
size k and both cut dtypes, on solver results written by hand (tests/feed_ref.py) -- independent of the solvers.

CPU part: the launcher's carve arithmetic restated says which instance every row of feed_ref.CASES lands on, and the float64
oracle is shown accurate on exactly these inputs against a longdouble restatement (a condition on the inputs, not a
measurement of the kernel).  GPU part: the kernel against the float64 oracle at the tier-A bound of DESIGN.md section 2.

n is the smallest width of the issue's table at which the instance is reached; the carve restatement agrees with every row, so
none was moved.  One row is degenerate by construction: at n = 1 the single column of y is overwritten with exactly 0.0, which
under the squared-error loss makes Z^-1 = 0 and the 1 x 1 block G Z^-1 G^T exactly zero.  Its condition number is undefined;
the bordered system [[0, 1], [1, 0]] stays regular and gives c = 0, v = 0 (the reference solves the bordered system,
completion/icnn_ebundle.py:512-518).  There the precondition asserts that instead of cond <= 1e3.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import feed_ref
from oracle import implicit_feed_oracle as feed_oracle

LOSSES = ["xent", "mse"]
TIER_A = 1e-9          # same mathematics, float64 summation / elimination order only
INSTANCES = {(t, kt, where) for t in ("float", "double") for kt in (16, 32) for where in ("LDS", "GLB")}


@functools.lru_cache(maxsize=None)
def _case(name, loss):
    """(state, oracle rows) of a table row: computed once, shared by the tests, never written to"""
    s = feed_ref.case_state(name, loss)
    A, xs, lams = s.bundles()
    with np.errstate(all="ignore"):
        rows = feed_oracle.feed_rows(s.y, s.labels, A, xs, lams, loss)
    for a in rows:
        a.setflags(write=False)
    return s, rows


def _zinv(y, loss):
    with np.errstate(divide="ignore"):
        yc = np.clip(y, 1e-8, 1.0 - 1e-8) if loss == "xent" else y
        return 1.0 / (1.0 / yc + 1.0 / (1.0 - yc))


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_table_reaches_every_instance_and_every_bundle_size():
    """The carve restatement puts every row on the instance it names; together the rows launch all eight instances and every k
    at which the kernel branches (spd_solve2_ks at 4 / 8 / 16, the 8x8 contraction up to 7, the second tile at 16,
    contract_mfma_cover2 at 17..20, the general loop from 21)."""
    seen, ks = set(), set()
    for name, inst, cut, slots, n, variant, counts in feed_ref.CASES:
        assert feed_ref.feed_instance(n, slots, cut) == inst, name
        assert max(counts) <= slots
        seen.add(inst)
        ks.update(counts)
    assert seen == INSTANCES
    assert ks == set(feed_ref.ALL_K)
    # the pdipm row's feed fits the LDS although its dual step needs the staging area (test_scratch_... below)
    assert feed_ref.feed_lds_bytes(1024, 31, np.float32) <= feed_ref.LDS_LIMIT < feed_ref.feed_lds_bytes(1104, 31, np.float32)


def test_carve_restatement_matches_the_library():
    """One wave of variant dual (n < 1024) carves exactly like the feed: icnn_be_bundle_capacity is the restated rows_fit, and
    the row is an LDS instance exactly when every slot fits."""
    from icnn_amd import _lib
    lib = _lib.load()
    checked = 0
    for name, inst, cut, slots, n, variant, counts in feed_ref.CASES:
        if n >= 1024 or variant != "dual":
            continue
        cd = _lib.CUT_F64 if cut == np.float64 else _lib.CUT_F32
        cap = lib.icnn_be_bundle_capacity(n, slots, cd, _lib.VARIANT["dual"])
        assert cap == feed_ref.rows_fit(n, slots, cut), name
        assert (cap == slots) == (inst[2] == "LDS"), name
        checked += 1
    assert checked >= 7
    # and off the table, across the threshold in both dtypes
    for cut, cd in ((np.float32, _lib.CUT_F32), (np.float64, _lib.CUT_F64)):
        for slots in (15, 31):
            for n in (159, 500, 640, 777, 1000, 1023):
                assert lib.icnn_be_bundle_capacity(n, slots, cd, _lib.VARIANT["dual"]) == feed_ref.rows_fit(n, slots, cut)


def _scratch_expected(case):
    """bytes of BundleState.scratch for a table row: [B][slots + 2][pitch] cuts where the state's DUAL STEP needs the staging
    area (be_dual.hip scratch_bytes), else 0"""
    name, inst, cut, slots, n, variant, counts = case
    staged = inst[2] == "GLB" or name == "f32_32_pdipm_n1024"
    return len(counts) * (slots + 2) * feed_ref.dual_row_pitch((n + 15) & ~15) * np.dtype(cut).itemsize if staged else 0


@pytest.mark.parametrize("case", feed_ref.CASES, ids=feed_ref.CASE_IDS)
def test_scratch_bytes_exactly_where_the_bundle_is_staged(case):
    from icnn_amd import _lib
    name, inst, cut, slots, n, variant, counts = case
    s = _lib.State()
    s.batch, s.n, s.slots = len(counts), n, slots
    s.cut_dtype = _lib.CUT_F64 if cut == np.float64 else _lib.CUT_F32
    s.variant = _lib.VARIANT[variant]
    assert int(_lib.load().icnn_be_scratch_bytes(C.byref(s))) == _scratch_expected(case)
    if inst[2] == "GLB":
        assert _scratch_expected(case) > 0
    # variant rl has no staging area: the refusal of test_feed_refuses_wide_rl_state_before_launch
    s.variant = _lib.VARIANT["rl"]
    assert int(_lib.load().icnn_be_scratch_bytes(C.byref(s))) == 0


@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("name", feed_ref.CASE_IDS)
def test_oracle_is_accurate_on_the_synthetic_inputs(name, loss):
    """Precondition of the GPU comparison: the float64 oracle within 1e-13 (1 + |ref|) of the longdouble restatement on c and v,
    cond2(G Z^-1 G^T) <= 1e3, every output finite, the saturated columns in place, NaN everywhere the kernel must not read."""
    s, (idx, rows_y, rows_v, rows_c) = _case(name, loss)
    A, xs, lams = s.bundles()
    with np.errstate(all="ignore"):
        idx_l, y_l, v_l, c_l = feed_ref.feed_rows_ld(s.y, s.labels, A, xs, lams, loss)
    assert np.array_equal(idx, idx_l) and np.array_equal(idx, np.repeat(np.arange(s.B), s.count))
    assert np.array_equal(rows_y, y_l)
    assert np.isfinite(rows_c).all() and np.isfinite(rows_v).all() and np.isfinite(rows_y).all()
    err_c = np.abs(rows_c - c_l) / (1.0 + np.abs(c_l))
    err_v = np.abs(rows_v - v_l) / (1.0 + np.abs(v_l))
    worst = 0.0
    for u in range(s.B):
        k = s.count[u]
        assert np.array_equal(s.y[u, s.sat], feed_ref.SATURATED[:len(s.sat)])
        assert np.isnan(s.lam[u, k:]).all() and np.isfinite(s.lam[u, :k]).all()
        off = np.setdiff1d(np.arange(s.slots), s.active[u, :k])
        assert np.isnan(s.G[u, off]).all() and np.isnan(s.ys[u, off]).all()
        assert len(set(s.active[u, :k].tolist())) == k
        if k == 0:
            continue
        Gm = np.array(A[u])
        M = (Gm * _zinv(s.y[u], loss)).dot(Gm.T)
        if s.n == 1 and not M.any():          # module docstring: y = 0.0 at n = 1 under mse
            assert loss == "mse" and k == 1 and rows_c[idx == u] == 0.0 and not rows_v[idx == u].any()
            continue
        cond = np.linalg.cond(M)
        worst = max(worst, cond)
        assert cond <= 1e3, (u, cond)
    print("%s %s: oracle vs longdouble c %.2e v %.2e, cond2 <= %.1f" % (name, loss, err_c.max(initial=0.0),
                                                                        err_v.max(initial=0.0), worst))
    assert np.all(err_c <= 1e-13) and np.all(err_v <= 1e-13)
    # slots in random order, not 0..k-1: otherwise the indirection G_u + slots[r] * n is not exercised
    assert any(not np.array_equal(s.active[u, :s.count[u]], np.arange(s.count[u])) for u in range(s.B))


def test_longdouble_elimination_solves_a_known_system():
    rng = np.random.RandomState(0)
    M = rng.randn(9, 9)
    M[0, 0] = 0.0                              # needs the row exchange
    x = rng.randn(9)
    got = feed_ref.solve_gepp_ld(M, M.dot(x))
    assert got.dtype == np.longdouble and np.allclose(np.asarray(got, dtype=np.float64), x, rtol=0, atol=1e-12)


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _run_feed(s, loss):
    import torch
    from icnn_amd import bundle_entropy
    res = s.to_device()
    out = []
    for _ in range(2):
        feed = bundle_entropy.implicit_feed(res, s.labels, loss)
        out.append([t.cpu().numpy() for t in feed.as_tuple()])
    torch.cuda.synchronize()
    return res, out


def _assert_feed(s, loss, rows, out, label):
    idx, rows_y, rows_v, rows_c = rows
    (sample, fy, fv, fc), again = out
    assert np.array_equal(sample, idx)
    assert np.array_equal(fy, rows_y)
    assert np.isfinite(fc).all() and np.isfinite(fv).all() and np.isfinite(fy).all()      # the NaN poison
    err_c = np.abs(fc - rows_c) / (1.0 + np.abs(rows_c))
    err_v = np.abs(fv - rows_v) / (1.0 + np.abs(rows_v))
    print("%s %s: device vs oracle c %.3e v %.3e (rows %d)" % (label, loss, err_c.max(initial=0.0), err_v.max(initial=0.0),
                                                               len(idx)))
    assert np.all(err_c <= TIER_A), float(err_c.max())
    assert np.all(err_v <= TIER_A), float(err_v.max())
    # rule :416: where y is exactly 0 or 1, c_y = 0 and v is c_lam,i (y - ys_i) alone
    exact = s.sat[:2]
    want = fc[:, None] * (s.y[idx][:, exact] - rows_y[:, exact])
    assert np.array_equal(fv[:, exact], want)
    for a, b in zip(out[0], again):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", feed_ref.CASES, ids=feed_ref.CASE_IDS)
def test_feed_kernel_instance(case, loss):
    name, inst, cut, slots, n, variant, counts = case
    s, rows = _case(name, loss)
    res, out = _run_feed(s, loss)
    want_scratch = _scratch_expected(case)
    assert (res.state.scratch.numel() if res.state.scratch is not None else 0) == want_scratch
    _assert_feed(s, loss, rows, out, "%s <%s,%d,%s>" % ((name,) + inst))


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
def test_feed_of_a_single_empty_bundle_has_no_rows(loss):
    s = feed_ref.synth_state(77, 1, 8, np.float32, "dual", (0,), loss)
    _, out = _run_feed(s, loss)
    sample, fy, fv, fc = out[0]
    assert sample.shape == (0,) and fc.shape == (0,) and fy.shape == (0, 1) and fv.shape == (0, 1)


@pytest.mark.gpu
def test_feed_refuses_wide_rl_state_before_launch():
    """Variant rl has no staging area (scratch_bytes is 0) and 31 slots of n = 2048 exceed the LDS: launch_implicit_feed
    returns hipErrorInvalidValue before anything is launched."""
    import torch
    from icnn_amd import bundle_entropy
    assert feed_ref.feed_instance(2048, 31, np.float32) == ("float", 32, "GLB")
    s = feed_ref.synth_state(78, 2048, 31, np.float32, "rl", (1, 8), "mse")
    res = s.to_device()
    assert res.state.scratch is None
    with pytest.raises(RuntimeError, match="ICNN_BE_EINVAL"):
        bundle_entropy.implicit_feed(res, s.labels, "mse")
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("loss", LOSSES)
def test_feed_of_an_rl_state_that_fits_equals_the_dual_state(loss):
    s, rows = _case("f32_16", loss)
    _, out_dual = _run_feed(s, loss)
    rl = feed_ref.case_state("f32_16", loss)
    rl.variant = "rl"
    res, out_rl = _run_feed(rl, loss)
    assert res.state.variant == "rl"
    _assert_feed(rl, loss, rows, out_rl, "f32_16 as rl")
    for a, b in zip(out_dual[0], out_rl[0]):
        assert a.tobytes() == b.tobytes()
