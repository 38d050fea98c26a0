"""CPU-only checks: the C-ABI library loads and exports every symbol include/icnn_be.h declares,
argument validation works without a GPU, the weight packer is a pure permutation, and the
oracle PICNN is self-consistent (autograd gradient, convexity in y)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import problems

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    from icnn_amd import _lib, build
    build.build()
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    declared = sorted(set(re.findall(r"ICNN_BE_API\s+[\w\s\*]+?\b(icnn_be_\w+)\s*\(", header)))
    assert declared, "no ICNN_BE_API declarations found"
    assert sorted(_lib.EXPORTS) == declared
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.icnn_be_abi_version() == _lib.ABI_VERSION


def test_struct_layouts_match_header_sizes():
    from icnn_amd import _lib
    lib = _lib.load()
    assert C.sizeof(_lib.State) == lib.icnn_be_struct_size(0) == 6 * 4 + 18 * 8 + 8      # + fvals, iters (padded)
    assert C.sizeof(_lib.FcModel) == lib.icnn_be_struct_size(1) == 64


def test_argument_validation_without_gpu():
    from icnn_amd import _lib
    lib = _lib.load()
    st = _lib.State()
    assert lib.icnn_be_state_init(C.byref(st), None) == -1          # n = 0
    st.batch, st.n, st.slots = 4, 5, 40
    assert lib.icnn_be_state_init(C.byref(st), None) == -2          # slots > ICNN_BE_MAX_SLOTS
    st.slots = 10
    assert lib.icnn_be_state_init(C.byref(st), None) == -1          # null buffers
    assert lib.icnn_be_dual_lds_bytes(159, 10, 0) > 0
    assert lib.icnn_be_dual_lds_bytes(159, 10, 0) < lib.icnn_be_dual_lds_bytes(159, 30, 0) <= 160 * 1024
    m = _lib.FcModel()
    m.n, m.n_layers = 159, 3
    m.width[0], m.width[1], m.width[2] = 600, 159, 2                 # last width must be 1
    m.ctx_width = 1996
    assert lib.icnn_be_fc_pack_floats(C.byref(m)) == 0
    m.width[2] = 1
    assert lib.icnn_be_fc_pack_floats(C.byref(m)) > 216399
    m.ctx_width = 7
    assert lib.icnn_be_fc_pack_floats(C.byref(m)) == 0               # context width mismatch


def test_adam_obs_entry_refuses_mismatched_model_and_context_descriptions():
    """icnn_be_adam_fc_obs reads the context producer's stage matrices (laid out for icnn_be_fc_ctx.width) with the MODEL's
    widths: both structs must describe the same network, width by width (ADVICE r2 / VERDICT r3: a C caller with
    mismatched structs would read out of bounds).  Checked before anything is enqueued: no GPU needed."""
    from icnn_amd import _lib
    lib = _lib.load()
    m = _lib.FcModel()
    m.n, m.n_layers = 6, 3
    m.width[0], m.width[1], m.width[2] = 200, 200, 1
    m.alpha, m.action_box = 0.01, 0
    m.ctx_width = 3 * 6 + 200 + 200 + 1 + 200 + 200
    dummy = (C.c_float * 4)()
    m.wpack = C.cast(dummy, C.c_void_p)
    assert lib.icnn_be_fc_pack_floats(C.byref(m)) > 0
    cx = _lib.FcCtx()
    cx.n_features, cx.n, cx.n_layers = 17, 6, 3
    cx.width[0], cx.width[1], cx.width[2] = 200, 200, 1
    cx.batchnorm, cx.bn_eps = 0, 1e-5
    for i in range(3):
        cx.w_stage[i] = C.cast(dummy, C.c_void_p)
        cx.b_stage[i] = C.cast(dummy, C.c_void_p)
    # past validation an empty batch only zeroes `iters` on the device: with a GPU that must be device memory (a host
    # array makes the memset fail, and the runtime keeps that error for the next launch in the process)
    gpu = torch.cuda.is_available()
    iters = torch.full((1,), 7, dtype=torch.int32, device="cuda") if gpu else None
    args = (C.byref(m), C.byref(cx), dummy, 0, 10, dummy, dummy, C.c_void_p(iters.data_ptr()) if gpu else dummy, dummy, None)
    if gpu:
        assert lib.icnn_be_adam_fc_obs(*args) == 0                   # consistent description: past validation
        assert int(iters.item()) == 0
    else:
        assert lib.icnn_be_adam_fc_obs(*args) in (0, -3)             # consistent description: past validation (empty batch;
                                                                     # -3 = the memset of `iters` found no device on this box)
    cx.width[1] = 100                                                # another hidden width: refused
    assert lib.icnn_be_adam_fc_obs(*args) == -1
    cx.width[1] = 200
    cx.n = 5
    assert lib.icnn_be_adam_fc_obs(*args) == -1
    cx.n = 6
    cx.n_layers = 2
    assert lib.icnn_be_adam_fc_obs(*args) == -1


def test_adam_obs_entry_refuses_a_relu_last_u_context_without_batchnorm():
    """The in-kernel context producer keeps the last u-layer linear, so a context description with u_last_relu set is a bad
    argument to icnn_be_adam_fc_obs (ICNN_BE_EINVAL, not the ICNN_BE_ELIMIT that sends a caller to context + Adam) also for a
    model without BatchNorm, at any batch, and icnn_be_debug_adam_plan refuses it alike.  rl_adam.AdamSolver.solve_obs
    therefore answers None for such a model before it calls the library.  Nothing is enqueued: no GPU needed."""
    from icnn_amd import _lib
    lib = _lib.load()
    m = _lib.FcModel()
    m.n, m.n_layers = 6, 3
    m.width[0], m.width[1], m.width[2] = 24, 16, 1
    m.alpha, m.action_box = 0.01, 0
    m.ctx_width = 3 * 6 + 24 + 16 + 1 + 24 + 16
    dummy = (C.c_float * 4)()
    m.wpack = C.cast(dummy, C.c_void_p)
    assert lib.icnn_be_fc_pack_floats(C.byref(m)) > 0
    cx = _lib.FcCtx()
    cx.n_features, cx.n, cx.n_layers = 7, 6, 3
    cx.width[0], cx.width[1], cx.width[2] = 24, 16, 1
    cx.batchnorm, cx.bn_eps, cx.u_last_relu = 0, 1e-5, 1
    for i in range(3):
        cx.w_stage[i] = C.cast(dummy, C.c_void_p)
        cx.b_stage[i] = C.cast(dummy, C.c_void_p)
    out = (C.c_int * 4)()
    for batch in (0, 1, 3, 700):
        assert lib.icnn_be_adam_fc_obs(C.byref(m), C.byref(cx), dummy, batch, 10, dummy, dummy, dummy, dummy, None) == -1
    assert lib.icnn_be_debug_adam_plan(C.byref(m), C.byref(cx), 3, C.byref(out)) == -1
    # up to four states the plan is host arithmetic (one workgroup, no occupancy query): without the flag it is the latency
    # path with the observation form accepted, and 7 features against ctx_off = 464 are far inside the scratch guard
    cx.u_last_relu = 0
    assert _lib.adam_plan(m, 3, cx) == ("ROWS", 3, 1, False, True)
    assert _lib.adam_plan(m, 3) == ("ROWS", 3, 1, False, False)
    cx.n_features = 233                                              # 2 * 233 > 464: outside the guard
    assert _lib.adam_plan(m, 3, cx) == ("ROWS", 3, 1, False, False)
    cx.n_features = 232
    assert _lib.adam_plan(m, 3, cx) == ("ROWS", 3, 1, False, True)
    cx.batchnorm = 1
    cx.bn_gamma[0] = cx.bn_beta[0] = C.cast(dummy, C.c_void_p)
    assert _lib.adam_plan(m, 3, cx) == ("ROWS", 3, 1, False, False)
    m.n = 65                                                         # one tile: still no device needed
    m.ctx_width = 3 * 65 + 24 + 16 + 1 + 24 + 16
    assert _lib.adam_plan(m, 16) == ("TILE", 16, 1, False, False)
    assert lib.icnn_be_debug_adam_plan(C.byref(m), None, 0, C.byref(out)) == -1       # nothing to plan
    assert lib.icnn_be_debug_adam_plan(C.byref(m), None, 16, None) == -1
    m.action_box = 1
    assert lib.icnn_be_debug_adam_plan(C.byref(m), None, 16, C.byref(out)) == -1      # as icnn_be_adam_fc refuses it


def test_context_stage_accepts_an_empty_shard_with_null_buffers():
    """a data-parallel rank whose shard is empty (batch < world size) hands over zero-element tensors, whose data
    pointers are NULL; icnn_be_fc_context_stage must return its "sums pending" code (1) for the normalised stages -- so that
    the rank still joins the all-reduce -- and 0 for the others, not ICNN_BE_EINVAL.  Host-side decision: no GPU needed."""
    from icnn_amd import _lib
    lib = _lib.load()
    cx = _lib.FcCtx()
    cx.n_features, cx.n, cx.n_layers = 17, 6, 3
    cx.width[0], cx.width[1], cx.width[2] = 200, 200, 1
    cx.batchnorm, cx.bn_eps = 1, 1e-5
    dummy = (C.c_float * 4)()
    for i in range(3):
        cx.w_stage[i] = C.cast(dummy, C.c_void_p)
        cx.b_stage[i] = C.cast(dummy, C.c_void_p)
        cx.bn_gamma[i] = C.cast(dummy, C.c_void_p)
        cx.bn_beta[i] = C.cast(dummy, C.c_void_p)
    ctx_width = 3 * 6 + 200 + 200 + 1 + 200 + 200
    rcs = [lib.icnn_be_fc_context_stage(C.byref(cx), stage, None, 0, None, ctx_width, None, None, None) for stage in range(3)]
    assert rcs == [1, 0, 0], rcs                      # stage 0 is followed by BatchNorm (n_layers - 2 = 1 normalised stage)
    assert lib.icnn_be_fc_context_stage(C.byref(cx), 0, None, 4, None, ctx_width, None, None, None) == -1   # rows but no buffers


def test_weight_pack_is_a_permutation_of_both_orientations():
    from icnn_amd import _lib, picnn
    lib = _lib.load()
    spec = picnn.FCSpec(20, 21, (37, 21))
    params = picnn.init_params(spec, 0, "init")
    m = _lib.FcModel()
    m.n, m.n_layers, m.ctx_width = spec.n_labels, spec.n_layers, spec.ctx_width
    for i, w in enumerate(spec.widths):
        m.width[i] = w
    nf = lib.icnn_be_fc_pack_floats(C.byref(m))
    out = np.empty(nf, np.float32)
    keep = [np.ascontiguousarray(params["z%d_yu/W" % i]) for i in range(3)]
    keepz = [None] + [np.ascontiguousarray(params["z%d_zu_proj/W" % i]) for i in (1, 2)]
    yu = (C.c_void_p * 3)(*[a.ctypes.data for a in keep])
    zu = (C.c_void_p * 3)(*[None if a is None else a.ctypes.data for a in keepz])
    assert lib.icnn_be_fc_pack(C.byref(m), yu, zu, out.ctypes.data) == 0
    # every hidden-layer weight appears exactly twice (forward and transposed operand), the final
    # layer's vectors once; everything else is zero padding
    expect = 2 * sum(float(np.abs(keep[i]).sum()) for i in (0, 1)) + 2 * float(np.abs(keepz[1]).sum()) \
        + float(np.abs(keep[2]).sum()) + float(np.abs(keepz[2]).sum())
    assert abs(float(np.abs(out).sum()) - expect) <= 1e-3 * expect
    # first forward tile of z0_yu: pack[lane*4+s] = W[4*(lane>>4)+s][lane&15]
    W = keep[0]
    for lane in (0, 5, 17, 63):
        for s in range(4):
            assert out[lane * 4 + s] == W[4 * (lane >> 4) + s, lane & 15]


def test_device_model_recognises_period_three_cycles():
    """The limit-cycle rule of the device formulation (oracle/device_model.py, mirrored by the kernel): an
    iteration that revisits lam_{t-3} returns the iterate whose phase matches the reference's final count."""
    from oracle import device_model

    # the rule itself, as a pure function of the history (what the kernel implements in registers)
    def stop(done, cap, lam_new, prev1, prev2, prev3, tol=device_model.CYCLE_TOL):
        if prev1 is not None and np.max(np.abs(lam_new - prev1)) <= tol:
            return lam_new
        if prev2 is not None and np.max(np.abs(lam_new - prev2)) <= tol:
            return lam_new if (cap - done) % 2 == 0 else prev1
        if prev3 is not None and np.max(np.abs(lam_new - prev3)) <= tol:
            return (lam_new, prev2, prev1)[(cap - done) % 3]
        return None

    cap = 100
    seq = [np.array([0.2, 0.8]), np.array([0.5, 0.5]), np.array([0.7, 0.3])]     # an exact 3-cycle
    hist = [seq[t % 3] for t in range(cap + 1)]               # lam_0 .. lam_cap
    for done in range(4, 12):                                  # detection may happen at any phase
        got = stop(done, cap, hist[done], hist[done - 1], hist[done - 2], hist[done - 3])
        assert got is not None and np.array_equal(got, hist[cap]), done
    # and the text of the model uses the same selection
    import inspect
    src = inspect.getsource(device_model.simplex_newton_device)
    assert "(lam_new, prev2, prev1)[r]" in src and "% 3" in src


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    from icnn_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    with pytest.raises(ImportError, match="no CPU fallback"):
        _lib.load()


def test_solvebatch_refuses_to_run_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from icnn_amd import bundle_entropy
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        bundle_entropy.solveBatch(lambda y: (y.sum(1), y), np.full((2, 3), 0.5))


def test_solver_argument_of_the_interior_point_module():
    """lib/bundle_entropy.py:192 takes solver='pc'|'boyd' as fifth argument: 'pc' selects the interior-point variant
    (GPU tests), 'boyd' is not built and says so, an unknown name raises what the reference raises (:232)."""
    from icnn_amd import bundle_entropy
    y0 = np.full((2, 3), 0.5)
    fg = lambda y: (np.zeros(2, np.float32), np.zeros((2, 3), np.float32))
    with pytest.raises(NotImplementedError, match="pdipm_boyd"):
        bundle_entropy.solveBatch(fg, y0, nIter=10, solver="boyd")
    with pytest.raises(RuntimeError, match="Solver unknown"):
        bundle_entropy.solveBatch(fg, y0, solver="simplex")


def test_dropin_modules_expose_the_reference_signatures():
    """`dropin/` is what replaces `../lib` on the scripts' sys.path (multi-label-cls/icnn_ebundle.py:27-30,
    RL/src/icnn.py:8): module name, function name and the positional parameters of the reference."""
    import importlib.util
    import inspect
    for fname, variant in (("bundle_entropy_dual.py", "dual"), ("bundle_entropy_rl.py", "rl")):
        spec = importlib.util.spec_from_file_location("dropin_" + fname[:-3], os.path.join(REPO, "dropin", fname))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        params = list(inspect.signature(mod.solveBatch).parameters.values())
        assert [p.name for p in params[:4]] == ["fg", "initXs", "nIter", "callback"]
        assert params[3].default is None        # nIter=None resolves to the variant's default (10 / 5) inside
        assert inspect.signature(mod.solveBatch).parameters["variant"].default == variant
        if variant == "dual":                   # lib/bundle_entropy_dual.py:87  solve(fg, initX, nIter=10, callback=None)
            params = list(inspect.signature(mod.solve).parameters.values())
            assert [p.name for p in params[:4]] == ["fg", "initX", "nIter", "callback"]
            assert params[2].default == 10 and params[3].default is None
    # the module the icnn_ebundle.py scripts import: lib/bundle_entropy.py's five positional parameters and defaults
    spec = importlib.util.spec_from_file_location("dropin_be", os.path.join(REPO, "dropin", "bundle_entropy.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    params = list(inspect.signature(mod.solveBatch).parameters.values())
    assert [p.name for p in params[:5]] == ["fg", "initXs", "nIter", "callback", "solver"]
    assert params[2].default == 10 and params[3].default is None and params[4].default == "pc"


def test_adam_host_mirror_checks_the_model_before_touching_the_gpu():
    """rl_adam.AdamSolver rejects the [0,1]-box re-parametrisation (adam() works on the action itself)."""
    from icnn_amd import picnn, rl_adam

    class FakeModel:
        spec = picnn.halfcheetah_spec()          # action_box=True

    with pytest.raises(ValueError, match="action_box"):
        rl_adam.AdamSolver(FakeModel(), 1)


def test_oracle_picnn_gradient_and_convexity():
    from icnn_amd import picnn
    from oracle import picnn_oracle
    for spec, kw in ((picnn.FCSpec(30, 13, (21, 13)), {}),
                     (picnn.FCSpec(17, 6, (20, 20), alpha=0.01, batchnorm=False), dict(yu_bias=1.0, gate_bias=1.0))):
        params = picnn.init_params(spec, 2, "spread", **kw)
        rng = np.random.RandomState(0)
        x = rng.randn(9, spec.n_features).astype(np.float32)
        ctx = picnn_oracle.context(params, x, list(spec.szs), spec.batchnorm)
        y = rng.rand(9, spec.n_labels).astype(np.float32)
        E, g = picnn_oracle.energy_and_grad(params, ctx, y, list(spec.szs), spec.alpha)

        # the same network in torch float64 with autograd
        t = {k: torch.tensor(v, dtype=torch.float64) for k, v in params.items()}
        yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
        z = None
        L = len(spec.szs)
        for i in range(L + 1):
            c = ctx[i]
            p = (yt * torch.tensor(c["yu"], dtype=torch.float64)) @ t["z%d_yu/W" % i] \
                + torch.tensor(c["zu"], dtype=torch.float64)
            if i > 0:
                p = p + (z * torch.tensor(c["gate"], dtype=torch.float64)) @ t["z%d_zu_proj/W" % i]
            z = torch.where(p > 0, p, spec.alpha * p) if i < L else p
        Et = z.reshape(-1)
        Et.sum().backward()
        assert np.allclose(E, Et.detach().numpy(), rtol=2e-5, atol=2e-5)
        assert np.allclose(g, yt.grad.numpy(), rtol=2e-4, atol=2e-5)

        # convexity in y along random segments: E(mid) <= (E(a)+E(b))/2
        a, b = rng.rand(9, spec.n_labels).astype(np.float32), rng.rand(9, spec.n_labels).astype(np.float32)
        Ea, _ = picnn_oracle.energy_and_grad(params, ctx, a, list(spec.szs), spec.alpha)
        Eb, _ = picnn_oracle.energy_and_grad(params, ctx, b, list(spec.szs), spec.alpha)
        Em, _ = picnn_oracle.energy_and_grad(params, ctx, (a + b) / 2, list(spec.szs), spec.alpha)
        assert np.all(Em <= (Ea + Eb) / 2 + 1e-4 * (1 + np.abs(Ea) + np.abs(Eb)))


def test_device_model_reproduces_reference_golden():
    """The device formulations (Gram/inertia rank test, partial-pivot LU, limit-cycle shortcut,
    NumPy-order sums) give the reference's results on every golden case (variant dual)."""
    import problems
    from golden_util import assert_matches_golden, flatten_slots, load_golden
    from oracle import device_model
    for case in sorted(problems.GOLDEN_CASES):
        factory, n_iter = problems.GOLDEN_CASES[case]
        prob = factory()
        with np.errstate(all="ignore"):
            res = device_model.solve_batch_device(prob.fg, prob.y0(), n_iter, variant="dual")
        got = flatten_slots(res.y, res.G, res.h, res.ys, res.active, res.lam, res.n_iters, n_iter)
        assert_matches_golden(got, load_golden(case, "dual"), y_tol=1e-9, lam_tol=1e-6, chk_rtol=1e-7, what=case)


def test_conv_kernel_order_oracle_agrees_with_the_autograd_oracle():
    """oracle/picnn_conv_chain.c (float32 sums in the HIP kernel's order, hand-written backward pass) against
    oracle/picnn_conv_oracle.py (torch conv2d + autograd): same network, float32 rounding apart."""
    from icnn_amd import picnn
    from oracle import picnn_conv_oracle as co
    spec = picnn.ConvSpec()
    for regime in ("spread", "init"):
        params = picnn.init_conv_params(spec, 0, regime)
        x = np.random.RandomState(50).rand(5, spec.H, spec.W, 1).astype(np.float32)
        ctx = co.flat_context(co.context(params, torch.from_numpy(x)))
        y = 0.05 + 0.9 * np.random.RandomState(3).rand(5, spec.n_labels)
        f1, g1 = co.energy_and_grad_chain(params, ctx, y, spec.H, spec.W)
        f2, g2 = co.make_fg_from_context(params, ctx, spec.H, spec.W)(y)
        assert np.max(np.abs(f1 - f2)) <= 2e-6 * max(1.0, np.abs(f2).max())
        assert np.max(np.abs(g1 - g2)) <= 2e-6 * np.abs(g2).max()


def test_conv_weight_pack_holds_every_weight_the_expected_number_of_times():
    """Host packing of the conv PICNN operands (icnn_be_conv_pack, no GPU involved): raw single-channel pieces once,
    every 'zu_proj' tensor once in its forward operand and once across its transposed operand(s) -- the stride-2 layer's
    taps are dealt over four parity-class operands, the first layer's over the pixel-shuffle operand, each tap exactly
    once --, the 2048 x 512 matrix in both orientations; everything else zero padding."""
    from icnn_amd import _lib, picnn
    lib = _lib.load()
    spec = picnn.ConvSpec()
    params = picnn.init_conv_params(spec, 3, "spread")
    m = _lib.ConvModel()
    m.H, m.W = spec.H, spec.W
    for l, (nf, k, s) in enumerate(picnn.CONV_LAYERS):
        m.filters[l], m.ksize[l], m.stride[l] = nf, k, s
    m.fc_hidden, m.ctx_width = picnn.CONV_FCS[0], spec.ctx_width
    n = int(lib.icnn_be_conv_pack_floats(C.byref(m)))
    assert n > 0
    keep = []

    def ptr(name):
        a = np.ascontiguousarray(params[name], dtype=np.float32)
        keep.append(a)
        return a.ctypes.data

    w_yu = (C.c_void_p * 3)(*[ptr("z%d_yu/W" % l) for l in range(3)])
    w_yr = (C.c_void_p * 3)(*([ptr("z%d_y_red/W" % l) for l in range(2)] + [None]))
    b_yr = (C.c_void_p * 3)(*([ptr("z%d_y_red/b" % l) for l in range(2)] + [None]))
    w_zu = (C.c_void_p * 3)(*([None] + [ptr("z%d_zu_proj/W" % l) for l in (1, 2)]))
    host = np.empty(n, dtype=np.float32)
    assert lib.icnn_be_conv_pack(C.byref(m), w_yu, w_yr, b_yr, w_zu, ptr("z3_zu_proj/W"), ptr("z4_zu_proj/W"),
                                 host.ctypes.data) == 0
    mass = lambda name: float(np.abs(params[name].astype(np.float64)).sum())     # noqa: E731
    expect = (2 * mass("z0_yu/W") + mass("z0_yu/W")          # raw + forward operand + pixel-shuffle operand
              + mass("z1_yu/W") + mass("z2_yu/W")            # raw (VALU chains, forward and transposed)
              + mass("z0_y_red/W") + mass("z1_y_red/W") + mass("z0_y_red/b") + mass("z1_y_red/b")
              + 2 * mass("z1_zu_proj/W") + 2 * mass("z2_zu_proj/W") + 2 * mass("z3_zu_proj/W") + mass("z4_zu_proj/W"))
    assert abs(float(np.abs(host.astype(np.float64)).sum()) - expect) <= 1e-6 * expect
    # the scratch query scales with the batch and the shape is refused when it is not the reference network
    assert lib.icnn_be_conv_work_floats(C.byref(m), 256) == 256 * (16 * 8 * 32 + 8 * 4 * 64 + 2 * 2048 + 2 * 512)
    m.filters[1] = 48
    assert lib.icnn_be_conv_pack_floats(C.byref(m)) == 0


def test_stage_concatenation_of_the_context_weights():
    """picnn.stage_weights (the host packing icnn_be_fc_context consumes): prev_i @ W_stage_i + b_stage_i, cut at the
    documented column boundaries, equals the torch statement of the context."""
    from icnn_amd import picnn
    spec = picnn.FCSpec(23, 7, (12, 9, 5))
    params = picnn.init_params(spec, 2, "spread")
    x = np.random.RandomState(4).randn(6, 23).astype(np.float32)
    ref = picnn.context(spec, params, torch.from_numpy(x)).numpy()
    stages = picnn.stage_weights(spec, params)
    L, n, w = len(spec.szs), spec.n_labels, spec.widths
    prev, cols = x, []
    for i, (W, b) in enumerate(stages):
        assert W.shape[1] % 4 == 0 and W.shape[0] == prev.shape[1]
        out = prev @ W[:, :len(b)] + b
        o = 0
        if i < L:
            u = out[:, :w[i]]
            o = w[i]
            if i < L - 1:
                u = np.maximum(u, 0)
                mean, var = u.mean(0), ((u - u.mean(0)) ** 2).mean(0)
                u = (u - mean) / np.sqrt(var + 1e-5) * params["u%d/bn/gamma" % i] + params["u%d/bn/beta" % i]
        cols.append(out[:, o:o + n]); o += n
        cols.append(out[:, o:o + w[i]]); o += w[i]
        if i > 0:
            cols.append(np.maximum(out[:, o:o + w[i - 1]], 0)); o += w[i - 1]
        assert o == len(b)
        if i < L:
            prev = u.astype(np.float32)
    got = np.concatenate(cols, axis=1)
    assert got.shape == ref.shape
    assert np.max(np.abs(got - ref)) <= 1e-4 * max(1.0, np.abs(ref).max())


def test_stage_concatenation_of_the_conv_context_weights():
    """picnn.stage_conv_weights (what icnn_be_conv_context consumes) through a NumPy statement of the kernel's mapping
    -- GEMM row = (sample, output position), K index = (ky, kx, ci), zero outside the image, a head's columns routed to
    ctx[b][off + pos * F + f] at the offsets of include/icnn_be.h -- equals the torch statement of the context."""
    from icnn_amd import picnn
    spec = picnn.ConvSpec(H=16, W=8)
    params = picnn.init_conv_params(spec, 3, "spread")
    B = 3
    x = np.random.RandomState(8).rand(B, spec.H, spec.W, 1).astype(np.float32)
    ref = picnn.conv_context(spec, params, torch.from_numpy(x)).numpy()
    stages = picnn.stage_conv_weights(params)

    def im2col(inp, k, s, p):                        # [B][IH][IW][C] -> [B * OH * OW][k * k * C], (ky, kx, ci) order
        Bn, IH, IW, C = inp.shape
        OH, OW = (IH + s - 1) // s, (IW + s - 1) // s
        pad = np.zeros((Bn, IH + 2 * p + k, IW + 2 * p + k, C), np.float32)
        pad[:, p:p + IH, p:p + IW] = inp
        rows = np.empty((Bn, OH, OW, k, k, C), np.float32)
        for oy in range(OH):
            for ox in range(OW):
                rows[:, oy, ox] = pad[:, oy * s:oy * s + k, ox * s:ox * s + k]
        return rows.reshape(Bn * OH * OW, k * k * C), OH, OW

    def bn(u, i):
        mean, var = u.mean(0), ((u - u.mean(0)) ** 2).mean(0)
        return ((u - mean) / np.sqrt(var + 1e-5) * params["u%d/bn/gamma" % i] + params["u%d/bn/beta" % i]).astype(np.float32)

    (F0, K0, S0), (F1, K1, S1), (F2, K2, S2) = picnn.CONV_LAYERS
    fch = picnn.CONV_FCS[0]
    relu = lambda v: np.maximum(v, 0)
    per_sample = lambda m: m.reshape(B, -1)          # [B * P][F] -> [B][P * F]: what the routed epilogue writes
    a, oh0, ow0 = im2col(x, K0, S0, 2)
    o = a @ stages[0][0] + stages[0][1]
    u0, zu0 = bn(relu(o[:, :F0]), 0), per_sample(o[:, F0:])
    a, _, _ = im2col(x, 3, 1, 1)
    yu0 = per_sample(a @ stages[1][0] + stages[1][1])
    u0_map = u0.reshape(B, oh0, ow0, F0)
    a, oh1, ow1 = im2col(u0_map, K1, S1, 1)
    o = a @ stages[2][0] + stages[2][1]
    u1, zu1 = bn(relu(o[:, :F1]), 1), per_sample(o[:, F1:])
    a, _, _ = im2col(u0_map, 3, 1, 1)
    o = a @ stages[3][0] + stages[3][1]
    gate1, yu1 = per_sample(relu(o[:, :F0])), per_sample(o[:, F0:])
    u1_map = u1.reshape(B, oh1, ow1, F1)
    a, _, _ = im2col(u1_map, K2, S2, 1)
    o = a @ stages[4][0] + stages[4][1]
    u2 = bn(relu(o[:, :F2]), 2)
    gate2, yu2, zu2 = per_sample(relu(o[:, F2:F2 + F1])), per_sample(o[:, F2 + F1:F2 + F1 + 1]), per_sample(o[:, F2 + F1 + 1:])
    flat = per_sample(u2)
    o = flat @ stages[5][0] + stages[5][1]
    u3, gate3, zu3 = bn(relu(o[:, :fch]), 3), relu(o[:, fch:fch + flat.shape[1]]), o[:, fch + flat.shape[1]:]
    o = u3 @ stages[6][0] + stages[6][1]
    gate4, zu4 = relu(o[:, :fch]), o[:, fch:]
    got = np.concatenate([yu0, zu0, gate1, yu1, zu1, gate2, yu2, zu2, gate3, zu3, gate4, zu4], axis=1)
    assert got.shape == ref.shape == (B, spec.ctx_width)
    assert np.max(np.abs(got - ref)) <= 1e-4 * max(1.0, np.abs(ref).max())


def test_bundle_capacity_and_scratch_size_are_host_computations():
    """icnn_be_bundle_capacity / icnn_be_scratch_bytes (no kernel launch): narrow rows stage every slot in LDS and need no
    scratch; the completion width stages 12 float32 cuts (fewer for the interior-point variant and for float64 cuts) and
    asks for [B][slots + 2][pitch] cuts of device memory as soon as there are more slots than that; the RL variant has no
    device-memory staging."""
    from icnn_amd import _lib
    lib = _lib.load()
    D, P, R = _lib.VARIANT["dual"], _lib.VARIANT["pdipm"], _lib.VARIANT["rl"]
    assert lib.icnn_be_bundle_capacity(159, 31, _lib.CUT_F32, D) == 31
    assert lib.icnn_be_bundle_capacity(6, 5, _lib.CUT_F32, R) == 5
    cap = lib.icnn_be_bundle_capacity(2048, 30, _lib.CUT_F32, D)
    assert cap == 12
    assert lib.icnn_be_bundle_capacity(2048, 5, _lib.CUT_F32, D) == 5
    assert 2 <= lib.icnn_be_bundle_capacity(2048, 30, _lib.CUT_F64, D) < lib.icnn_be_bundle_capacity(2048, 30, _lib.CUT_F32, P) < cap
    assert lib.icnn_be_bundle_capacity(2048, 40, _lib.CUT_F32, D) < 0          # more slots than ICNN_BE_MAX_SLOTS

    def scratch(n, slots, variant, cut=_lib.CUT_F32, batch=256, flags=0):
        s = _lib.State()
        s.batch, s.n, s.slots, s.cut_dtype, s.variant, s.flags = batch, n, slots, cut, variant, flags
        return int(lib.icnn_be_scratch_bytes(C.byref(s)))

    assert scratch(159, 31, D) == 0 and scratch(2048, 5, D) == 0 and scratch(2048, 12, D) == 0
    got = scratch(2048, 30, D)
    assert got > 0 and got % (256 * 32 * 4) == 0 and got // (256 * 32 * 4) >= 2048
    assert scratch(2048, 30, P) == got and scratch(2048, 30, D, _lib.CUT_F64) == 2 * got
    assert scratch(2048, 30, R) == 0
    assert scratch(2048, 5, D, flags=_lib.FLAG_GLOBAL_BUNDLE) > 0             # forced staging (diagnostic flag)


def test_repack_keeps_the_context_weights_usable():
    """INTEGRATION.md's per-update flow is model.repack(params) followed by model.context(x) / rl_adam.adam(model, obs):
    repack must leave the x-only stage weights (struct icnn_be_fc_ctx) rebuilt from the SAME parameter set, not unset
    (ADVICE round 2).  Host-side check on a CPU-resident model; the GPU half is in tests/test_gpu_parity.py."""
    from icnn_amd import picnn
    spec = picnn.halfcheetah_spec()
    p0 = picnn.init_params(spec, 0, "spread", yu_bias=1.0, gate_bias=1.0)
    model = picnn.FCModel(spec, p0, "cpu")
    assert model.c_ctx is not None and model.c_ctx.w_stage[0]
    p1 = {k: (v * 1.5).astype(np.float32) for k, v in p0.items()}
    model.repack(p1)
    assert model.c_ctx is not None, "repack() left the context weights unset"
    W0 = picnn.stage_weights(spec, p1)[0][0]
    assert np.array_equal(model._ctx_keep[0].numpy(), W0)           # stage 0 of the NEW parameters
    assert model.c_ctx.w_stage[0] == model._ctx_keep[0].data_ptr()


@pytest.mark.parametrize("case,variant", [("maxaffine_n159", "dual"), ("maxaffine_n159_long", "dual"), ("action_box", "rl"),
                                          ("zero_gradient", "dual"), ("lse_n33", "rl")])
def test_fused_callback_replay_reconstructs_the_reference_sequence(case, variant):
    """icnn_amd.bundle_entropy._replay_callbacks rebuilds callback(t, f, y) / callback(t, f) of a fused solve from the
    slot arrays after the launch.  Host logic, checked on CPU: the oracle (pinned to the reference) runs a problem with a
    recording callback -- that IS the reference's sequence, lib/bundle_entropy_dual.py:144-145 -- then a state laid out the
    way the device leaves it (point and energy of iteration t in slot t, samples that left the loop keep their iterate) is
    replayed: same number of calls, same energies, same iterates.  Cases with rank-test finishes (every sample of
    maxaffine leaves early), stall-rule finishes (rl) and zero gradients."""
    import types
    from icnn_amd import _lib, bundle_entropy
    from oracle import bundle_entropy_oracle as oracle
    factory, n_iter = problems.GOLDEN_CASES[case]
    prob = factory()
    seen = []

    def rec(t, f, y=None):
        seen.append((t, np.array(f, copy=True), None if y is None else np.array(y, copy=True)))

    with np.errstate(all="ignore"):
        ora = oracle.solve_batch(prob.fg, prob.y0(), n_iter, callback=rec, variant=variant)
    B, T = prob.B, n_iter
    filled_last = np.array([np.max(np.nonzero(np.any(ora.ys[u] != 0, axis=1))[0]) for u in range(B)])
    done = np.asarray(ora.finished, dtype=bool)
    if variant == "rl":
        t_next = filled_last + 1
    else:
        t_next = np.where(done, filled_last, T)
    fvals = np.zeros((B, T))
    for t, f, _ in seen:
        take = t <= filled_last
        fvals[take, t] = np.asarray(f, dtype=np.float64)[take]
    state = types.SimpleNamespace(
        B=B, T=T, fvals=torch.from_numpy(fvals), ys=torch.from_numpy(ora.ys), y=torch.from_numpy(ora.y),
        t_next=torch.from_numpy(t_next.astype(np.int32)), finished=torch.from_numpy(done.astype(np.int32)),
        G=torch.zeros(1, dtype=torch.float64 if ora.G.dtype == np.float64 else torch.float32),
        c_state=types.SimpleNamespace(flags=0))
    got = []

    def rec2(t, f, y=None):
        got.append((t, np.array(f, copy=True), None if y is None else np.array(y, copy=True)))

    bundle_entropy._replay_callbacks(state, rec2, variant, lambda yy: torch.from_numpy(np.asarray(prob.fg(yy.numpy().copy())[0])))
    assert [g[0] for g in got] == [s[0] for s in seen], "number / order of the calls"
    for (t, f, y), (_, f2, y2) in zip(seen, got):
        assert f2.dtype == np.asarray(f).dtype and np.array_equal(np.asarray(f), f2), "energies of iteration %d" % t
        assert (y is None) == (y2 is None)
        if y is not None:
            assert np.array_equal(y, y2), "iterates of iteration %d" % t
    if case == "maxaffine_n159_long":
        assert done.any(), "the case is meant to contain samples that leave the loop early"


def test_profiling_variant_is_a_separate_library():
    """The diagnostic laps behind icnn_be_debug_profile* live in csrc/prof/libicnn_be.so (-DICNN_BE_PROF=1), not in the
    production library: the build knows both targets and the binding can be pointed at the profiling one before loading."""
    import inspect
    from icnn_amd import _lib, build
    assert build.PROF_LIB != build.LIB and os.path.dirname(build.PROF_LIB) == build.PROF_DIR
    assert "prof" in inspect.signature(build.build).parameters
    assert callable(_lib.use_profiling_build)
    src = open(os.path.join(os.path.dirname(build.LIB), "be_common.h")).read()
    assert "#define ICNN_BE_PROF 0" in src, "the production build must not carry the laps"


def test_ragged_lists_of_the_reference_tuple_are_lists_built_on_demand():
    """A, b, xs, lam of BundleResult.as_reference_tuple (lib/bundle_entropy_dual.py:179): `list`s of B per-sample entries over
    one packed host array, built in one bulk pass on first use -- through every route the reference's call sites take
    (multi-label-cls/icnn_ebundle.py:235, :300-307; completion/icnn_ebundle.py:319-328) and the ones Python offers besides --
    and plain lists (no overridden method) from then on."""
    import copy
    import pickle
    from icnn_amd.bundle_entropy import _BuiltList, _RaggedList
    rows = np.arange(20.0, dtype=np.float32).reshape(10, 2)
    offs, B = [0, 3, 3, 7, 10], 4
    built = []

    def make():
        def all_of_them():
            built.append(1)
            return [list(rows[offs[u]:offs[u + 1]]) for u in range(B)]
        return _RaggedList(B, all_of_them)

    A = make()
    assert isinstance(A, list) and len(A) == B and built == [] and type(A) is _RaggedList
    assert len(A[2]) == 4 and isinstance(A[2], list) and A[2][1].dtype == np.float32 and np.array_equal(A[2][1], [8.0, 9.0])
    assert type(A) is _BuiltList and "__getitem__" not in vars(_BuiltList) and A[2] is A[2] and built == [1]
    assert len(A[-1]) == 3 and len(A[1]) == 0 and built == [1]
    assert [len(a) for a in make()] == [3, 0, 4, 3]                        # icnn_ebundle.py:235
    assert np.array(make()[0]).shape == (3, 2)                             # :300
    plain = pickle.loads(pickle.dumps(make()))
    assert type(plain) is list and [len(a) for a in plain] == [3, 0, 4, 3]
    assert type(copy.deepcopy(make())) is list and len(copy.copy(make())[2]) == 4
    assert [len(a) for a in make()[1:3]] == [0, 4] and len(make() + [[]]) == 5
    assert np.array(make(), dtype=object).shape == (4,)
    for a, c in zip(make(), make()):
        assert len(a) == len(c)
    with pytest.raises(IndexError):
        make()[4]
    grown = make()
    grown.append([])
    assert len(grown) == 5 and len(grown[2]) == 4
    assert _RaggedList(0, lambda: []) == [] and len(_RaggedList(0, lambda: [])) == 0
    lam = _RaggedList(2, lambda: [None, np.ones(2)])
    assert lam[0] is None and lam[1].shape == (2,)


def test_models_state_entries_that_the_header_declares():
    """Callers build every C entry name from what the model CLASS states (solve_entry, gd_entry, grad_floats_entry, the
    stems grad_entry and context_entry plus the suffixes train.surrogate_grad / surrogate_work_floats and context append):
    each is an export include/icnn_be.h declares.  No device, no instance."""
    from icnn_amd import ficnn, picnn
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    declared = set(re.findall(r"ICNN_BE_API\s+[\w\s\*]+?\b(icnn_be_\w+)\s*\(", header))
    picnn_grad = ("_bn", "_dev", "_work_floats", "_dev_work_floats")
    picnn_ctx = ("", "_bn", "_bn_dev", "_work_floats", "_bn_work_floats")
    for cls, grad, ctx in ((picnn.FCModel, picnn_grad, picnn_ctx), (picnn.ConvModel, picnn_grad, picnn_ctx),
                           (ficnn.FICNNModel, ("", "_work_floats"), None)):
        names = [cls.solve_entry, cls.gd_entry, cls.grad_floats_entry] + [cls.grad_entry + s for s in grad]
        if ctx is not None:
            names += [cls.context_entry + s for s in ctx]
        for name in names:
            assert name in declared, (cls.__name__, name)
    assert len({picnn.FCModel.grad_entry, picnn.ConvModel.grad_entry, ficnn.FICNNModel.grad_entry}) == 3


def test_grad_layout_of_each_spec_kind_follows_its_init_params():
    """train.grad_layout stays a function of the spec, whichever module keeps the spec's layout: names in the key order of
    the init function, shapes those of its arrays."""
    from icnn_amd import ficnn, picnn, train
    for spec, params in ((picnn.bibtex_spec(), picnn.init_params(picnn.bibtex_spec())),
                         (picnn.ConvSpec(), picnn.init_conv_params(picnn.ConvSpec())),
                         (ficnn.synthetic_spec(), ficnn.init_params(ficnn.synthetic_spec()))):
        assert train.grad_layout(spec) == [(k, tuple(v.shape)) for k, v in params.items()], type(spec).__name__


def test_trainers_start_point_forms():
    """train._start_point, the one normaliser behind BundleTrainer.set_y0 and ConvGDTrainer.set_y0: a scalar comes back as
    a Python float, every other accepted form as a float64 tensor that expands to the rows the trainers copy from it."""
    from icnn_amd import train
    H, W, B, E = 4, 2, 3, 5
    n = H * W
    rng = np.random.RandomState(0)
    cpu = torch.device("cpu")
    assert train._start_point(0.25, n, B, E, cpu) == 0.25 and isinstance(train._start_point(np.float32(0.5), n, B, None, cpu), float)
    row, rows = rng.rand(n), rng.rand(B, n)
    for given, want, eval_batch in ((row, row, E), (row.reshape(1, n), row, E), (row.reshape(H, W, 1), row, E),
                                    (row.astype(np.float32), row.astype(np.float32).astype(np.float64), None),
                                    (rows, rows, B), (rows, rows, None), (rows.reshape(B, H, W, 1), rows, B),
                                    (torch.from_numpy(rows), rows, B)):
        got = train._start_point(given, n, B, eval_batch, cpu)
        assert torch.is_tensor(got) and got.dtype == torch.float64 and got.dim() == want.ndim
        for count in (B, eval_batch or B):
            assert np.array_equal(got.expand(count, n).numpy(), np.broadcast_to(want, (count, n)))
    for bad, eval_batch in ((rng.rand(n + 1), None), (rng.rand(B + 1, n), None), (rng.rand(B + 1, H, W, 1), None),
                            (rng.rand(2, B, n + 1), None), (rows, E), (rows.reshape(B, H, W, 1), E)):
        with pytest.raises(ValueError):
            train._start_point(bad, n, B, eval_batch, cpu)
