"""Exploration on the device (icnn_be_explore, rl_agent.Explorer) against tests/vec_replay_ref.py.

Exact bits wherever no transcendental is involved: test=True (clip only; noise and counter untouched), the reset mask, the
counter under graph replay, both input dtypes, and the noise recurrence itself -- with theta = 0, sigma = 1 and zero noise
one launch leaves noise = 0 - (0 * 0 - 1 * z) = z exactly, so the device's own deviates can be read out and the recurrence
noise <- noise - (theta * noise - sigma * z), action = clip(raw + noise) restated in NumPy on THEM must agree bit for bit.

The deviates against the float64 NumPy restatement and against x87 extended precision (log, sqrt and cos on the same float64
uniforms and the same float64 angle): the device's log and cos differ from the host's by a few ULP.  Measured on the MI355X over
2^16 deviates: worst relative difference 4.232e-16 against NumPy, 3.138e-16 against extended precision (NumPy's own float64
against extended precision: 3.138e-16); the bound Z_REL is 8 x the larger, 3.4e-15, and would never be set above 1e-12.
A float32 constant or intermediate is an error of 1e-8 or more (test_a_float32_two_pi_is_far_outside_the_bound).

Moments on 2^16 deviates at 6 sigma of their sampling distributions: mean 0 +- 6 / sqrt(N), variance 1 +- 6 sqrt(2 / N),
third moment 0 +- 6 sqrt(15 / N), fourth moment 3 +- 6 sqrt(96 / N)."""
import ctypes as C

import numpy as np
import pytest
import torch

import replay_ref
import vec_replay_ref as ref
from icnn_amd import _lib, rl_agent

Z_REL = 8 * 4.232e-16            # 3.4e-15 (module docstring)
N_MOMENTS = 1 << 16


# ------------------------------------------------------------------------------------------------ CPU


def test_vector_philox_is_the_scalar_one():
    c = np.array([[0, 0, 0, 3], [7, 1023, 64, 3], [0xFFFFFFFF, 5, 2, 3], [123456789, 0, 1, 0]], np.uint64)
    for seed in (0, 5, (0xDEADBEEF << 32) | 0x12345678):
        words = ref.philox_words(c[:, 0], c[:, 1], c[:, 2], c[:, 3], seed)
        for r, row in enumerate(c):
            want = replay_ref.philox4x32_10([int(v) for v in row], (seed & replay_ref.MASK, seed >> 32))
            assert tuple(int(w[r]) for w in words) == want


def test_uniforms_keep_the_logarithm_finite():
    u1, u2 = ref.uniforms(3, 1024, 64, 9)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0
    assert (np.uint64(0xFFFFFFFFFFFFFFFF) >> np.uint64(11)) + np.uint64(1) == np.uint64(1 << 53)     # the largest u1 is exactly 1
    z = ref.normals(3, 1024, 64, 9)
    assert np.all(np.isfinite(z)) and z.dtype == np.float64


def test_a_float32_two_pi_is_far_outside_the_bound():
    """what a float32 constant does to the deviates: 1e-8 or more, four decades beyond anything Z_REL may be"""
    u1, u2 = ref.uniforms(0, 256, 64, 1)
    z = ref.normals(0, 256, 64, 1)
    z32 = np.sqrt(-2.0 * np.log(u1)) * np.cos(np.float64(np.float32(ref.TWO_PI)) * u2)
    big = np.abs(z) > 0.1
    assert np.max(np.abs(z32[big] - z[big]) / np.abs(z[big])) > 1e-8 and Z_REL <= 1e-12


def test_bad_arguments_are_rejected_before_launch():
    lib = _lib.load()

    def call(E=3, dimA=2, raw=512, f32=0, noise=1024, counter=2048, theta=0.15, sigma=0.1, action=4096):
        return lib.icnn_be_explore(E, dimA, raw, f32, noise, counter, theta, sigma, 5, 0, action, None)
    for kw in (dict(E=0), dict(dimA=0), dict(raw=None), dict(noise=None), dict(counter=None), dict(action=None), dict(raw=516),
               dict(raw=514, f32=1), dict(noise=1028), dict(counter=2050), dict(action=4100), dict(theta=float("nan")),
               dict(sigma=float("nan"))):
        assert call(**kw) == -1, kw
    assert call(E=1 << 20, dimA=1 << 12) == -2
    with pytest.raises(ValueError):
        rl_agent.Explorer(0, 2, device="cpu")


# ------------------------------------------------------------------------------------------------ GPU


def _device_normals(E, dimA, seed, step):
    """the device's own z(step): theta = 0, sigma = 1, zero noise (module docstring)"""
    ex = rl_agent.Explorer(E, dimA, 0.0, 1.0, "cuda", seed)
    ex.counter.fill_(step)
    ex.step(torch.zeros(E, dimA, dtype=torch.float64, device="cuda"))
    return ex.noise.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_test_mode_clips_and_touches_nothing(dtype):
    big = 1e300 if dtype == torch.float64 else 3e38
    raw = np.array([[big, -big, 1.0, -1.0, 0.3], [1.0000001, -1.0000001, 0.0, -0.0, -0.99999]])
    raw = torch.tensor(raw, dtype=dtype, device="cuda")
    ex = rl_agent.Explorer(2, 5, device="cuda", seed=4)
    ex.noise.copy_(torch.from_numpy(np.random.RandomState(0).randn(2, 5)))
    ex.counter.fill_(17)
    before = ex.noise.clone()
    got = ex.step(raw, test=True).cpu().numpy()
    want = np.clip(raw.cpu().numpy().astype(np.float64), -1.0, 1.0)
    assert got.dtype == np.float64 and np.array_equal(got, want) and got.max() == 1.0 and got.min() == -1.0
    assert torch.equal(ex.noise, before) and int(ex.counter.item()) == 17


@pytest.mark.gpu
def test_reset_mask_zeroes_those_rows_only():
    E, dimA = 5, 3
    ex = rl_agent.Explorer(E, dimA, device="cuda", seed=2)
    raw = torch.zeros(E, dimA, dtype=torch.float64, device="cuda")
    ex.step(raw)
    ex.step(raw)
    before = ex.noise.cpu().numpy().copy()
    assert np.all(before != 0.0)
    mask = np.array([False, True, False, False, True])
    ex.reset(mask)
    after = ex.noise.cpu().numpy()
    assert np.array_equal(after[~mask], before[~mask]) and not after[mask].any() and int(ex.counter.item()) == 2
    # the next step: a restarted environment's noise is sigma * z alone, the others carry on
    z = _device_normals(E, dimA, 2, 2)
    ex.step(raw)
    want_action, want_noise = ref.explore(np.zeros((E, dimA)), after, z, ex.theta, ex.sigma)
    assert np.array_equal(ex.noise.cpu().numpy(), want_noise) and np.array_equal(ex.action.cpu().numpy(), want_action)
    assert np.array_equal(want_noise[mask], (0.0 - (ex.theta * 0.0 - ex.sigma * z))[mask])
    ex.reset()
    assert not ex.noise.any()


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_noise_recurrence_and_counter_under_graph_replay(dtype):
    """three replays of one captured launch are steps 1, 2, 3 of the recurrence on the device's own deviates, bit for bit;
    raw is scaled so that some actions clip"""
    E, dimA, seed = 3, 6, 21
    raw = torch.tensor(np.random.RandomState(1).randn(E, dimA) * 0.8, dtype=dtype, device="cuda")
    ex = rl_agent.Explorer(E, dimA, 0.15, 0.1, "cuda", seed)
    zs = [_device_normals(E, dimA, seed, s) for s in range(4)]
    assert not np.array_equal(zs[0], zs[1])
    noise = np.zeros((E, dimA))
    ex.step(raw)                                                         # eager, step 0
    want, noise = ref.explore(raw.cpu().numpy(), noise, zs[0], 0.15, 0.1)
    assert np.array_equal(ex.action.cpu().numpy(), want) and np.array_equal(ex.noise.cpu().numpy(), noise)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ex.step(raw)
    assert int(ex.counter.item()) == 1                                   # the capture launched nothing
    clipped = 0
    for s in (1, 2, 3):
        g.replay()
        want, noise = ref.explore(raw.cpu().numpy(), noise, zs[s], 0.15, 0.1)
        assert np.array_equal(ex.noise.cpu().numpy(), noise) and np.array_equal(ex.action.cpu().numpy(), want)
        assert int(ex.counter.item()) == s + 1
        clipped += int((np.abs(want) == 1.0).sum())
    assert clipped > 0


@pytest.mark.gpu
def test_deviates_against_the_restatement_and_extended_precision():
    assert np.finfo(np.longdouble).nmant >= 63, "needs x87 extended precision for the reference values"
    E, dimA, seed, step = 1024, 64, 9, 3
    z = _device_normals(E, dimA, seed, step)
    z64 = ref.normals(step, E, dimA, seed)
    zL = ref.normals(step, E, dimA, seed, np.longdouble)
    assert np.all(zL != 0)
    rel64 = float(np.max(np.abs(z - z64) / np.abs(z64)))
    relL = float(np.max(np.abs((z.astype(np.longdouble) - zL) / zL)))
    host = float(np.max(np.abs((z64.astype(np.longdouble) - zL) / zL)))
    print("z over %d deviates: worst relative difference %.3e against NumPy float64, %.3e against extended precision "
          "(NumPy float64 itself: %.3e); bound %.3e" % (z.size, rel64, relL, host, Z_REL))
    assert Z_REL <= 1e-12
    assert rel64 <= Z_REL and relL <= Z_REL
    # the noise after three steps against the restatement on ITS deviates: every step adds sigma * z, so the difference is
    # bounded by Z_REL times the sum of sigma * |z| (the decay 1 - theta only shrinks earlier terms)
    ex = rl_agent.Explorer(E, dimA, 0.15, 0.1, "cuda", seed)
    raw = torch.zeros(E, dimA, dtype=torch.float64, device="cuda")
    noise, scale = np.zeros((E, dimA)), np.zeros((E, dimA))
    for s in range(3):
        ex.step(raw)
        zs = ref.normals(s, E, dimA, seed)
        _, noise = ref.explore(np.zeros((E, dimA)), noise, zs, 0.15, 0.1)
        scale += 0.1 * np.abs(zs)
    err = float(np.max(np.abs(ex.noise.cpu().numpy() - noise) / scale))
    print("noise after 3 steps: worst difference %.3e of the accumulated sigma * |z|" % err)
    assert err <= Z_REL


@pytest.mark.gpu
def test_moments_of_the_deviates():
    z = _device_normals(1024, 64, 31, 0).ravel()
    N = z.size
    assert N == N_MOMENTS
    m1, m2, m3, m4 = (float(np.mean(z ** p)) for p in (1, 2, 3, 4))
    print("N = %d: mean %.4f, second moment %.4f, third %.4f, fourth %.4f" % (N, m1, m2, m3, m4))
    assert abs(m1) <= 6.0 / np.sqrt(N)
    assert abs(m2 - 1.0) <= 6.0 * np.sqrt(2.0 / N)
    assert abs(m3) <= 6.0 * np.sqrt(15.0 / N)
    assert abs(m4 - 3.0) <= 6.0 * np.sqrt(96.0 / N)
    # neighbouring environments, components and steps are other numbers
    assert len(np.unique(z)) == N and not np.array_equal(z, _device_normals(1024, 64, 31, 1).ravel())
