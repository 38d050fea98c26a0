"""The three kernels of be_train_epoch.hip on the device: icnn_be_gd_eval against icnn_be_gd_feed and the
loss-only form of icnn_be_gd_feed_px at px = 1, icnn_be_macro_f1 against train.macro_f1, icnn_be_keep_best against a Python
restatement of the scripts' rule, with a gated copy behind it as the snapshot."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

PAD = -7


def _lib():
    from icnn_amd import _lib
    return _lib, _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ticket(n_bytes):
    return torch.zeros((int(n_bytes) + 7) // 8, dtype=torch.float64, device="cuda")


def _feed_problem(B, n, seed=0):
    """y_K as float64 holding float32 values on both sides of 0.5 (some exactly 0.5), 0/1 targets with a few other values"""
    rng = np.random.RandomState(seed + 31 * B + n)
    y = rng.rand(B, n).astype(np.float32)
    y[rng.rand(B, n) < 0.1] = 0.5
    t = (rng.rand(B, n) < 0.4).astype(np.float32)
    t[rng.rand(B, n) < 0.05] = 0.25                     # (int)t == 0: counted as a negative
    return torch.from_numpy(y.astype(np.float64)).cuda(), torch.from_numpy(t).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("B,n", [(1, 1), (7, 16), (4, 159), (600, 5)])
def test_gd_eval_has_the_feeds_bits(B, n):
    _l, lib = _lib()
    K = 3
    y, t = _feed_problem(B, n)
    coef = torch.tensor([-0.03, -0.02, -0.01], dtype=torch.float64, device="cuda")
    scale = float(np.float32(1.0) / np.float32(B * n))
    # ---- the feed, with throw-away rows ----
    v = torch.empty(B * K, n, dtype=torch.float64, device="cuda")
    c = torch.empty(B * K, dtype=torch.float64, device="cuda")
    off = torch.empty(B + 1, dtype=torch.int32, device="cuda")
    loss_feed = torch.full((), float(PAD), dtype=torch.float32, device="cuda")
    tal_feed = torch.full((B, 3), PAD, dtype=torch.int32, device="cuda")
    work_feed = _ticket(lib.icnn_be_gd_feed_work_bytes(B))
    _l.check(lib.icnn_be_gd_feed(y.data_ptr(), t.data_ptr(), coef.data_ptr(), B, n, K, scale, v.data_ptr(), c.data_ptr(),
                                 off.data_ptr(), loss_feed.data_ptr(), tal_feed.data_ptr(), work_feed.data_ptr(), _stream()),
             "icnn_be_gd_feed")
    # ---- the px feed's loss-only form at px = 1 ----
    loss_px = torch.full((), float(PAD), dtype=torch.float32, device="cuda")
    work_px = _ticket(lib.icnn_be_gd_feed_px_work_bytes(B, n, K))
    _l.check(lib.icnn_be_gd_feed_px(y.data_ptr(), t.data_ptr(), None, B, n, K, scale, 1.0, None, None, None, loss_px.data_ptr(),
                                    work_px.data_ptr(), _stream()), "icnn_be_gd_feed_px")
    # ---- the loss-only entry: its outputs sit inside buffers prefilled with PAD ----
    loss_buf = torch.full((5,), float(PAD), dtype=torch.float32, device="cuda")
    tal_buf = torch.full((B + 2, 3), PAD, dtype=torch.int32, device="cuda")
    y_before, t_before = y.clone(), t.clone()
    work = _ticket(lib.icnn_be_gd_eval_work_bytes(B))
    work_len = work.numel()

    def run(tallies):
        _l.check(lib.icnn_be_gd_eval(y.data_ptr(), t.data_ptr(), B, n, loss_buf[2:3].data_ptr(),
                                     tal_buf[1:B + 1].data_ptr() if tallies else None, work.data_ptr(), _stream()),
                 "icnn_be_gd_eval")
        torch.cuda.synchronize()
    run(False)                                          # without tallies: the loss alone
    assert torch.equal(loss_buf[2], loss_feed) and bool((tal_buf == PAD).all())
    assert int(work.view(torch.int32)[2 * B].item()) == 0            # the ticket is re-armed
    first = loss_buf.clone()
    run(True)
    assert torch.equal(loss_buf, first)                 # the same bits on a second call
    assert torch.equal(loss_buf[2], loss_feed) and torch.equal(loss_buf[2], loss_px)
    assert bool((loss_buf[[0, 1, 3, 4]] == PAD).all())
    assert torch.equal(tal_buf[1:B + 1], tal_feed)
    assert bool((tal_buf[0] == PAD).all()) and bool((tal_buf[B + 1] == PAD).all())
    assert torch.equal(y, y_before) and torch.equal(t, t_before) and work.numel() == work_len
    # the values are what the contract says, not merely equal to each other
    d = y.to(torch.float32) - t
    want = float((d.double() * d.double()).sum().item() / (B * n))
    assert abs(float(loss_feed.item()) - want) <= 2.0 ** -23 * want + 1e-45
    yh, th = y.cpu().numpy(), t.cpu().numpy()
    pred, truth = yh >= 0.5, th.astype(np.int32) != 0
    tallies = np.stack([(pred & truth).sum(1), (pred & ~truth).sum(1), (~pred & truth).sum(1)], 1)
    assert np.array_equal(tal_feed.cpu().numpy(), tallies)


def _tallies(B, seed=0):
    """rows with a zero denominator, rows with tp = 0 and a non-zero denominator, one row of large counts"""
    rng = np.random.RandomState(seed + B)
    t = rng.randint(0, 40, size=(B, 3)).astype(np.int32)
    t[rng.rand(B) < 0.2] = 0
    t[rng.rand(B) < 0.2, 0] = 0
    if B >= 3:
        t[0] = (0, 0, 0)
        t[1] = (0, 3, 4)
    t[B - 1] = (1_000_000_007, 999_999_937, 2_000_000_011)          # 2 tp + fp + fn is beyond int32
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 257, 5000])
def test_macro_f1_equals_the_host_function(B):
    from icnn_amd import train
    _l, lib = _lib()
    host = _tallies(B)
    dev = torch.from_numpy(host).cuda()
    out = torch.full((3,), float(PAD), dtype=torch.float64, device="cuda")

    def run():
        _l.check(lib.icnn_be_macro_f1(dev.data_ptr(), B, out[1:2].data_ptr(), _stream()), "icnn_be_macro_f1")
        torch.cuda.synchronize()
        return out.clone()
    first = run()
    want = train.macro_f1(host)
    got = float(first[1].item())
    print("B = %d: device %.17g, host %.17g, difference %.3g, bound %.3g" % (B, got, want, abs(got - want), B * 2.0 ** -52))
    assert 0.0 < want < 1.0 or B == 1
    assert abs(got - want) <= B * 2.0 ** -52
    assert float(first[0]) == PAD and float(first[2]) == PAD
    assert torch.equal(run(), first)                    # the same bits on a second call
    assert np.array_equal(dev.cpu().numpy(), host)
    # all-zero tallies: every denominator is zero
    zeros = torch.zeros(B, 3, dtype=torch.int32, device="cuda")
    _l.check(lib.icnn_be_macro_f1(zeros.data_ptr(), B, out[1:2].data_ptr(), _stream()), "icnn_be_macro_f1")
    assert float(out[1].item()) == 0.0


def _rule(mode, best, score):
    """the scripts' rule: strictly better, and a NaN never is"""
    if math.isnan(score):
        return False, best
    better = score > best if mode == "max" else score < best
    return (True, score) if better else (False, best)


OFFERS = [0.25, 0.5, 0.5, 0.375, float("nan"), 0.75, float("-inf"), float("inf"), float("inf"), 0.125, float("-inf"),
          float("nan"), -3.0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["max", "min"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("start", [None, 0.3], ids=["open", "start"])
def test_keep_best_follows_the_scripts_rule(mode, dtype, start):
    _l, lib = _lib()
    first = start if start is not None else (-math.inf if mode == "max" else math.inf)
    best = torch.tensor([PAD, first, PAD], dtype=torch.float64, device="cuda")
    gate = torch.zeros(5, dtype=torch.int32, device="cuda")
    gate[0] = gate[4] = PAD
    live = torch.zeros(300, dtype=torch.float32, device="cuda")
    snap = torch.full((300,), float(PAD), dtype=torch.float32, device="cuda")
    score = torch.zeros(1, dtype=dtype, device="cuda")
    want_best, offers, kept, want_snap = first, 0, 0, float(PAD)
    gos = []
    for i, s in enumerate(OFFERS):
        score.fill_(s)
        live.fill_(float(i + 1))
        _l.check(lib.icnn_be_keep_best(score.data_ptr(), int(dtype == torch.float64), _l.KEEP_MODE[mode], best[1:2].data_ptr(),
                                       gate[1:4].data_ptr(), _stream()), "icnn_be_keep_best")
        _l.check(lib.icnn_be_gated_copy(snap.data_ptr(), live.data_ptr(), live.numel(), gate[1:2].data_ptr(), 1, _stream()),
                 "icnn_be_gated_copy")
        torch.cuda.synchronize()
        go, want_best = _rule(mode, want_best, s)
        offers, kept = offers + 1, kept + int(go)
        want_snap = float(i + 1) if go else want_snap
        gos.append(go)
        assert gate.cpu().tolist() == [PAD, int(go), offers, kept, PAD], (i, s)
        b = best.cpu().tolist()
        assert b[0] == PAD and b[2] == PAD and b[1] == want_best, (i, s)
        assert bool((snap == want_snap).all()), (i, s)
        assert float(score.item()) == s or math.isnan(s)
    assert any(gos) and not all(gos)
    assert not gos[2] and not gos[4] and not gos[11]              # the exact tie and the NaNs
