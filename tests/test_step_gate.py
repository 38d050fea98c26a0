"""The device words of a skipped training step: icnn_be_step_gate (be_train_bundle.hip) against its rule,
icnn_be_param_update_gated (be_train_update.hip) against icnn_be_param_update on a twin set of buffers, icnn_be_gated_copy
against torch, each also captured in a graph and replayed with the device word rewritten between replays.  Every comparison
is between a launch and its ungated form, or against integers: exact."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from icnn_amd import _lib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ["icnn_be_step_gate", "icnn_be_param_update_gated", "icnn_be_gated_copy"]
FULL = _lib.ST_SINGULAR | _lib.ST_NONFINITE | _lib.ST_UNFINISHED | _lib.ST_OVERFLOW
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8


# ------------------------------------------------------------------------------------------------ CPU


def test_gate_entries_are_exported_declared_and_bound():
    lib = _lib.load()
    header = open(os.path.join(REPO, "include", "icnn_be.h")).read()
    assert _lib.ABI_VERSION == 12 == lib.icnn_be_abi_version()
    for name in NEW_EXPORTS:
        assert re.search(r"\b%s\(" % name, header), name
        assert name in _lib.EXPORTS and hasattr(lib, name)
        fn = getattr(lib, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert len(lib.icnn_be_step_gate.argtypes) == 4
    assert len(lib.icnn_be_param_update_gated.argtypes) == 3
    assert len(lib.icnn_be_gated_copy.argtypes) == 6
    assert _lib.ST_ERROR_MASK == FULL == 15


def _plausible_update_args():
    """arguments icnn_be_param_update's checks accept (never launched: the pointers are made up)"""
    a = _lib.ParamUpdateArgs()
    a.n, a.theta, a.m, a.v, a.grad, a.dest_off, a.dest, a.arena, a.step = 4, 16, 32, 48, 64, 80, 96, 112, 128
    a.arena_floats, a.lr, a.beta1, a.beta2, a.eps = 8, LR, B1, B2, EPS
    return a


def test_gate_entries_reject_null_pointers_before_any_launch():
    lib = _lib.load()
    fake = C.c_void_p(64)
    assert lib.icnn_be_step_gate(None, FULL, fake, None) == -1             # NULL counts
    assert lib.icnn_be_step_gate(fake, FULL, None, None) == -1             # NULL gate
    assert lib.icnn_be_step_gate(None, FULL, None, None) == -1
    a = _plausible_update_args()
    assert lib.icnn_be_param_update_gated(C.byref(a), None, None) == -1    # NULL go, everything else acceptable
    assert lib.icnn_be_param_update_gated(None, fake, None) == -1
    a.grad = 66                                                            # what icnn_be_param_update refuses, with a go
    assert lib.icnn_be_param_update_gated(C.byref(a), fake, None) == -1
    a.grad, a.n = 64, 0
    assert lib.icnn_be_param_update_gated(C.byref(a), fake, None) == -1
    assert lib.icnn_be_gated_copy(fake, fake, 4, None, 0, None) == -1      # NULL go
    assert lib.icnn_be_gated_copy(None, fake, 4, fake, 0, None) == -1
    assert lib.icnn_be_gated_copy(fake, None, 4, fake, 0, None) == -1
    assert lib.icnn_be_gated_copy(fake, fake, -1, fake, 0, None) == -1
    assert lib.icnn_be_gated_copy(fake, fake, 0, fake, 0, None) == 0       # nothing to copy: nothing launched


# ------------------------------------------------------------------------------------------------ GPU: the gate


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gate(counts, mask, gate):
    _lib.check(_lib.load().icnn_be_step_gate(counts.data_ptr(), mask, gate.data_ptr(), _stream()), "icnn_be_step_gate")


def _ints(*v):
    return torch.tensor(v, dtype=torch.int32, device="cuda")


ONE_BIT = [_lib.ST_SINGULAR, _lib.ST_NONFINITE, _lib.ST_OVERFLOW, _lib.ST_UNFINISHED]


@pytest.mark.gpu
@pytest.mark.parametrize("bits", [0] + ONE_BIT + [_lib.ST_SINGULAR | _lib.ST_UNFINISHED])
def test_step_gate_follows_its_rule(bits):
    rows, folds = 17, 5
    counts = _ints(rows, folds, bits)
    masks = [FULL, FULL & ~bits] + [FULL & ~b for b in ONE_BIT if bits & b and bits != b]     # two bits: each one excluded alone
    gate = _ints(0, -3, 0)
    skipped = 0
    for mask in masks:
        go = int((bits & mask) == 0)
        skipped += 1 - go
        _gate(counts, mask, gate)
        assert gate.cpu().tolist() == [go, folds if go else 0, skipped], (bits, mask)
    assert counts.cpu().tolist() == [rows, folds, bits]                     # read only
    if bits:
        assert skipped == len(masks) - 1                                    # only the mask without the bits lets it go


@pytest.mark.gpu
def test_step_gate_counts_the_steps_that_did_not_go():
    gate = _ints(0, 0, 0)
    sequence = [0, _lib.ST_SINGULAR, 0, 0, _lib.ST_NONFINITE | _lib.ST_OVERFLOW, _lib.ST_UNFINISHED, 0, _lib.ST_OVERFLOW]
    for i, bits in enumerate(sequence):
        _gate(_ints(3 + i, 2 + i, bits), FULL, gate)
    torch.cuda.synchronize()
    assert gate.cpu().tolist() == [0, 0, sum(1 for b in sequence if b)]
    _gate(_ints(9, 4, 0), FULL, gate)                                       # a step that goes leaves the total alone
    assert gate.cpu().tolist() == [1, 4, sum(1 for b in sequence if b)]
    gate[2] = 40                                                            # the caller's to reset, never the kernel's
    _gate(_ints(9, 4, _lib.ST_SINGULAR), FULL, gate)
    assert gate.cpu().tolist() == [0, 0, 41]


@pytest.mark.gpu
def test_step_gate_captured_follows_rewritten_counts():
    counts, gate = _ints(11, 6, 0), _ints(0, 0, 0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _gate(counts, FULL, gate)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _gate(counts, FULL, gate)
    torch.cuda.synchronize()
    assert gate.cpu().tolist() == [1, 6, 0]                                 # the warm-up launch; capturing ran nothing
    want_skipped = 0
    for rows, folds, bits in ((5, 3, _lib.ST_NONFINITE), (8, 9, 0), (2, 1, _lib.ST_OVERFLOW)):
        counts.copy_(_ints(rows, folds, bits))
        graph.replay()
        go = int(bits == 0)
        want_skipped += 1 - go
        assert gate.cpu().tolist() == [go, folds if go else 0, want_skipped]
    assert want_skipped == 2


# ------------------------------------------------------------------------------------------------ GPU: the gated update


GUARD = 7                      # floats behind the arena the kernel may write, filled with a value it never produces
GUARD_VALUE = -777.0


class _Update:
    """buffers and arguments of one update over n floats: a map with zero, one and three copies per element and one entry
    beyond arena_floats, two proj ranges of which one is empty"""

    def __init__(self, n, seed):
        rng = np.random.RandomState(seed)
        copies = np.array([(0, 1, 3)[j % 3] for j in range(n)])
        copies[-1] += 2                                                    # the last element: a copy inside, one beyond
        off = np.concatenate([[0], np.cumsum(copies)]).astype(np.int32)
        self.arena_floats = int(off[-1]) + 3
        dest = rng.permutation(self.arena_floats)[:off[-1]].astype(np.int32)
        dest[-1] = self.arena_floats + 2                                   # inside the guard: the kernel must skip it
        cuda = lambda a: torch.from_numpy(a).cuda()                        # noqa: E731
        self.theta = cuda((1e-2 * rng.randn(n)).astype(np.float32))
        self.m = cuda((1e-3 * rng.randn(n)).astype(np.float32))
        self.v = cuda((1e-6 * rng.rand(n)).astype(np.float32))
        self.grad = cuda(rng.randn(n).astype(np.float32))
        self.dest_off, self.dest = cuda(off), cuda(dest)
        self.arena = torch.full((self.arena_floats + GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
        self.step = torch.zeros(2, dtype=torch.int32, device="cuda")
        a = _lib.ParamUpdateArgs()
        a.n, a.theta, a.m, a.v, a.grad = n, self.theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.grad.data_ptr()
        a.dest_off, a.dest, a.arena = self.dest_off.data_ptr(), self.dest.data_ptr(), self.arena.data_ptr()
        a.arena_floats, a.step = self.arena_floats, self.step.data_ptr()
        a.lr, a.beta1, a.beta2, a.eps = LR, B1, B2, EPS
        a.n_proj = 2
        a.proj_begin[0], a.proj_end[0] = 0, min(n, 3)
        a.proj_begin[1], a.proj_end[1] = n // 2, n // 2                    # empty
        self.args = a
        self.names = ("theta", "m", "v", "arena", "step")

    def plain(self):
        _lib.check(_lib.load().icnn_be_param_update(C.byref(self.args), _stream()), "icnn_be_param_update")

    def gated(self, go):
        _lib.check(_lib.load().icnn_be_param_update_gated(C.byref(self.args), go.data_ptr(), _stream()),
                   "icnn_be_param_update_gated")

    def clones(self):
        return {k: getattr(self, k).clone() for k in self.names}

    def same(self, other):
        other = other if isinstance(other, dict) else {k: getattr(other, k) for k in self.names}
        for k in self.names:
            assert torch.equal(getattr(self, k), other[k]), k
        assert bool((self.arena[self.arena_floats:] == GUARD_VALUE).all())


SIZES = [1, 5, 1027]           # one element; less than a vector; a block of 1024 and a ragged tail of 3


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gated_update_with_go_is_the_plain_update(n):
    a, twin = _Update(n, n), _Update(n, n)
    before = a.clones()
    a.gated(_ints(1))
    twin.plain()
    torch.cuda.synchronize()
    a.same(twin)
    assert a.step.cpu().tolist() == [1, 0]
    assert not torch.equal(a.theta, before["theta"]) and not torch.equal(a.arena, before["arena"])
    assert bool((a.theta[:min(n, 3)] >= 0).all())                          # proj
    a.gated(_ints(-5))                                                     # any non-zero word goes
    twin.plain()
    a.same(twin)
    assert a.step.cpu().tolist() == [2, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gated_update_without_go_changes_nothing_and_the_next_one_is_the_first(n):
    a, twin = _Update(n, 10 + n), _Update(n, 10 + n)
    before = a.clones()
    go = _ints(0)
    a.gated(go)
    a.gated(go)
    torch.cuda.synchronize()
    a.same(before)                                                         # theta, m, v, the guard-filled arena, both step words
    assert a.step.cpu().tolist() == [0, 0]
    go.fill_(1)
    a.gated(go)
    twin.plain()
    a.same(twin)
    assert a.step.cpu().tolist() == [1, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_gated_update_captured_with_go_flipped_between_replays(n):
    a, twin = _Update(n, 20 + n), _Update(n, 20 + n)
    go = _ints(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        a.gated(go)                                                        # the warm-up launch does not go
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a.gated(go)
    for word in (1, 0, 1):
        go.fill_(word)
        graph.replay()
    twin.plain()
    twin.plain()
    torch.cuda.synchronize()
    a.same(twin)
    assert a.step.cpu().tolist() == [2, 0]


# ------------------------------------------------------------------------------------------------ GPU: the gated copy


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES + [1024 * 256 + 3])                    # the last: more than one pass of the grid
def test_gated_copy_copies_exactly_when_the_word_matches(n):
    lib = _lib.load()
    src = torch.arange(1, n + 1, dtype=torch.float32, device="cuda")
    for word, want, copies in ((0, 0, True), (1, 0, False), (1, 1, True), (0, 1, False), (-2, 1, True), (6, 0, False)):
        dst = torch.full((n + GUARD,), GUARD_VALUE, dtype=torch.float32, device="cuda")
        _lib.check(lib.icnn_be_gated_copy(dst.data_ptr(), src.data_ptr(), n, _ints(word).data_ptr(), want, _stream()),
                   "icnn_be_gated_copy")
        assert torch.equal(dst[:n], src) == copies, (word, want)
        assert copies or bool((dst[:n] == GUARD_VALUE).all()), (word, want)
        assert bool((dst[n:] == GUARD_VALUE).all()), (word, want)


@pytest.mark.gpu
def test_gated_copy_captured_follows_the_word():
    lib, n = _lib.load(), 1027
    src = torch.arange(1, n + 1, dtype=torch.float32, device="cuda")
    dst = torch.zeros(n, dtype=torch.float32, device="cuda")
    go = _ints(1)

    def launch():
        _lib.check(lib.icnn_be_gated_copy(dst.data_ptr(), src.data_ptr(), n, go.data_ptr(), 0, _stream()), "icnn_be_gated_copy")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        launch()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    graph.replay()
    assert not dst.any()                                                   # go = 1, want = 0: left alone
    go.fill_(0)
    graph.replay()
    assert torch.equal(dst, src)
    dst.zero_()
    go.fill_(1)
    graph.replay()
    assert not dst.any()
