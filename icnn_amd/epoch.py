"""The epoch level of the supervised training scripts on the device; icnn_amd.train re-exports every name.

    BestKeeper      the scripts' "save when the score is better" on the device: icnn_be_keep_best (and icnn_be_macro_f1 for a
                    score formed from F1 tallies) sets a gate, icnn_be_gated_copy snapshots theta, the arena and the BatchNorm
                    statistics behind it (be_train_epoch.hip).  icnn_amd.checkpoint saves and resumes the
                    trainers.

    DeviceDataset   the training arrays on the device and the scripts' `I = npr.randint(nTrain, size=batch); trainX[I],
                    trainY[I]` as one launch (icnn_be_dataset_draw, be_train_data.hip); StepLog, the per-iteration scalars of
                    train.csv in a device ring (icnn_be_log_row); EpochRunner, [draw, step, log] x k captured once and replayed
                    (DESIGN.md §21).

The classes here name the trainers of train.py inside their methods, and train.py re-exports them: each module imports the
other behind its own definitions, so either may be imported first.
"""
import ctypes as C
import math
from typing import Dict

import numpy as np
import torch

from . import _lib
from .fcn import FCNTrainer
from .ff import FFTrainer
from .flat import _positive


# --------------------------------------------------------------------------------------------- #
# Keeping the best model on the device
# --------------------------------------------------------------------------------------------- #
class BestKeeper:
    """The scripts' "save when the score is better" without a host round trip (multi-label-cls/icnn_ebundle.py:274-277: `if
    testF1 > bestTestF1: save`, mode "max" with start=0.0; synthetic-cls/icnn.py:206-209: `bestMSE is None or trainMSE <
    bestMSE`, mode "min"), for any trainer that owns a DeviceAdam as `.opt` (BundleTrainer, GDTrainer,
    ConvGDTrainer, ficnn.GDTrainer, rl_train.CriticTrainer).

    offer(score) enqueues icnn_be_keep_best on a one-element float32 or float64 device tensor and, behind its gate,
    icnn_be_gated_copy of opt.theta, opt.arena and the model's BatchNorm moving statistics into snapshots: they change only
    on an offer that is STRICTLY better than `best`.  offer_macro_f1(tallies) first forms util.macroF1 on the device
    (icnn_be_macro_f1) into the keeper's own score word, so a captured [evaluate, offer_macro_f1(eval_f1_tallies)] keeps the
    best test-F1 model with no host data.  No host wait in either.

    start=None: -inf for "max", +inf for "min", so the first finite offer is kept.  One deviation from synthetic-cls:
    `bestMSE is None or ...` would keep a NaN first loss; the keeper never keeps a NaN (no comparison with a NaN is true).

    For a model with BatchNorm the constructor calls model.flatten_bn_stats(), which MOVES the statistics' addresses:
    construct the keeper before capturing anything that reads them (a BundleTrainer(skip_on_error=True) has moved them
    already).  The snapshots start as copies of the current state, so restore() before any kept offer puts that back.

    best (float64 [1]) is the device scalar; offers, kept and best_value() read the device (one wait each)."""

    def __init__(self, trainer, mode="max", start=None):
        if mode not in _lib.KEEP_MODE:
            raise ValueError("mode must be 'max' or 'min', got %r" % (mode,))
        opt = getattr(trainer, "opt", None)
        if not isinstance(opt, DeviceAdam):
            raise TypeError("BestKeeper serves a trainer that owns a DeviceAdam as .opt, got %s" % type(trainer).__name__)
        self.trainer, self.opt, self.model, self.mode = trainer, opt, opt.model, mode
        self.device = dev = opt.device
        self._lib = opt.model._lib
        if start is None:
            start = -math.inf if mode == "max" else math.inf
        self.start = float(start)
        self.best = torch.full((1,), self.start, dtype=torch.float64, device=dev)
        self.gate = torch.zeros(3, dtype=torch.int32, device=dev)                # go, offers, kept
        self.score = torch.zeros(1, dtype=torch.float64, device=dev)             # offer_macro_f1's score word
        self.theta = opt.theta.clone()
        self.arena = opt.arena.clone()
        self._bn_live = self.bn = None
        self._bn_views = {}
        if getattr(self.model, "has_bn", False) and self.model.bn_stats:     # a one-layer u-path normalises nothing
            self._bn_live = live = self.model.flatten_bn_stats()
            self.bn = live.clone()
            self._bn_views = {k: ((t.data_ptr() - live.data_ptr()) // 4, tuple(t.shape))
                              for k, t in self.model.bn_stats.items()}

    def _pairs(self):
        """(snapshot, live) of everything the keeper keeps"""
        pairs = [(self.theta, self.opt.theta), (self.arena, self.opt.arena)]
        if self.bn is not None:
            pairs.append((self.bn, self._bn_live))
        return pairs

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def offer(self, score):
        """Offer a one-element float32 or float64 device tensor; the snapshots follow when it is strictly better."""
        if (not torch.is_tensor(score) or score.numel() != 1 or not score.is_cuda
                or score.dtype not in (torch.float32, torch.float64)):
            raise ValueError("score is one float32 or float64 on the device")
        stream = self._stream()
        _lib.check(self._lib.icnn_be_keep_best(score.data_ptr(), int(score.dtype == torch.float64), _lib.KEEP_MODE[self.mode],
                                               self.best.data_ptr(), self.gate.data_ptr(), stream), "icnn_be_keep_best")
        for snap, live in self._pairs():
            _lib.check(self._lib.icnn_be_gated_copy(snap.data_ptr(), live.data_ptr(), live.numel(), self.gate.data_ptr(), 1,
                                                    stream), "icnn_be_gated_copy")

    def offer_macro_f1(self, tallies):
        """Offer util.macroF1 of per-example tallies (int32 [B, 3] on the device: a trainer's f1_tallies / eval_f1_tallies)."""
        if (not torch.is_tensor(tallies) or tallies.dtype != torch.int32 or not tallies.is_cuda or not tallies.is_contiguous()
                or tallies.dim() != 2 or tallies.shape[1] != 3 or tallies.shape[0] < 1):
            raise ValueError("tallies is a contiguous int32 [B, 3] device tensor, B >= 1")
        _lib.check(self._lib.icnn_be_macro_f1(tallies.data_ptr(), tallies.shape[0], self.score.data_ptr(), self._stream()),
                   "icnn_be_macro_f1")
        self.offer(self.score)

    @property
    def offers(self) -> int:
        """offers made (reads the device: one wait)"""
        return int(self.gate[1].item())

    @property
    def kept(self) -> int:
        """offers that were kept (reads the device: one wait)"""
        return int(self.gate[2].item())

    def best_value(self) -> float:
        """the best score so far, `start` before any was kept (reads the device: one wait)"""
        return float(self.best.item())

    def host_params(self) -> Dict[str, np.ndarray]:
        """the kept model's theta as a NumPy dict keyed like grad_layout (one copy; synchronises): what goes into best.npz"""
        flat = self.theta.cpu().numpy()
        return {name: t.numpy().copy() for name, t in unpack_grad(self.opt.spec, torch.from_numpy(flat)).items()}

    def bn_stats(self) -> Dict[str, np.ndarray]:
        """the kept model's BatchNorm moving statistics keyed like picnn.init_bn_stats ({} without BatchNorm; synchronises)"""
        if self.bn is None:
            return {}
        flat = self.bn.cpu().numpy()
        return {k: flat[off:off + int(np.prod(shape))].reshape(shape).copy() for k, (off, shape) in self._bn_views.items()}

    def restore(self):
        """Copy the snapshots back: theta, the arena and the statistics become the kept model's, on the device.  Adam's m, v
        and the step count are left alone."""
        for snap, live in self._pairs():
            live.copy_(snap)


# --------------------------------------------------------------------------------------------- #
# The training set on the device: minibatch draw, step log, epochs as a graph
# --------------------------------------------------------------------------------------------- #
class DeviceDataset:
    """The training arrays of the supervised scripts on the device, and their `I = npr.randint(nTrain, size=batch);
    trainX[I], trainY[I]` (multi-label-cls/icnn_ebundle.py:214, icnn-back.py:190, completion/icnn_ebundle.py:210,
    icnn.back.py:216) as one launch without a host wait (icnn_be_dataset_draw, be_train_data.hip).

    arrays: 1 to 4 tensors or ndarrays that share their first dimension N, typically (X float32 [N, *x_shape], Y [N, n]) with
    Y in the dtype of the trainer buffer it feeds (float64 for BundleTrainer.true_y, float32 for the GD trainers' t); they
    are copied into contiguous device tensors this object owns.  The draw copies rows bit for bit and knows no transform: the
    completion scripts' h-flip of x (completion/icnn_ebundle.py:215) is the same flip on every batch, so flip once when
    building the set.

    The indices follow npr.randint's rule -- independent, with replacement -- with this library's own random numbers:
    idx[k] = (word * N) >> 32 with word = word 0 of Philox4x32-10 at counter (draw, k, 0, 1) and key `seed`.  The draw
    counter lives on the device and every launch advances it, so a captured draw_into replayed r times is r different
    minibatches.  `draws` is its host mirror, deterministic and never read back: every draw_into call adds one, a capture's
    calls included; whoever replays a captured draw adds what the replay made (EpochRunner does)."""

    def __init__(self, arrays, device="cuda", seed=0):
        if torch.is_tensor(arrays) or isinstance(arrays, np.ndarray):
            arrays = (arrays,)
        arrays = tuple(arrays)
        if not 1 <= len(arrays) <= _lib.DATASET_MAX_ARRAYS:
            raise ValueError("a dataset holds 1 to %d arrays, got %d" % (_lib.DATASET_MAX_ARRAYS, len(arrays)))
        self.seed = int(seed)
        if not 0 <= self.seed < 1 << 64:
            raise ValueError("seed must fit 64 bits")
        self.device = dev = torch.device(device)
        self.lib = _lib.load()
        self.arrays, self.row_words = [], []
        for i, a in enumerate(arrays):
            a = torch.as_tensor(a)
            if a.dim() < 1 or a.shape[0] != torch.as_tensor(arrays[0]).shape[0]:
                raise ValueError("array %d: the arrays share their first dimension" % i)
            row_bytes = (a.numel() // max(a.shape[0], 1)) * a.element_size()
            if a.shape[0] < 1 or row_bytes < 4 or row_bytes % 4:
                raise ValueError("array %d: a dataset needs N >= 1 rows of whole 4-byte words, got shape %s of %s"
                                 % (i, tuple(a.shape), a.dtype))
            own = torch.empty(a.shape, dtype=a.dtype, device=dev)
            own.copy_(a)
            self.arrays.append(own)
            self.row_words.append(row_bytes // 4)
        self.n_rows = int(self.arrays[0].shape[0])
        if self.n_rows >= 1 << 31:
            raise ValueError("a dataset holds fewer than 2^31 rows")
        self.ctrl = torch.zeros(_lib.DATASET_CTRL_INTS, dtype=torch.int32, device=dev)
        d = _lib.Dataset()
        d.n_rows, d.n_arrays, d.ctrl = self.n_rows, len(self.arrays), self.ctrl.data_ptr()
        for i, (a, w) in enumerate(zip(self.arrays, self.row_words)):
            d.src[i], d.row_words[i] = a.data_ptr(), w
        self._c = d
        self._idx = {}                       # batch -> the int32 index buffer (fixed: a captured graph writes it)
        self.draws = 0

    def reset(self):
        """back to draw 0 with a clear status word"""
        self.ctrl.zero_()
        self.draws = 0

    def draw_into(self, *buffers) -> torch.Tensor:
        """One minibatch into `buffers`, one per array: contiguous tensors on the dataset's device, in the array's dtype,
        with the array's row size and a common first dimension B (a view of the first B rows of a larger buffer will do).
        Returns the drawn indices (int32 [B], a buffer of this dataset that the next draw at this batch size overwrites).
        One launch on the current stream, no host wait (capturable)."""
        if len(buffers) != len(self.arrays):
            raise ValueError("the dataset holds %d arrays, got %d buffers" % (len(self.arrays), len(buffers)))
        B = None
        for i, (buf, a, w) in enumerate(zip(buffers, self.arrays, self.row_words)):
            if not torch.is_tensor(buf) or buf.device != a.device:
                raise ValueError("buffer %d: not a tensor on %s" % (i, a.device))
            if buf.dtype != a.dtype or not buf.is_contiguous():
                raise ValueError("buffer %d: a contiguous %s tensor is needed, got %s" % (i, a.dtype, buf.dtype))
            if buf.dim() < 1 or buf.shape[0] < 1 or buf.numel() != buf.shape[0] * (a.numel() // self.n_rows):
                raise ValueError("buffer %d: rows of %d elements are needed, got shape %s"
                                 % (i, a.numel() // self.n_rows, tuple(buf.shape)))
            if B is not None and buf.shape[0] != B:
                raise ValueError("buffer %d: %d rows, the first buffer has %d" % (i, buf.shape[0], B))
            if buf.data_ptr() % 16:
                raise ValueError("buffer %d: not 16-byte aligned" % i)
            B = int(buf.shape[0])
        if B not in self._idx:
            self._idx[B] = torch.zeros(B, dtype=torch.int32, device=self.device)
        dst = (C.c_void_p * len(buffers))(*[b.data_ptr() for b in buffers])
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.icnn_be_dataset_draw(C.byref(self._c), B, self.seed, dst, self._idx[B].data_ptr(), stream),
                   "icnn_be_dataset_draw")
        self.draws += 1
        return self._idx[B]

    @property
    def status(self) -> int:
        """the device's status word, an OR of _lib.DATASET_ST_* (synchronises)"""
        return int(self.ctrl[1].item())

    def raise_on_error(self):
        """Raise if a launch so far met an error on the device (synchronises)."""
        st = self.status
        if st:
            raise RuntimeError("dataset: a draw found its ticket outside its grid -- two draws of one dataset ran at the "
                               "same time (status %d)" % st)


class StepLog:
    """The per-iteration scalars the scripts write to train.csv, kept on the device so that reading them needs no
    synchronisation per step (icnn_be_log_row, be_train_data.hip).  columns: up to 8 (name, tensor) with the
    tensor one float32, float64 or int32 on the device (a trainer's loss, rows, went ...); capacity: rows of the ring.
    append() is one launch, no host wait (capturable): it widens every scalar to float64 (exactly) into row cursor %
    capacity and advances the device cursor."""

    def __init__(self, columns, capacity):
        columns = list(columns)
        if not 1 <= len(columns) <= _lib.LOG_MAX_COLUMNS:
            raise ValueError("a step log has 1 to %d columns, got %d" % (_lib.LOG_MAX_COLUMNS, len(columns)))
        self.capacity = _positive("capacity", capacity)
        self.names = [str(name) for name, _ in columns]
        if len(set(self.names)) != len(self.names):
            raise ValueError("column names repeat: %s" % self.names)
        self.columns = [t for _, t in columns]
        L = _lib.StepLog()
        for j, t in enumerate(self.columns):
            kind = _lib.LOG_KIND.get(str(t.dtype).replace("torch.", "")) if torch.is_tensor(t) else None
            if kind is None or t.numel() != 1 or not t.is_cuda or t.device != self.columns[0].device:
                raise ValueError("column %r: one float32, float64 or int32 on the device is needed" % self.names[j])
            L.col[j], L.kind[j] = t.data_ptr(), kind
        self.device = dev = self.columns[0].device
        self.lib = _lib.load()
        self.rows = torch.zeros(self.capacity, len(columns), dtype=torch.float64, device=dev)
        self.ctrl = torch.zeros(_lib.LOG_CTRL_INTS, dtype=torch.int32, device=dev)
        L.rows, L.ctrl, L.cap, L.width = self.rows.data_ptr(), self.ctrl.data_ptr(), self.capacity, len(columns)
        self._c = L
        self._read = 0                       # rows handed out so far: the cursor at the last read()

    def append(self):
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        _lib.check(self.lib.icnn_be_log_row(C.byref(self._c), stream), "icnn_be_log_row")

    def read(self) -> Dict[str, np.ndarray]:
        """The rows appended since the last read(), in order, as name -> float64 array.  Synchronises the device.
        RuntimeError if more than `capacity` rows were appended since the last read(): the oldest were overwritten (the
        next read() starts behind them)."""
        torch.cuda.synchronize(self.device)
        cursor = int(self.ctrl[0].item())
        first, self._read = self._read, cursor
        if cursor - first > self.capacity:
            raise RuntimeError("step log: %d rows appended since the last read(), the ring keeps %d"
                               % (cursor - first, self.capacity))
        rows = self.rows.cpu().numpy()[np.arange(first, cursor, dtype=np.int64) % self.capacity]
        return {name: rows[:, j].copy() for j, name in enumerate(self.names)}


class EpochRunner:
    """`steps` iterations of [dataset.draw_into(*buffers), trainer.step(), log.append()] per run(), with no host wait inside:
    the first run() is eager, the second captures the chain once on a side stream and replays it, later runs replay
    (DESIGN.md §21).  After r runs the trainer's state is that of r x steps eager iterations bit for bit, whichever runs
    were eager, capturing or replays.  trainer: a BundleTrainer (FC or conv), GDTrainer, ConvGDTrainer, ff.FFTrainer or fcn.FCNTrainer; step() reads its
    buffers as step(None, None) does.  buffers: where the dataset's arrays go, by default (trainer.x, trainer.true_y) for a
    trainer that has true_y, else (trainer.x, trainer.t).  log: a StepLog, appended to after every step.

    With BundleTrainer(skip_on_error=True) a skipped step still consumes its draw, as the reference draws before its try."""

    def __init__(self, trainer, dataset, steps, log=None, buffers=None):
        if not isinstance(trainer, (BundleTrainer, GDTrainer, ConvGDTrainer, FFTrainer, FCNTrainer)):
            raise TypeError("EpochRunner serves BundleTrainer, GDTrainer, ConvGDTrainer, ff.FFTrainer and fcn.FCNTrainer, got %s"
                            % type(trainer).__name__)
        if not isinstance(dataset, DeviceDataset):
            raise TypeError("dataset is a train.DeviceDataset, got %s" % type(dataset).__name__)
        if log is not None and not isinstance(log, StepLog):
            raise TypeError("log is a train.StepLog, got %s" % type(log).__name__)
        self.trainer, self.dataset, self.log = trainer, dataset, log
        self.steps = _positive("steps", steps)
        if buffers is None:
            buffers = (trainer.x, trainer.true_y if hasattr(trainer, "true_y") else trainer.t)
        self.buffers = tuple(buffers)
        self.runs = 0
        self._graph = None

    def _chain(self):
        for _ in range(self.steps):
            self.dataset.draw_into(*self.buffers)
            self.trainer.step()
            if self.log is not None:
                self.log.append()

    def run(self):
        """`steps` iterations, enqueued on the current stream"""
        if self.runs == 0:
            self._chain()
            self.runs = 1
            return
        if self._graph is None:
            draws = self.dataset.draws
            s = torch.cuda.Stream(self.dataset.device)
            s.wait_stream(torch.cuda.current_stream(self.dataset.device))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(s):
                with torch.cuda.graph(graph, stream=s):
                    self._chain()
            torch.cuda.current_stream(self.dataset.device).wait_stream(s)
            self.dataset.draws = draws                  # the capture launched nothing
            self._graph = graph
        self._graph.replay()
        self.dataset.draws += self.steps
        self.runs += 1


# behind the classes above: train.py imports them at its own end
from .train import BundleTrainer, ConvGDTrainer, DeviceAdam, GDTrainer, unpack_grad  # noqa: E402
