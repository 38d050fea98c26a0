"""NumPy statement of the device dataset's index rule (include/icnn_be.h, icnn_be_dataset_draw; icnn_amd/csrc/be_train_data.hip;
icnn_amd/train.DeviceDataset): sample k of draw d takes row

    (word * N) >> 32,   word = word 0 of Philox4x32-10 at counter (d, k, 0, 1) and key (seed & 0xffffffff, seed >> 32)

-- npr.randint(N, size=batch) of multi-label-cls/icnn_ebundle.py:214 with this library's random numbers: independent, with
replacement.  Counter word 3 is the domain tag that keeps the stream apart from the replay memory's (tag 0, replay_ref)."""
import numpy as np

from replay_ref import MASK, philox4x32_10

DOMAIN = 1


def index(seed, draw, k, n_rows):
    word = philox4x32_10((draw, k, 0, DOMAIN), (seed & MASK, (seed >> 32) & MASK))[0]
    return (word * n_rows) >> 32


def indices(seed, draw, batch, n_rows):
    """the int32 [batch] indices of draw number `draw`"""
    return np.array([index(seed, draw, k, n_rows) for k in range(batch)], np.int32)


def chi_square(seed, n_rows, draws=16, batch=1024):
    """Pearson's statistic of the histogram over draws 0..draws-1 x k 0..batch-1 against the uniform law"""
    counts = np.zeros(n_rows, np.int64)
    for d in range(draws):
        counts += np.bincount(indices(seed, d, batch, n_rows), minlength=n_rows)
    expect = draws * batch / n_rows
    return float(((counts - expect) ** 2 / expect).sum())
