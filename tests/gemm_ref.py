"""Host restatement of the split-K plan of launch_tr_gemm (be_train_common.hip, gemm_splits) for the training tests: which
feeds cut a weight-gradient product into many chunks with a short last one."""

# be_train_common.hip: 64 x 64 output tiles, K in steps of 16, at most 32 splits
GBM = GBN = 64
GBK = 16
MAX_SPLITS = 32


def gemm_splits(M, N, K):
    """(splits, kchunk) of be_train_common.hip's gemm_splits, restated"""
    tiles = -(-M // GBM) * -(-N // GBN)
    splits = 1
    if tiles < 256 and K > 64:
        splits = min(-(-256 // tiles), -(-K // 64), MAX_SPLITS)
    kchunk = -(-K // splits)
    kchunk = max(-(-kchunk // GBK) * GBK, GBK)
    return (-(-K // kchunk) if K > 0 else 1), kchunk
