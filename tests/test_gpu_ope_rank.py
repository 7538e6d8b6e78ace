"""GPU parity of the dense ranks (dds_ope_rank, dds_ope_rank_device): labels, distinct keys and counts bit-exact
against np.unique(keys of the valid rows, return_inverse=True, return_counts=True), in the host and the device
form, for the sizes around the rank kernels' scan tile, the edges of int64, invalid rows, both paths of the sort
underneath, and the labels as dds_col_fold_groups' input."""
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096  # kRankTile, csrc/ddshe_launch.hpp ("constexpr int kRankTile = 4096;")
NONE = 0xFFFFFFFF
I64 = np.iinfo(np.int64)


def reference(col, valid):
    col = np.asarray(col, dtype=np.int64)
    v = np.ones(len(col), dtype=bool) if valid is None else np.asarray(valid) != 0
    keys, inv, counts = np.unique(col[v], return_inverse=True, return_counts=True)
    labels = np.full(len(col), NONE, dtype=np.uint32)
    labels[v] = inv
    return labels, keys, counts.astype(np.uint64)


def check(eng, col, valid=None):
    """both forms against the reference; returns the host form's result"""
    import torch
    col = np.asarray(col, dtype=np.int64)
    n = len(col)
    want = reference(col, valid)
    labels, keys, counts = eng.ope_rank(col, valid)
    assert labels.dtype == np.uint32 and keys.dtype == np.int64 and counts.dtype == np.uint64
    for got, ref in zip((labels, keys, counts), want):
        assert np.array_equal(got, ref)
    if n == 0:
        assert eng.ope_rank_device(0, None, 0, None, None, None) == 0
        return labels, keys, counts
    d_col = torch.from_numpy(col).cuda()
    d_valid = None if valid is None else torch.from_numpy(np.asarray(valid, dtype=np.uint8)).cuda()
    # int32 / int64 tensors carry the uint32 labels and counts bit for bit
    d_lab = torch.full((n,), -2, dtype=torch.int32, device="cuda")
    d_keys = torch.zeros(n, dtype=torch.int64, device="cuda")
    d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ng = eng.ope_rank_device(d_col.data_ptr(), None if d_valid is None else d_valid.data_ptr(), n, d_lab.data_ptr(),
                             d_keys.data_ptr(), d_cnt.data_ptr())
    assert ng == len(want[1])
    assert np.array_equal(d_lab.cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(d_keys.cpu().numpy()[:ng], want[1])
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32)[:ng], want[2].astype(np.uint32))
    assert eng.ope_rank_device(d_col.data_ptr(), None if d_valid is None else d_valid.data_ptr(), n, None, None,
                               None) == ng  # every output is optional
    return labels, keys, counts


@pytest.mark.parametrize("col", [[], [5], [5, 5], [9, -9], [-9, 9]])
def test_tiny(eng, col):
    check(eng, col)
    if col:
        check(eng, col, [1] * len(col))
        check(eng, col, [0] + [1] * (len(col) - 1))


def test_all_equal_and_all_distinct(eng):
    rng = random.Random(71)
    check(eng, [-3] * 1000)
    distinct = list(range(-500, 500))
    rng.shuffle(distinct)
    labels, keys, counts = check(eng, distinct)
    assert keys.tolist() == list(range(-500, 500)) and counts.tolist() == [1] * 1000


def test_edges_of_int64(eng):
    rng = random.Random(72)
    col = [I64.min, I64.max, -1, 0, 1, I64.min + 1, I64.max - 1] * 9 + [rng.randrange(-10 ** 6, 10 ** 6) for _ in range(200)]
    rng.shuffle(col)
    labels, keys, _ = check(eng, col)
    assert keys[0] == I64.min and keys[-1] == I64.max
    check(eng, col, [rng.randrange(4) != 0 for _ in col])


def test_invalid_rows(eng):
    rng = random.Random(73)
    col = [rng.randrange(-40, 40) for _ in range(3001)]
    labels, _, _ = check(eng, col, [i % 2 for i in range(3001)])  # every other row
    assert (labels[0::2] == NONE).all() and (labels[1::2] != NONE).all()
    labels, keys, counts = check(eng, col, [0] * 3001)  # none valid
    assert len(keys) == 0 and len(counts) == 0 and (labels == NONE).all()
    check(eng, col, [0] * 3000 + [1])  # one valid row, in the last slot of the permutation


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_around_the_scan_tile(eng, n):
    rng = random.Random(n)
    col = np.asarray([rng.randrange(-300, 300) for _ in range(n)], dtype=np.int64)
    check(eng, col)
    valid = np.asarray([rng.randrange(8) != 0 for _ in range(n)], dtype=np.uint8)
    valid[-1] = 1
    check(eng, col, valid)
    check(eng, np.arange(n, 0, -1))  # every slot a head: the tiles' sums are full


@pytest.mark.parametrize("span_bits", [40, 20])
def test_both_paths_of_the_sort(eng, span_bits):
    """n >= 2^16: a key span above 2^24 takes the sort's MSD path (msd_enabled, csrc/ddshe_sort.hip), one below it
    the LSD passes only"""
    n = 2 ** 16 + 77
    rng = np.random.default_rng(span_bits)
    pool = rng.integers(-(1 << (span_bits - 1)), 1 << (span_bits - 1), size=5000, dtype=np.int64)
    pool[0], pool[1] = -(1 << (span_bits - 1)), (1 << (span_bits - 1)) - 1
    col = pool[rng.integers(0, len(pool), size=n)]
    col[:2] = pool[:2]
    assert int(col.max()) - int(col.min()) >= 1 << (span_bits - 1)
    check(eng, col)
    valid = (rng.integers(0, 5, size=n) != 0).astype(np.uint8)
    valid[:2] = 1
    check(eng, col, valid)


def test_labels_feed_fold_groups(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(74)
    n = 500
    col = [rng.randrange(-20, 20) for _ in range(n)]
    valid = [rng.randrange(5) != 0 for _ in range(n)]
    rows = [rng.randrange(N) for _ in range(n)]
    labels, ks, counts = eng.ope_rank(col, valid)
    c = eng.column(N, n)
    try:
        c.append(rows)
        c.set_live([i for i in range(n) if not valid[i]], 0)  # 0xFFFFFFFF is no label: those rows are dead
        safe = np.where(labels == NONE, 0, labels)
        vals, cnt = c.fold_groups(safe, len(ks))
        assert cnt.tolist() == counts.tolist()
        for g, k in enumerate(ks.tolist()):
            assert vals[g] == math.prod(rows[i] for i in range(n) if valid[i] and col[i] == k) % N
        # and as they are, over the valid rows only
        ids = [i for i in range(n) if valid[i]]
        vals2, cnt2 = c.fold_groups(labels[ids], len(ks), row_ids=ids)
        assert vals2 == vals and cnt2.tolist() == counts.tolist()
    finally:
        c.close()
