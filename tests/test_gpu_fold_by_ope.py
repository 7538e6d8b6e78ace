"""GPU parity of the grouped fold keyed by a resident OPE column (dds_col_fold_by_ope, dds_col_fold_by_ope_be):
keys, counts and every group's value bit-exact against a plain-Python GROUP BY (a dict by key, the product mod N
with Python ints), in the column and the big-endian form, for group sizes that give one, two and three fold levels,
few and many groups, dead rows in either column, rows lacking the position, WHERE masks from a real search_mask,
the capacity and element errors, Paillier's meaning through the existing decryption, and two threads."""
import ctypes as C
import math
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1025)  # one level up to 32 rows, two up to 1,024, three above


def prod_mod(xs, N):
    r = 1
    for i in range(0, len(xs), 16):
        r = r * math.prod(xs[i:i + 16]) % N
    return r % N


def oracle(rows, keyvals, part, N):
    """(keys ascending, values, counts) of the rows with part[i] true, grouped by keyvals[i]"""
    groups = {}
    for x, k, p in zip(rows, keyvals, part):
        if p:
            groups.setdefault(int(k), []).append(x)
    ks = sorted(groups)
    return ks, [prod_mod(groups[k], N) for k in ks], [len(groups[k]) for k in ks]


def mask_of(part):
    """uint64 words, bit r % 64 of word r / 64 = part[r]: the layout of dds_opecol_search_mask"""
    bits = np.zeros((len(part) + 63) // 64 * 64, dtype=np.uint8)
    bits[:len(part)] = np.asarray(part, dtype=bool)
    return np.packbits(bits, bitorder="little").view(np.uint64)


def check(eng, col, by, N, rows, keyvals, part, mask=None):
    """both forms against the oracle over the rows with part[i] true"""
    ks, vals, sizes = oracle(rows, keyvals, part, N)
    keys, got, counts = col.fold_by_ope(by, mask)
    assert keys.dtype == np.int64 and counts.dtype == np.uint64
    assert keys.tolist() == ks and counts.tolist() == sizes
    assert got == vals
    out = eng.column(N, len(ks) + 2)
    try:
        out.append(rows[:2])
        keys, counts = out.append_fold_by_ope(col, by, mask)
        assert keys.tolist() == ks and counts.tolist() == sizes
        assert len(out) == 2 + len(ks) and out.live_count == len(out)
        assert out.read(0, 2) == rows[:2] and out.read(2, len(ks)) == vals
    finally:
        out.close()
    return ks, vals, sizes


@pytest.fixture(scope="module")
def base(eng, keys):
    """sum(SIZES) = 1,122 seeded rows below the smallest committed Paillier n² in a resident column, and an OPE
    column whose keys give groups of exactly SIZES rows, shuffled; keys negative and positive"""
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(81)
    rows = [rng.randrange(N) for _ in range(sum(SIZES))]
    keyvals = [k for k, c in zip((-7, 0, 3, 10 ** 12, 44), SIZES) for _ in range(c)]
    rng.shuffle(keyvals)
    col, by = eng.column(N, len(rows)), eng.opecol(len(rows))
    col.append(rows)
    by.append(keyvals)
    yield N, rows, keyvals, col, by
    col.close()
    by.close()


def test_one_two_and_three_levels(eng, base):
    N, rows, keyvals, col, by = base
    ks, _, sizes = check(eng, col, by, N, rows, keyvals, [True] * len(rows))
    assert ks == [-7, 0, 3, 44, 10 ** 12] and sorted(sizes) == sorted(SIZES)


@pytest.mark.parametrize("ngroups", [3, 300])
def test_few_and_many_groups(eng, keys, ngroups):
    """on either side of kGroupsLdsLabels = 256 (the counting sort's threshold): this path has no such regime"""
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(ngroups)
    n = 700
    rows = [rng.randrange(N) for _ in range(n)]
    keyvals = [rng.randrange(ngroups) * 1000 - 5000 for _ in range(n)]
    keyvals[:ngroups] = [g * 1000 - 5000 for g in range(ngroups)]
    col, by = eng.column(N, n), eng.opecol(n)
    try:
        col.append(rows)
        by.append(keyvals)
        ks, _, _ = check(eng, col, by, N, rows, keyvals, [True] * n)
        assert len(ks) == ngroups
    finally:
        col.close()
        by.close()


def test_dead_rows_and_rows_lacking_the_position(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(82)
    n = 400
    rows = [rng.randrange(N) for _ in range(n)]
    keyvals = [rng.randrange(-6, 6) for _ in range(n)]
    cls = [rng.choice((0, 1, 2, 2)) for _ in range(n)]
    cls[:3] = [0, 1, 2]
    col, by = eng.column(N, n), eng.opecol(n)
    try:
        col.append(rows)
        by.append(keyvals, cls)
        part = [c != 0 for c in cls]
        check(eng, col, by, N, rows, keyvals, part)  # class 0 drops out, class 1 takes part
        dead_col = set(rng.sample(range(n), 60))
        col.set_live(sorted(dead_col), 0)
        part_c = [p and i not in dead_col for i, p in enumerate(part)]
        check(eng, col, by, N, rows, keyvals, part_c)  # dead in col only
        col.set_live(sorted(dead_col), 1)
        dead_by = set(rng.sample(range(n), 60)) | {i for i in range(n) if keyvals[i] == 5}  # a whole key goes
        by.set_live(sorted(dead_by), 0)
        part_b = [p and i not in dead_by for i, p in enumerate(part)]
        ks, _, _ = check(eng, col, by, N, rows, keyvals, part_b)  # dead in by only
        assert 5 not in ks
        col.set_live(sorted(dead_col), 0)
        check(eng, col, by, N, rows, keyvals, [a and b for a, b in zip(part_c, part_b)])  # in both
        col.set_live(list(range(n)), 0)
        keys_, vals, counts = col.fold_by_ope(by)  # no participating row
        assert len(keys_) == 0 and vals == [] and len(counts) == 0
    finally:
        col.close()
        by.close()


@pytest.mark.parametrize("op", ["gt", "ge", "lt", "le"])
def test_where_mask_from_search_mask(eng, base, op):
    """WHERE key <op> 3, 3 a present key: the mask of dds_opecol_search_mask passes straight through"""
    N, rows, keyvals, col, by = base
    words, matches = by.search_mask(3, op)
    pred = {"gt": lambda k: k > 3, "ge": lambda k: k >= 3, "lt": lambda k: k < 3, "le": lambda k: k <= 3}[op]
    part = [pred(k) for k in keyvals]
    assert matches == sum(part)
    ks, _, _ = check(eng, col, by, N, rows, keyvals, part, words)
    assert (3 in ks) == (op in ("ge", "le"))


def test_masks(eng, base):
    N, rows, keyvals, col, by = base
    rng = random.Random(83)
    part = [rng.randrange(3) == 0 for _ in rows]
    check(eng, col, by, N, rows, keyvals, part, mask_of(part))
    keys_, vals, counts = col.fold_by_ope(by, mask_of([False] * len(rows)))  # the mask removes every row
    assert len(keys_) == 0 and vals == [] and len(counts) == 0
    import ddshe
    with pytest.raises(ddshe.DDSError) as ei:
        col.fold_by_ope(by, mask_of(part)[:-1])  # one word short
    assert ei.value.status == ddshe.DDS_E_ARG


def test_capacity_one_too_small(eng, base):
    import ddshe
    N, rows, keyvals, col, by = base
    lib = ddshe._lib
    mb = col.mb
    for cap in (4, 0):
        ng = C.c_size_t(0)
        keys_ = (C.c_int64 * 5)(*[99] * 5)
        counts = (C.c_uint64 * 5)(*[99] * 5)
        buf = (C.c_uint8 * (mb * 5))()
        assert lib.dds_col_fold_by_ope_be(col._h, by._h, None, 0, buf, keys_, counts, cap,
                                          C.byref(ng)) == ddshe.DDS_E_BUFSIZE
        assert ng.value == 5  # the count required
        assert list(keys_) == [99] * 5 and list(counts) == [99] * 5 and bytes(buf) == bytes(mb * 5)
        out = eng.column(N, 16)
        try:
            out.append(rows[:3])
            ng = C.c_size_t(0)
            assert lib.dds_col_fold_by_ope(col._h, by._h, None, 0, out._h, keys_, counts, cap,
                                           C.byref(ng)) == ddshe.DDS_E_BUFSIZE
            assert ng.value == 5 and len(out) == 3 and list(keys_) == [99] * 5
            assert lib.dds_col_fold_by_ope(col._h, by._h, None, 0, out._h, keys_, counts, 5, C.byref(ng)) == ddshe.DDS_OK
            assert ng.value == 5 and len(out) == 8 and list(keys_) == [-7, 0, 3, 44, 10 ** 12]
        finally:
            out.close()
    small = eng.column(N, 4)  # room in keys and counts, not in the output column
    try:
        with pytest.raises(ddshe.DDSError) as ei:
            small.append_fold_by_ope(col, by)
        assert ei.value.status == ddshe.DDS_E_ARG and len(small) == 0
    finally:
        small.close()


def test_element_errors(eng, keys):
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(84)
    texts = ["7", "07", "-2", "+7", "12x", "9" * 30, "-2"]  # row 4 malformed, row 5 outside int64
    rows = [rng.randrange(N) for _ in texts]
    col, by, out = eng.column(N, 8), eng.opecol(8), eng.column(N, 8)
    try:
        col.append(rows)
        by.append_dec(texts, is_string=[1, 1, 0, 1, 1, 1, 1])  # a non-String element is fine: values compare
        for call in (lambda: col.fold_by_ope(by), lambda: out.append_fold_by_ope(col, by)):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_FORMAT
        by.set_live([4], 0)
        for call in (lambda: col.fold_by_ope(by), lambda: out.append_fold_by_ope(col, by)):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_UNSUPPORTED
        assert len(out) == 0
        by.set_live([5], 0)  # the same rows marked dead are accepted
        keyvals = [7, 7, -2, 7, 0, 0, -2]
        check(eng, col, by, N, rows, keyvals, [True, True, True, True, False, False, True])
        by.set_live([4], 1)
        by.write_rows_dec([4], ["12"])  # repaired in place
        keyvals[4] = 12
        check(eng, col, by, N, rows, keyvals, [True, True, True, True, True, False, True])
    finally:
        for c in (col, by, out):
            c.close()


def test_row_count_mismatch(eng, base):
    import ddshe
    N, rows, keyvals, col, by = base
    short, out = eng.opecol(8), eng.column(N, 8)
    try:
        short.append(keyvals[:8])
        for call in (lambda: col.fold_by_ope(short), lambda: out.append_fold_by_ope(col, short)):
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
        assert len(out) == 0
        with pytest.raises(ddshe.DDSError) as ei:
            col.append_fold_by_ope(col, by)  # out == col
        assert ei.value.status == ddshe.DDS_E_ARG
    finally:
        short.close()
        out.close()


def test_equals_fold_groups_on_host_labels(base):
    N, rows, keyvals, col, by = base
    uniq, inv = np.unique(np.asarray(keyvals, dtype=np.int64), return_inverse=True)
    vals, counts = col.fold_groups(inv.astype(np.uint32), len(uniq))
    keys_, got, cnt = col.fold_by_ope(by)
    assert keys_.tolist() == uniq.tolist() and got == vals and cnt.tolist() == counts.tolist()


def test_paillier_meaning_under_the_2048_bit_key(eng, keys):
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(85)
    ms = [rng.randrange(10000) for _ in range(150)]
    rs = [rng.randrange(1, n) for _ in ms]
    days = [rng.randrange(20260101, 20260108) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    src, by, out = eng.column(nsq, 150), eng.opecol(150), eng.column(nsq, 8)
    try:
        src.append(cs)
        by.append(days)
        ks, vals, _ = check(eng, src, by, nsq, cs, days, [True] * 150)
        keys_, counts = out.append_fold_by_ope(src, by)
        sums = [sum(m for m, d in zip(ms, days) if d == k) % n for k in ks]
        assert keys_.tolist() == ks and counts.tolist() == [days.count(k) for k in ks]
        assert out.decrypt_paillier(0, len(ks), key["p"], key["q"], g) == sums
    finally:
        for c in (src, by, out):
            c.close()


def test_rsa_modulus(eng, keys):
    N = keys["rsa1024_committed"]["n"]
    rng = random.Random(86)
    rows = [rng.randrange(N) for _ in range(90)]
    keyvals = [rng.randrange(-3, 3) for _ in rows]
    col, by = eng.column(N, 90), eng.opecol(90)
    try:
        col.append(rows)
        by.append(keyvals)
        check(eng, col, by, N, rows, keyvals, [True] * 90)
    finally:
        col.close()
        by.close()


def test_two_threads_on_one_context(base):
    N, rows, keyvals, col, by = base
    rng = random.Random(87)
    parts = [[True] * len(rows), [rng.randrange(2) == 0 for _ in rows]]
    masks = [None, mask_of(parts[1])]
    want = [oracle(rows, keyvals, p, N) for p in parts]
    got = [None, None]

    def run(i):
        for _ in range(3):
            ks, vals, counts = col.fold_by_ope(by, masks[i])
            got[i] = (ks.tolist(), vals, counts.tolist())

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == [tuple(w) for w in want]
