"""GPU parity of the running totals inside each key of a resident OPE column (dds_col_scan_part_by_ope,
dds_col_scan_part_by_ope_be: SUM(x) OVER (PARTITION BY key ORDER BY row)): slot order, row ids, keys, counts and every
value bit-exact against a plain-Python GROUP BY with a sequential product inside each group, forward and suffix, in
the column and the big-endian form, with long partitions and partitions of one row, dead rows in either column, rows
lacking the position, a WHERE mask from a real search_mask, both capacity errors, no participating row, every row a
partition of its own, the resident store's methods against a dict over its rows, and Paillier's meaning."""
import ctypes as C
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def oracle(rows, keyvals, part, N, suffix):
    """(row ids, values, keys ascending, counts) of the rows with part[i] true in (key, row id) order: the value of
    a row is the product of its key's rows up to it (suffix: from it on)"""
    groups = {}
    for i, (k, p) in enumerate(zip(keyvals, part)):
        if p:
            groups.setdefault(int(k), []).append(i)
    ks = sorted(groups)
    ids, vals = [], []
    for k in ks:
        g, r, run = groups[k], 1, []
        for i in (reversed(g) if suffix else g):
            r = r * rows[i] % N
            run.append(r)
        ids += g
        vals += run[::-1] if suffix else run
    return ids, vals, ks, [len(groups[k]) for k in ks]


def check(eng, col, by, N, rows, keyvals, part, mask=None):
    """both forms and both directions against the oracle over the rows with part[i] true"""
    for suffix in (False, True):
        ids, vals, ks, cnt = oracle(rows, keyvals, part, N, suffix)
        got_rows, got, keys, counts = col.scan_part_by_ope(by, mask, suffix=suffix)
        assert got_rows.dtype == np.uint64 and keys.dtype == np.int64 and counts.dtype == np.uint64
        assert keys.tolist() == ks and counts.tolist() == cnt and got_rows.tolist() == ids
        assert got == vals
        out = eng.column(N, len(ids) + 2)
        try:
            out.append(rows[:2])
            got_rows, keys, counts = out.append_scan_part_by_ope(col, by, mask, suffix=suffix)
            assert keys.tolist() == ks and counts.tolist() == cnt and got_rows.tolist() == ids
            assert len(out) == 2 + len(ids) and out.live_count == len(out)
            assert out.read(0, 2) == rows[:2] and out.read(2, len(ids)) == vals
        finally:
            out.close()
    return ks


@pytest.fixture(scope="module")
def base(eng, keys):
    """1,100 seeded rows below the smallest committed Paillier n², keys in a small range so that the partitions are
    long (about 120 rows: several chunks each), and three keys of one row each"""
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(311)
    n = 1100
    rows = [rng.randrange(N) for _ in range(n)]
    keyvals = [rng.randrange(-4, 5) for _ in range(n)]
    keyvals[0], keyvals[500], keyvals[n - 1] = -100, 77, 10 ** 12  # partitions of one row: first, inside, last
    col, by = eng.column(N, n), eng.opecol(n)
    col.append(rows)
    by.append(keyvals)
    yield N, rows, keyvals, col, by
    col.close()
    by.close()


def test_long_partitions_and_partitions_of_one_row(eng, base):
    N, rows, keyvals, col, by = base
    ks = check(eng, col, by, N, rows, keyvals, [True] * len(rows))
    assert ks == [-100] + list(range(-4, 5)) + [77, 10 ** 12]


@pytest.mark.parametrize("op", ["gt", "le"])
def test_where_mask_from_search_mask(eng, base, op):
    N, rows, keyvals, col, by = base
    words, matches = by.search_mask(1, op)
    pred = {"gt": lambda k: k > 1, "le": lambda k: k <= 1}[op]
    part = [pred(k) for k in keyvals]
    assert matches == sum(part)
    ks = check(eng, col, by, N, rows, keyvals, part, words)
    assert (1 in ks) == (op == "le")


def test_dead_rows_and_rows_lacking_the_position(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(312)
    n = 200
    rows = [rng.randrange(N) for _ in range(n)]
    keyvals = [rng.randrange(-3, 3) for _ in range(n)]
    cls = [rng.choice((0, 1, 2, 2)) for _ in range(n)]
    cls[:3] = [0, 1, 2]
    col, by = eng.column(N, n), eng.opecol(n)
    try:
        col.append(rows)
        by.append(keyvals, cls)
        part = [c != 0 for c in cls]
        check(eng, col, by, N, rows, keyvals, part)
        dead_col = set(rng.sample(range(n), 30))
        dead_by = set(rng.sample(range(n), 30)) | {i for i in range(n) if keyvals[i] == 2}  # a whole key goes
        col.set_live(sorted(dead_col), 0)
        by.set_live(sorted(dead_by), 0)
        ks = check(eng, col, by, N, rows, keyvals,
                   [p and i not in dead_col and i not in dead_by for i, p in enumerate(part)])
        assert 2 not in ks
        col.set_live(list(range(n)), 0)
        for suffix in (False, True):
            got_rows, vals, keys_, counts = col.scan_part_by_ope(by, suffix=suffix)  # no participating row
            assert len(got_rows) == 0 and vals == [] and len(keys_) == 0 and len(counts) == 0
    finally:
        col.close()
        by.close()


def test_every_row_its_own_partition(eng, keys):
    """ngroups == nrows: every row a head, the values are the rows' residues in key order"""
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(313)
    n = 300
    rows = [rng.randrange(N) for _ in range(n)]
    keyvals = list(range(n))
    rng.shuffle(keyvals)
    col, by = eng.column(N, n), eng.opecol(n)
    try:
        col.append(rows)
        by.append(keyvals)
        ks = check(eng, col, by, N, rows, keyvals, [True] * n)
        assert len(ks) == n
        got_rows, vals, _, counts = col.scan_part_by_ope(by)
        assert counts.tolist() == [1] * n and vals == [rows[int(r)] for r in got_rows]
    finally:
        col.close()
        by.close()


def test_either_capacity_too_small_writes_nothing(eng, base):
    import ddshe
    N, rows, keyvals, col, by = base
    lib = ddshe._lib
    mb, n, ngr = col.mb, len(rows), 12
    for suffix in (0, 1):
        for cap_rows, cap_groups in ((n - 1, ngr), (n, ngr - 1), (0, 0)):
            nr, ng = C.c_size_t(0), C.c_size_t(0)
            rows_ = (C.c_uint64 * n)(*[99] * n)
            keys_ = (C.c_int64 * ngr)(*[99] * ngr)
            counts = (C.c_uint64 * ngr)(*[99] * ngr)
            buf = (C.c_uint8 * (mb * 8))()  # nothing may be written: eight rows of room are watched
            assert lib.dds_col_scan_part_by_ope_be(col._h, by._h, None, 0, suffix, buf, rows_, cap_rows, keys_, counts,
                                                   cap_groups, C.byref(nr), C.byref(ng)) == ddshe.DDS_E_BUFSIZE
            assert (nr.value, ng.value) == (n, ngr)  # both set to what is required
            assert list(rows_) == [99] * n and list(keys_) == [99] * ngr and list(counts) == [99] * ngr
            assert bytes(buf) == bytes(mb * 8)
            out = eng.column(N, n + 3)
            try:
                out.append(rows[:3])
                assert lib.dds_col_scan_part_by_ope(col._h, by._h, None, 0, suffix, out._h, rows_, cap_rows, keys_,
                                                    counts, cap_groups, C.byref(nr), C.byref(ng)) == ddshe.DDS_E_BUFSIZE
                assert (nr.value, ng.value) == (n, ngr) and len(out) == 3 and list(keys_) == [99] * ngr
            finally:
                out.close()
    small = eng.column(N, 4)  # room in rows, keys and counts, not in the output column
    try:
        with pytest.raises(ddshe.DDSError) as ei:
            small.append_scan_part_by_ope(col, by)
        assert ei.value.status == ddshe.DDS_E_ARG and len(small) == 0
    finally:
        small.close()


def test_modmuls_equal_the_plan(eng, base):
    N, rows, keyvals, col, by = base
    _, _, _, cnt = oracle(rows, keyvals, [True] * len(rows), N, False)
    starts = [0] + np.cumsum(cnt)[:-1].tolist()
    eng.set_timing(True)
    try:
        for suffix in (False, True):
            eng.reset_timing()
            col.scan_part_by_ope(by, suffix=suffix)
            fold_ms, launches, total_ms, modmuls = eng.timing()
            _, levels, products, _ = eng.segscan_plan(len(rows), starts, suffix)
            assert modmuls == products and launches == 2 * levels + 1 and fold_ms > 0 and total_ms > 0
    finally:
        eng.set_timing(False)
        eng.reset_timing()


def test_paillier_meaning_under_the_2048_bit_key(eng, keys):
    """decrypting the output gives the partial sums inside each partition"""
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(314)
    ms = [rng.randrange(10000) for _ in range(150)]
    rs = [rng.randrange(1, n) for _ in ms]
    accounts = [rng.randrange(5) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    src, by, out = eng.column(nsq, 150), eng.opecol(150), eng.column(nsq, 150)
    try:
        src.append(cs)
        by.append(accounts)
        got_rows, keys_, counts = out.append_scan_part_by_ope(src, by)
        assert keys_.tolist() == sorted(set(accounts)) and int(counts.sum()) == 150
        balances, run = [], {}
        for r in got_rows.tolist():  # (account, row) order: a running balance per account
            run[accounts[r]] = (run.get(accounts[r], 0) + ms[r]) % n
            balances.append(run[accounts[r]])
        assert out.decrypt_paillier(0, 150, key["p"], key["q"], g) == balances
    finally:
        for c in (src, by, out):
            c.close()


def by_reference(st, position, by_position, N, descending):
    """the store's rows SumAll folds that hold an element at by_position, grouped by its value: per key the
    (stored-set key, running product as text) pairs in row order"""
    seen, groups = set(), {}
    for name, row in st.keyed_rows():
        if row is None or not len(row) - 1 > position:
            continue
        sig = tuple(str(v) for v in row)
        if sig in seen:
            continue
        seen.add(sig)
        if len(row) > by_position:
            groups.setdefault(int(row[by_position]), []).append((name, int(row[position])))
    out = {}
    for k, members in groups.items():
        r, run = 1, []
        for name, x in (reversed(members) if descending else members):
            r = r * x % N
            run.append((name, str(r)))
        out[k] = run[::-1] if descending else run
    return out


def test_store_running_sum_partition_by_ope(eng, keys):
    from ddshe.routes import NotFound, ServerError
    from ddshe.store import ResidentStore
    nsq = keys["paillier1024_seed1"]["nsquare"]
    rsa = keys["rsa1024_committed"]
    rng = random.Random(315)
    # contents: [name, Paillier c, RSA c, day (OPE), price band (OPE), tail]
    st = ResidentStore(eng, paillier={1: nsq}, rsa={2: rsa["n"]}, ope=(3, 4), capacity=64, strings=False)
    try:
        with pytest.raises(NotFound):
            st.running_sum_partition_by_ope(1, 3, str(nsq))
        days = ["20260101", "20260102", "20260101", "7", "07", "20260102", "-5", "20260101", "7", "20260103"]
        sets = [[f"k{i}", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), d, str(rng.randrange(1, 6)), "x"]
                for i, d in enumerate(days)]
        sets.append(["short", str(rng.randrange(nsq))])  # fails both guards, lacks the grouping position
        sets.append(["gone", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "20260101", "3", "x"])
        keys_ = st.put_sets(sets)
        st.remove_set(keys_[11])
        for descending in (False, True):
            want = by_reference(st, 1, 3, nsq, descending)
            assert set(want) == {20260101, 20260102, 20260103, 7, -5} and len(want[7]) == 3
            assert st.running_sum_partition_by_ope(1, 3, str(nsq), descending=descending) == want
            assert st.running_mult_partition_by_ope(2, 3, rsa["x509_hex"], descending=descending) == \
                by_reference(st, 2, 3, rsa["n"], descending)
        # the last row of a partition ascending and its first descending hold the partition's SumAll
        asc = st.running_sum_partition_by_ope(1, 3, str(nsq))
        desc = st.running_sum_partition_by_ope(1, 3, str(nsq), descending=True)
        full = st.sum_all_by_ope(1, 3, str(nsq))
        assert {k: v[-1][1] for k, v in asc.items()} == full == {k: v[0][1] for k, v in desc.items()}
        where = ("SearchGtEq", 3, "20260101")
        got = st.running_sum_partition_by_ope(1, 3, str(nsq), where=where)
        assert got == {k: v for k, v in asc.items() if k >= 20260101} and set(got) == {20260101, 20260102, 20260103}
        for call in (lambda: st.running_sum_partition_by_ope(1, 5, str(nsq)),
                     lambda: st.running_sum_partition_by_ope(1, 3, "x"),
                     lambda: st.running_mult_partition_by_ope(2, 3, "zz")):
            with pytest.raises(ServerError):
                call()
    finally:
        st.close()
