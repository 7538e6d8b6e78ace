"""GPU parity of the cumulative SUM by key over resident columns (dds_col_scan_by_ope, dds_col_scan_by_ope_be):
keys, cumulative counts and every key's running value bit-exact against a plain-Python GROUP BY followed by a
sequential product over the sorted keys, ascending and suffix, in the column and the big-endian form, for group
sizes that give one, two and three fold levels, enough distinct keys for the scan of the totals itself to have one
and two levels, dead rows, rows lacking the position, a WHERE mask from a real search_mask, the capacity error, and
the resident store's running_sum_by_ope against a dict over its rows."""
import ctypes as C
import math
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1025)  # one fold level up to 32 rows, two up to 1,024, three above


def prod_mod(xs, N):
    r = 1
    for i in range(0, len(xs), 16):
        r = r * math.prod(xs[i:i + 16]) % N
    return r % N


def oracle(rows, keyvals, part, N, suffix):
    """(keys ascending, running values, cumulative counts) of the rows with part[i] true, grouped by keyvals[i]:
    the value of a key is the product of the rows whose key is <= it (suffix: >= it)"""
    groups = {}
    for x, k, p in zip(rows, keyvals, part):
        if p:
            groups.setdefault(int(k), []).append(x)
    ks = sorted(groups)
    vals, counts, r, c = [0] * len(ks), [0] * len(ks), 1, 0
    for g in (range(len(ks) - 1, -1, -1) if suffix else range(len(ks))):
        r = r * prod_mod(groups[ks[g]], N) % N
        c += len(groups[ks[g]])
        vals[g], counts[g] = r, c
    return ks, vals, counts


def mask_of(part):
    """uint64 words, bit r % 64 of word r / 64 = part[r]: the layout of dds_opecol_search_mask"""
    bits = np.zeros((len(part) + 63) // 64 * 64, dtype=np.uint8)
    bits[:len(part)] = np.asarray(part, dtype=bool)
    return np.packbits(bits, bitorder="little").view(np.uint64)


def check(eng, col, by, N, rows, keyvals, part, mask=None):
    """both forms and both directions against the oracle over the rows with part[i] true"""
    for suffix in (False, True):
        ks, vals, cum = oracle(rows, keyvals, part, N, suffix)
        keys, got, counts = col.scan_by_ope(by, mask, suffix=suffix)
        assert keys.dtype == np.int64 and counts.dtype == np.uint64
        assert keys.tolist() == ks and counts.tolist() == cum
        assert got == vals
        out = eng.column(N, len(ks) + 2)
        try:
            out.append(rows[:2])
            keys, counts = out.append_scan_by_ope(col, by, mask, suffix=suffix)
            assert keys.tolist() == ks and counts.tolist() == cum
            assert len(out) == 2 + len(ks) and out.live_count == len(out)
            assert out.read(0, 2) == rows[:2] and out.read(2, len(ks)) == vals
        finally:
            out.close()
    return ks


@pytest.fixture(scope="module")
def base(eng, keys):
    """the key layout of tests/test_gpu_fold_by_ope.py: sum(SIZES) = 1,122 seeded rows below the smallest
    committed Paillier n² and an OPE column whose keys give groups of exactly SIZES rows, shuffled"""
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(111)
    rows = [rng.randrange(N) for _ in range(sum(SIZES))]
    keyvals = [k for k, c in zip((-7, 0, 3, 10 ** 12, 44), SIZES) for _ in range(c)]
    rng.shuffle(keyvals)
    col, by = eng.column(N, len(rows)), eng.opecol(len(rows))
    col.append(rows)
    by.append(keyvals)
    yield N, rows, keyvals, col, by
    col.close()
    by.close()


def test_one_two_and_three_fold_levels(eng, base):
    N, rows, keyvals, col, by = base
    assert check(eng, col, by, N, rows, keyvals, [True] * len(rows)) == [-7, 0, 3, 44, 10 ** 12]
    _, _, counts = col.scan_by_ope(by)
    assert counts.tolist()[-1] == len(rows)  # cumulative: the last key has seen every row


@pytest.mark.parametrize("op", ["gt", "le"])
def test_where_mask_from_search_mask(eng, base, op):
    N, rows, keyvals, col, by = base
    words, matches = by.search_mask(3, op)
    pred = {"gt": lambda k: k > 3, "le": lambda k: k <= 3}[op]
    part = [pred(k) for k in keyvals]
    assert matches == sum(part)
    ks = check(eng, col, by, N, rows, keyvals, part, words)
    assert (3 in ks) == (op == "le")


def test_dead_rows_and_rows_lacking_the_position(eng, keys):
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(112)
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
        check(eng, col, by, N, rows, keyvals, part)
        dead_col = set(rng.sample(range(n), 60))
        dead_by = set(rng.sample(range(n), 60)) | {i for i in range(n) if keyvals[i] == 5}  # a whole key goes
        col.set_live(sorted(dead_col), 0)
        by.set_live(sorted(dead_by), 0)
        ks = check(eng, col, by, N, rows, keyvals,
                   [p and i not in dead_col and i not in dead_by for i, p in enumerate(part)])
        assert 5 not in ks
        col.set_live(list(range(n)), 0)
        for suffix in (False, True):
            keys_, vals, counts = col.scan_by_ope(by, suffix=suffix)  # no participating row
            assert len(keys_) == 0 and vals == [] and len(counts) == 0
    finally:
        col.close()
        by.close()


@pytest.mark.parametrize("ngroups", [300, 1100])
def test_many_keys(eng, keys, ngroups):
    """300 distinct keys: the scan of the totals has one level of chunk totals; 1,100: two"""
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(ngroups)
    n = ngroups + 400
    rows = [rng.randrange(N) for _ in range(n)]
    keyvals = [rng.randrange(ngroups) * 1000 - 5000 for _ in range(n)]
    keyvals[:ngroups] = [g * 1000 - 5000 for g in range(ngroups)]
    assert eng.scan_plan(ngroups)[1] == (1 if ngroups == 300 else 2)
    col, by = eng.column(N, n), eng.opecol(n)
    try:
        col.append(rows)
        by.append(keyvals)
        ks = check(eng, col, by, N, rows, keyvals, [True] * n)
        assert len(ks) == ngroups
    finally:
        col.close()
        by.close()


def test_capacity_one_too_small(eng, base):
    import ddshe
    N, rows, keyvals, col, by = base
    lib = ddshe._lib
    mb = col.mb
    for suffix in (0, 1):
        ng = C.c_size_t(0)
        keys_ = (C.c_int64 * 5)(*[99] * 5)
        counts = (C.c_uint64 * 5)(*[99] * 5)
        buf = (C.c_uint8 * (mb * 5))()
        assert lib.dds_col_scan_by_ope_be(col._h, by._h, None, 0, suffix, buf, keys_, counts, 4,
                                          C.byref(ng)) == ddshe.DDS_E_BUFSIZE
        assert ng.value == 5  # the count required
        assert list(keys_) == [99] * 5 and list(counts) == [99] * 5 and bytes(buf) == bytes(mb * 5)
        out = eng.column(N, 16)
        try:
            out.append(rows[:3])
            ng = C.c_size_t(0)
            assert lib.dds_col_scan_by_ope(col._h, by._h, None, 0, suffix, out._h, keys_, counts, 4,
                                           C.byref(ng)) == ddshe.DDS_E_BUFSIZE
            assert ng.value == 5 and len(out) == 3 and list(keys_) == [99] * 5
            assert lib.dds_col_scan_by_ope(col._h, by._h, None, 0, suffix, out._h, keys_, counts, 5,
                                           C.byref(ng)) == ddshe.DDS_OK
            assert ng.value == 5 and len(out) == 8 and list(keys_) == [-7, 0, 3, 44, 10 ** 12]
        finally:
            out.close()
    small = eng.column(N, 4)  # room in keys and counts, not in the output column
    try:
        with pytest.raises(ddshe.DDSError) as ei:
            small.append_scan_by_ope(col, by)
        assert ei.value.status == ddshe.DDS_E_ARG and len(small) == 0
    finally:
        small.close()


def test_equals_scan_of_fold_by_ope(eng, base):
    """the same values as Column.scan over the rows fold_by_ope leaves"""
    N, rows, keyvals, col, by = base
    totals = eng.column(N, 8)
    try:
        keys_, counts = totals.append_fold_by_ope(col, by)
        for suffix in (False, True):
            ks, vals, cum = col.scan_by_ope(by, suffix=suffix)
            assert ks.tolist() == keys_.tolist() and vals == totals.scan(suffix=suffix)
            run = np.cumsum(counts[::-1])[::-1] if suffix else np.cumsum(counts)
            assert cum.tolist() == run.tolist()
    finally:
        totals.close()


def test_paillier_meaning_under_the_2048_bit_key(eng, keys):
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(113)
    ms = [rng.randrange(10000) for _ in range(150)]
    rs = [rng.randrange(1, n) for _ in ms]
    days = [rng.randrange(20260101, 20260108) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    src, by, out = eng.column(nsq, 150), eng.opecol(150), eng.column(nsq, 8)
    try:
        src.append(cs)
        by.append(days)
        keys_, counts = out.append_scan_by_ope(src, by)
        ks = sorted(set(days))
        assert keys_.tolist() == ks and counts.tolist() == [sum(d <= k for d in days) for k in ks]
        sums = [sum(m for m, d in zip(ms, days) if d <= k) % n for k in ks]
        assert out.decrypt_paillier(0, len(ks), key["p"], key["q"], g) == sums
    finally:
        for c in (src, by, out):
            c.close()


def by_reference(rows, position, by_position, N, descending):
    """the store's rows SumAll folds that hold an element at by_position, grouped by its value, then the running
    product over the keys up to (descending: from) each key"""
    seen, groups = set(), {}
    for row in rows:
        if row is None or not len(row) - 1 > position:
            continue
        sig = tuple(str(v) for v in row)
        if sig in seen:
            continue
        seen.add(sig)
        if len(row) > by_position:
            groups.setdefault(int(row[by_position]), []).append(int(row[position]))
    out, r = {}, 1
    for k in sorted(groups, reverse=descending):
        r = r * math.prod(groups[k]) % N
        out[k] = str(r)
    return out


def test_store_running_sum_by_ope(eng, keys):
    from ddshe.routes import NotFound, ServerError
    from ddshe.store import ResidentStore
    nsq = keys["paillier1024_seed1"]["nsquare"]
    rsa = keys["rsa1024_committed"]
    rng = random.Random(114)
    # contents: [name, Paillier c, RSA c, day (OPE), price band (OPE), tail]
    st = ResidentStore(eng, paillier={1: nsq}, rsa={2: rsa["n"]}, ope=(3, 4), capacity=64, strings=False)
    try:
        with pytest.raises(NotFound):
            st.running_sum_by_ope(1, 3, str(nsq))
        days = ["20260101", "20260102", "20260101", "7", "07", "20260102", "-5", "20260101", "7", "20260103"]
        sets = [[f"k{i}", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), d, str(rng.randrange(1, 6)), "x"]
                for i, d in enumerate(days)]
        sets.append(["short", str(rng.randrange(nsq))])  # fails both guards, lacks the grouping position
        sets.append(["gone", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "20260101", "3", "x"])
        keys_ = st.put_sets(sets)
        st.remove_set(keys_[11])
        for descending in (False, True):
            want = by_reference(st.rows(), 1, 3, nsq, descending)
            assert set(want) == {20260101, 20260102, 20260103, 7, -5}
            assert st.running_sum_by_ope(1, 3, str(nsq), descending=descending) == want
            assert st.running_mult_by_ope(2, 3, rsa["x509_hex"], descending=descending) == \
                by_reference(st.rows(), 2, 3, rsa["n"], descending)
        # the last key ascending and the first descending hold the SumAll of every grouped row
        asc, desc = st.running_sum_by_ope(1, 3, str(nsq)), st.running_sum_by_ope(1, 3, str(nsq), descending=True)
        assert asc[20260103] == desc[-5]
        where = ("SearchGtEq", 3, "20260101")
        got = st.running_sum_by_ope(1, 3, str(nsq), where=where)
        full = st.sum_all_by_ope(1, 3, str(nsq), where=where)
        r, want = 1, {}
        for k in sorted(full):
            r = r * int(full[k]) % nsq
            want[k] = str(r)
        assert got == want and set(got) == {20260101, 20260102, 20260103}
        for call in (lambda: st.running_sum_by_ope(1, 5, str(nsq)), lambda: st.running_sum_by_ope(1, 3, "x"),
                     lambda: st.running_mult_by_ope(2, 3, "zz")):
            with pytest.raises(ServerError):
                call()
    finally:
        st.close()
