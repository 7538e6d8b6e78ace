"""GPU parity of the grouped fold keyed by a resident string table (dds_col_fold_by_str, dds_col_fold_by_str_be) and
of the text egress of its group keys (dds_strtab_read_elems): first rows, counts and every group's value bit-exact
against a plain-Python GROUP BY (a dict by element text in order of first occurrence, the product mod N with Python
ints), in the column and the big-endian form, for group sizes that give one, two and three fold levels, few and many
groups, mixed element types, rows that take no part, tables after writes and a heap compaction, the collision path
under DDSHE_STRKEY_BITS, the errors, Paillier's meaning through the existing decryption, the resident store, and two
threads."""
import ctypes as C
import math
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (1, 31, 32, 33, 1025)  # one level up to 32 rows, two up to 1,024, three above
LONG = "".join(chr(ord("a") + (7 * i) % 26) for i in range(300))
TEXTS = ("", "a", "ab", LONG, LONG[:-1] + "#")  # a proper prefix pair, and 300 bytes differing in the last only
M64 = (1 << 64) - 1


def strkey_digest(b: bytes, salt: int = 0) -> int:
    """csrc/ddshe_strkey.hpp: strkey_digest"""
    h = (0xCBF29CE484222325 ^ (salt * 0x9E3779B97F4A7C15 & M64)) ^ len(b)
    for c in b:
        h = ((h ^ c) * 0x100000001B3) & M64
    h ^= h >> 30
    h = h * 0xBF58476D1CE4E5B9 & M64
    h ^= h >> 27
    h = h * 0x94D049BB133111EB & M64
    return h ^ (h >> 31)


def prod_mod(xs, N):
    r = 1
    for i in range(0, len(xs), 16):
        r = r * math.prod(xs[i:i + 16]) % N
    return r % N


def oracle(rows, trows, position, part, N):
    """(first rows, values, counts, texts) of the rows with part[i] true that hold the position, grouped by the text
    of their element there, the groups in order of first occurrence"""
    import ddshe
    groups, first = {}, {}
    for r, (x, t, p) in enumerate(zip(rows, trows, part)):
        if p and t is not None and len(t) > position:
            k = ddshe.element_text(t[position])
            first.setdefault(k, r)
            groups.setdefault(k, []).append(x)
    ks = list(groups)
    return [first[k] for k in ks], [prod_mod(groups[k], N) for k in ks], [len(groups[k]) for k in ks], ks


def mask_of(part):
    """uint64 words, bit r % 64 of word r / 64 = part[r]: the layout of dds_opecol_search_mask"""
    bits = np.zeros((len(part) + 63) // 64 * 64, dtype=np.uint8)
    bits[:len(part)] = np.asarray(part, dtype=bool)
    return np.packbits(bits, bitorder="little").view(np.uint64)


def check(eng, col, tab, N, rows, trows, position, part, mask=None, passes=1):
    """both forms against the oracle over the rows with part[i] true; passes: the exact count, or (lo,) a minimum"""
    fr, vals, sizes, texts = oracle(rows, trows, position, part, N)
    first, got, counts, np_ = col.fold_by_str(tab, position, mask)
    assert first.dtype == np.uint64 and counts.dtype == np.uint64
    assert first.tolist() == fr and counts.tolist() == sizes
    assert got == vals
    assert np_ >= passes[0] if isinstance(passes, tuple) else np_ == passes, np_
    assert tab.read_elems(first, position) == [t.encode() for t in texts]
    out = eng.column(N, len(fr) + 2)
    try:
        out.append(rows[:2])
        first, counts, np_ = out.append_fold_by_str(col, tab, position, mask)
        assert first.tolist() == fr and counts.tolist() == sizes
        assert np_ >= passes[0] if isinstance(passes, tuple) else np_ == passes, np_
        assert len(out) == 2 + len(fr) and out.live_count == len(out)
        assert out.read(0, 2) == rows[:2] and out.read(2, len(fr)) == vals
    finally:
        out.close()
    return fr, vals, sizes, texts


@pytest.fixture(scope="module")
def base(eng, keys):
    """sum(SIZES) = 1,122 seeded rows below the smallest committed Paillier n² in a resident column, and a string
    table whose element 1 gives groups of exactly SIZES rows, shuffled; every third row ends at that element"""
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(181)
    rows = [rng.randrange(N) for _ in range(sum(SIZES))]
    texts = [t for t, c in zip(TEXTS, SIZES) for _ in range(c)]
    rng.shuffle(texts)
    trows = [[f"k{i}", t] if i % 3 == 0 else [f"k{i}", t, "tail"] for i, t in enumerate(texts)]
    col, tab = eng.column(N, len(rows)), ddshe.StrTable(eng, trows)
    col.append(rows)
    yield N, rows, trows, col, tab
    col.close()
    tab.close()


def test_one_two_and_three_levels(eng, base):
    N, rows, trows, col, tab = base
    _, _, sizes, texts = check(eng, col, tab, N, rows, trows, 1, [True] * len(rows))
    assert sorted(texts) == sorted(TEXTS) and sorted(sizes) == sorted(SIZES)


@pytest.mark.parametrize("ngroups", [3, 300])
def test_few_and_many_groups(eng, keys, ngroups):
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(ngroups)
    n = 700
    rows = [rng.randrange(N) for _ in range(n)]
    texts = [f"dept-{rng.randrange(ngroups)}" for _ in range(n)]
    texts[:ngroups] = [f"dept-{g}" for g in reversed(range(ngroups))]
    trows = [[t, i] for i, t in enumerate(texts)]
    col, tab = eng.column(N, n), ddshe.StrTable(eng, trows)
    try:
        col.append(rows)
        fr, _, _, _ = check(eng, col, tab, N, rows, trows, 0, [True] * n)
        assert fr[:ngroups] == list(range(ngroups))  # first occurrence, not digest or text order
    finally:
        col.close()
        tab.close()


def test_mixed_element_types(eng, keys):
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(182)
    elems = [7, "7", "07", None, "None", True, "true", False, "café", "cafè", "caf", "日本", 7, "07", ""]
    rows = [rng.randrange(N) for _ in elems]
    trows = [["x", e, "y"] for e in elems]
    col, tab = eng.column(N, len(rows)), ddshe.StrTable(eng, trows)
    try:
        col.append(rows)
        fr, _, sizes, texts = check(eng, col, tab, N, rows, trows, 1, [True] * len(rows))
        assert texts == ["7", "07", "None", "true", "false", "café", "cafè", "caf", "日本", ""]
        assert sizes == [3, 2, 2, 2, 1, 1, 1, 1, 1, 1] and fr[:3] == [0, 2, 3]
    finally:
        col.close()
        tab.close()


def test_rows_that_take_no_part(eng, keys):
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(183)
    n = 400
    rows = [rng.randrange(N) for _ in range(n)]
    vals = [rng.randrange(-6, 6) for _ in range(n)]
    # length 1: lacks position 1; length 2: position 1 is the last element and takes part; length 3: inner
    trows = [[str(i), f"g{rng.randrange(9)}", "t"][:rng.choice((1, 2, 3, 3))] for i in range(n)]
    trows[:3] = [["0"], ["1", "g0"], ["2", "g0", "t"]]
    col, tab, ope = eng.column(N, n), ddshe.StrTable(eng, trows), eng.opecol(n)
    try:
        col.append(rows)
        ope.append(vals)
        every = [True] * n
        fr, _, _, _ = check(eng, col, tab, N, rows, trows, 1, every)
        assert fr[0] == 1  # row 0 lacks the position, row 1 ends at it
        dead_col = set(rng.sample(range(n), 60))
        col.set_live(sorted(dead_col), 0)
        part_c = [i not in dead_col for i in range(n)]
        check(eng, col, tab, N, rows, trows, 1, part_c)  # dead in col only
        col.set_live(sorted(dead_col), 1)
        dead_tab = set(rng.sample(range(n), 60)) | {i for i in range(n) if len(trows[i]) > 1 and trows[i][1] == "g5"}
        tab.set_live(sorted(dead_tab), 0)
        part_t = [i not in dead_tab for i in range(n)]
        _, _, _, texts = check(eng, col, tab, N, rows, trows, 1, part_t)  # dead in the table only: a whole key goes
        assert "g5" not in texts
        col.set_live(sorted(dead_col), 0)
        both = [a and b for a, b in zip(part_c, part_t)]
        check(eng, col, tab, N, rows, trows, 1, both)
        for op, pred in (("gt", lambda v: v > 0), ("le", lambda v: v <= -2)):  # a WHERE from a real search_mask
            words, matches = ope.search_mask(0 if op == "gt" else -2, op)
            where = [pred(v) for v in vals]
            assert matches == sum(where)
            check(eng, col, tab, N, rows, trows, 1, [a and b for a, b in zip(both, where)], words)
        tab.set_live(sorted(dead_tab), 1)
        col.set_live(sorted(dead_col), 1)
        # the mask drops every group's first row: first_rows move to the next holder
        fr0, _, sizes0, _ = oracle(rows, trows, 1, every, N)
        assert min(sizes0) >= 2
        part = [i not in set(fr0) for i in range(n)]
        fr1, _, _, _ = check(eng, col, tab, N, rows, trows, 1, part, mask_of(part))
        assert all(b > a for a, b in zip(sorted(fr0), sorted(fr1)))
        first, got, counts, passes = col.fold_by_str(tab, 1, mask_of([False] * n))  # the mask removes every row
        assert len(first) == 0 and got == [] and len(counts) == 0
        first, got, counts, passes = col.fold_by_str(tab, 5)  # no row holds the position
        assert len(first) == 0 and got == [] and len(counts) == 0
        col.set_live(list(range(n)), 0)
        first, got, counts, passes = col.fold_by_str(tab, 1)  # no live row
        assert len(first) == 0 and got == [] and len(counts) == 0
    finally:
        for c in (col, tab, ope):
            c.close()


def test_after_writes_and_a_compaction(eng, keys):
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(184)
    n = 300
    rows = [rng.randrange(N) for _ in range(n)]
    trows = [[f"k{i}", f"g{rng.randrange(7)}", "t" * 20] for i in range(n)]  # 900 elements: room for 124 more
    col, tab = eng.column(N, n), ddshe.StrTable(eng, [list(t) for t in trows])
    try:
        col.append(rows)
        every = [True] * n
        check(eng, col, tab, N, rows, trows, 1, every)
        before = tab.stats()
        ids = rng.sample(range(n), 10)  # moved to other groups, a new one among them; old versions stay in the heap
        for i in ids:
            trows[i] = [f"k{i}", rng.choice(("g0", "g6", "new")), "t", "longer"]
        tab.write_rows(ids, [trows[i] for i in ids])
        assert tab.stats()["heap_elems"] > before["heap_elems"] and tab.stats()["compactions"] == before["compactions"]
        check(eng, col, tab, N, rows, trows, 1, every)
        for _ in range(4):  # rewrites past the heap's room: a compaction
            ids = rng.sample(range(n), 150)
            for i in ids:
                trows[i] = [f"k{i}", f"g{rng.randrange(9)}"]
            tab.write_rows(ids, [trows[i] for i in ids])
        assert tab.stats()["compactions"] > before["compactions"]
        check(eng, col, tab, N, rows, trows, 1, every)
        off = rng.sample(range(n), 40)
        tab.set_live(off, 0)
        check(eng, col, tab, N, rows, trows, 1, [i not in set(off) for i in range(n)])
        tab.set_live(off, 1)
        check(eng, col, tab, N, rows, trows, 1, every)
    finally:
        col.close()
        tab.close()


@pytest.mark.parametrize("bits,equal_length", [(4, False), (1, False), (1, True)])
def test_collision_path(eng, keys, monkeypatch, bits, equal_length):
    """40 distinct values sorted by the top 4 bits (or the top bit) of their digests on the first pass: by pigeonhole
    some segment holds two strings, the verification must reject the pass, and the second pass must be exact.
    Without the switch the fixture's 64-bit digests are distinct, so one pass stands."""
    import ddshe
    N = keys["paillier1024_seed1"]["nsquare"]
    rng = random.Random(185 + bits)
    values = [f"v{i:02d}" if equal_length else "v" * (i % 5) + str(i) for i in range(40)]
    assert len({strkey_digest(v.encode()) for v in values}) == 40  # no 64-bit collision at salt 0
    assert len({strkey_digest(v.encode()) >> (64 - bits) for v in values}) < 40  # a certain one at `bits` bits
    n = 200
    rows = [rng.randrange(N) for _ in range(n)]
    trows = [[values[i % 40] if i < 40 else rng.choice(values), i] for i in range(n)]
    col, tab = eng.column(N, n), ddshe.StrTable(eng, trows)
    try:
        col.append(rows)
        check(eng, col, tab, N, rows, trows, 0, [True] * n, passes=1)
        monkeypatch.setenv("DDSHE_STRKEY_BITS", str(bits))
        check(eng, col, tab, N, rows, trows, 0, [True] * n, passes=(2,))
        part = [rng.randrange(2) == 0 for _ in range(n)]
        check(eng, col, tab, N, rows, trows, 0, part, mask_of(part), passes=(1,))
        monkeypatch.delenv("DDSHE_STRKEY_BITS")
        check(eng, col, tab, N, rows, trows, 0, [True] * n, passes=1)
    finally:
        col.close()
        tab.close()


def test_errors(eng, base):
    import ddshe
    N, rows, trows, col, tab = base
    lib = ddshe._lib
    mb = col.mb
    fr, _, _, _ = oracle(rows, trows, 1, [True] * len(rows), N)
    for cap in (4, 0):
        ng, passes = C.c_size_t(0), C.c_int(0)
        first = (C.c_uint64 * 5)(*[99] * 5)
        counts = (C.c_uint64 * 5)(*[99] * 5)
        buf = (C.c_uint8 * (mb * 5))()
        assert lib.dds_col_fold_by_str_be(col._h, tab._h, 1, None, 0, buf, first, counts, cap, C.byref(ng),
                                          C.byref(passes)) == ddshe.DDS_E_BUFSIZE
        assert ng.value == 5  # the count required
        assert list(first) == [99] * 5 and list(counts) == [99] * 5 and bytes(buf) == bytes(mb * 5)
        out = eng.column(N, 16)
        try:
            out.append(rows[:3])
            ng = C.c_size_t(0)
            assert lib.dds_col_fold_by_str(col._h, tab._h, 1, None, 0, out._h, first, counts, cap, C.byref(ng),
                                           None) == ddshe.DDS_E_BUFSIZE
            assert ng.value == 5 and len(out) == 3 and list(first) == [99] * 5
            assert lib.dds_col_fold_by_str(col._h, tab._h, 1, None, 0, out._h, first, None, 5, C.byref(ng),
                                           None) == ddshe.DDS_OK  # counts and passes are nullable
            assert ng.value == 5 and len(out) == 8 and list(first) == fr and list(counts) == [99] * 5
        finally:
            out.close()
    small = eng.column(N, 4)  # room in first_rows and counts, not in the output column
    short = ddshe.StrTable(eng, trows[:8])
    try:
        with pytest.raises(ddshe.DDSError) as ei:
            small.append_fold_by_str(col, tab, 1)
        assert ei.value.status == ddshe.DDS_E_ARG and len(small) == 0
        for call in (lambda: col.fold_by_str(short, 1), lambda: small.append_fold_by_str(col, short, 1),  # rows differ
                     lambda: col.append_fold_by_str(col, tab, 1),  # out == col
                     lambda: col.fold_by_str(tab, 1, mask_of([True] * len(rows))[:-1])):  # one word short
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
        assert len(small) == 0
    finally:
        small.close()
        short.close()


def test_paillier_meaning_under_the_2048_bit_key(eng, keys):
    import ddshe
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(186)
    ms = [rng.randrange(10000) for _ in range(150)]
    rs = [rng.randrange(1, n) for _ in ms]
    depts = [rng.choice(("sales", "ops", "r&d", "legal", "")) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    trows = [[d, "x"] for d in depts]
    src, tab, out = eng.column(nsq, 150), ddshe.StrTable(eng, trows), eng.column(nsq, 8)
    try:
        src.append(cs)
        _, _, _, texts = check(eng, src, tab, nsq, cs, trows, 0, [True] * 150)
        first, counts, _ = out.append_fold_by_str(src, tab, 0)
        sums = [sum(m for m, d in zip(ms, depts) if d == t) % n for t in texts]
        assert counts.tolist() == [depts.count(t) for t in texts]
        assert out.decrypt_paillier(0, len(texts), key["p"], key["q"], g) == sums
    finally:
        for c in (src, tab, out):
            c.close()


def test_read_elems(eng):
    import ddshe
    trows = [["a", "bb", "ccc"], ["only"], ["x", "", "z"], ["dead", "row"], ["e", "é" * 40, LONG]]
    tab = ddshe.StrTable(eng, trows)
    try:
        tab.set_live([3], 0)
        ids = [4, 0, 1, 3, 2, 0, 4]  # a short row, a dead row, repeated ids
        for position in (0, 1, 2, 3):
            want = [None if r == 3 or len(trows[r]) <= position else trows[r][position].encode() for r in ids]
            assert tab.read_elems(ids, position) == want
        assert tab.read_elems([], 0) == []
        lib = ddshe._lib
        rows = np.asarray(ids, dtype=np.uint64)
        total = sum(len(trows[r][1].encode()) for r in ids if r != 3 and len(trows[r]) > 1)
        offs = np.full(len(ids) + 1, 99, dtype=np.uint64)
        pres = np.full(len(ids), 9, dtype=np.uint8)
        buf = C.create_string_buffer(total)
        need = C.c_size_t(0)
        args = (tab._h, rows.ctypes.data_as(C.POINTER(C.c_uint64)), len(ids), 1, buf)
        tail = (offs.ctypes.data_as(C.POINTER(C.c_uint64)), pres.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(need))
        assert lib.dds_strtab_read_elems(*args, total - 1, *tail) == ddshe.DDS_E_BUFSIZE  # one byte short
        assert need.value == total and buf.raw == bytes(total) and offs.tolist() == [99] * (len(ids) + 1)
        assert pres.tolist() == [9] * len(ids)
        assert lib.dds_strtab_read_elems(*args, total, *tail) == ddshe.DDS_OK
        assert need.value == total and int(offs[-1]) == total and pres.tolist() == [1, 1, 0, 0, 1, 1, 1]
        assert buf.raw == b"".join(trows[r][1].encode() for r in ids if r != 3 and len(trows[r]) > 1)
        rows[2] = len(trows)  # out of range
        assert lib.dds_strtab_read_elems(*args, total, *tail) == ddshe.DDS_E_ARG
    finally:
        tab.close()


def test_store_sum_all_by_str_and_mult_all_by_str(eng, keys):
    from ddshe.routes import NotFound, ServerError
    from ddshe.store import ResidentStore
    nsq = keys["paillier1024_seed1"]["nsquare"]
    rsa = keys["rsa1024_committed"]
    rng = random.Random(187)
    # contents: [name, Paillier c, RSA c, day (OPE), department, tail]
    st = ResidentStore(eng, paillier={1: nsq}, rsa={2: rsa["n"]}, ope=(3,), capacity=64, strings=True)
    bare = ResidentStore(eng, paillier={1: nsq}, capacity=8, strings=False)
    try:
        with pytest.raises(NotFound):
            st.sum_all_by_str(1, 4, str(nsq))
        depts = ["sales", "ops", "sales", "7", "07", "ops", "", "sales", 7, "r&d"]
        sets = [[f"k{i}", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), str(20260101 + i % 4), d, "x"]
                for i, d in enumerate(depts)]
        sets.append(["short", str(rng.randrange(nsq))])  # fails both guards, lacks the grouping position
        sets.append(["nodept", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "20260101"])
        sets.append(["gone", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "20260101", "sales", "x"])
        keys_ = st.put_sets(sets)
        st.remove_set(keys_[12])
        st.write_element(keys_[1], 4, "legal")  # rewrites: a row moves to a new group, one joins an old one
        st.write_element(keys_[9], 4, "ops")
        st.add_element(keys_[11], "late")  # now holds the grouping position
        for pos in range(6):
            st.write_element(keys_[5], pos, st.rows()[0][pos])  # row 5 now repeats row 0: folded once
        got = st.sum_all_by_str(1, 4, str(nsq))
        want = st.sum_all_by(1, 4, str(nsq))
        assert got == want and list(got) == list(want)
        assert {"sales", "7", "07", "", "legal", "ops", "late"} <= set(got)  # the Int 7 and "7" are one group
        got = st.mult_all_by_str(2, 4, rsa["x509_hex"])
        want = st.mult_all_by(2, 4, rsa["x509_hex"])
        assert got == want and list(got) == list(want)
        for where, pred in ((("SearchGtEq", 3, "20260102"), lambda d: d >= 20260102),
                            (("SearchLt", 3, 20260101), lambda d: False)):
            groups, seen = {}, set()
            for row in st.rows():  # the rows SumAll folds that hold the department and pass the WHERE
                if row is None or not len(row) - 1 > 1 or tuple(map(str, row)) in seen:
                    continue
                seen.add(tuple(map(str, row)))
                if len(row) > 4 and len(row) - 1 > 3 and pred(int(row[3])):
                    groups.setdefault(str(row[4]), []).append(int(row[1]))
            assert st.sum_all_by_str(1, 4, str(nsq), where=where) == {k: str(math.prod(v) % nsq)
                                                                      for k, v in groups.items()}, where
        for call in (lambda: st.sum_all_by_str(1, 4, str(nsq + 2)), lambda: st.sum_all_by_str(2, 4, str(nsq)),
                     lambda: st.sum_all_by_str(1, 4, "x"), lambda: st.mult_all_by_str(2, 4, "zz"),
                     lambda: st.sum_all_by_str(1, 4, str(nsq), where=("SearchGt", 5, "1"))):
            with pytest.raises(ServerError):
                call()
        bare.put_sets([["a", str(rng.randrange(nsq)), "d"], ["b", str(rng.randrange(nsq)), "d"]])
        with pytest.raises(ServerError):
            bare.sum_all_by_str(1, 2, str(nsq))  # no string table resident
    finally:
        st.close()
        bare.close()


def test_two_threads_on_one_context(base):
    N, rows, trows, col, tab = base
    rng = random.Random(188)
    parts = [[True] * len(rows), [rng.randrange(2) == 0 for _ in rows]]
    masks = [None, mask_of(parts[1])]
    want = [oracle(rows, trows, 1, p, N)[:3] for p in parts]
    got = [None, None]

    def run(i):
        for _ in range(3):
            first, vals, counts, _ = col.fold_by_str(tab, 1, masks[i])
            got[i] = (first.tolist(), vals, counts.tolist())

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == [tuple(w) for w in want]
