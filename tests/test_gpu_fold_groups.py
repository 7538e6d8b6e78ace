"""GPU parity of the grouped SumAll / MultAll (dds_col_fold_groups, dds_col_fold_groups_be): every group's value
bit-exact against Python's math.prod(rows of the group) % N, for one modulus per lane-group shape, group sizes on
both sides of the fan (32 rows per lane group and level) and of its square, a skewed call, both regimes of the
counting sort (counters in LDS up to 256 groups, global above), the row_ids and range forms, liveness, the argument
errors, the resident column form, Paillier's meaning Dec(group's product) = sum of the group's m through the
existing encryption and decryption, the store's sum_all_by / mult_all_by, and two threads on one context."""
import math
import random
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# modulus -> (key, field): S = 40 / TPI 2, S = 76 / TPI 2, S = 148 / TPI 4, S = 232 / TPI 8
MODULI = {"rsa1024": ("rsa1024_committed", "n"), "nsq1024": ("paillier1024_seed1", "nsquare"),
          "nsq2048": ("paillier2048_committed", "nsquare"), "nsq3072": ("paillier3072_seed4", "nsquare")}
# seeded odd moduli with the top bit set: S = 112 / TPI 4, S = 320 / TPI 16, S = 640 / TPI 32
WIDE_BITS = (3000, 8000, 16384)


def modulus(keys, name):
    key, field = MODULI[name]
    return keys[key][field]


def prod_mod(xs, N):
    """math.prod(xs) % N, reduced every 16 factors (the unreduced product of 5,000 rows takes Python 20 s)"""
    r = 1
    for i in range(0, len(xs), 16):
        r = r * math.prod(xs[i:i + 16]) % N
    return r % N


def reference(rows, labels, ngroups, N):
    groups = [[] for _ in range(ngroups)]
    for x, g in zip(rows, labels):
        groups[g].append(x)
    return [prod_mod(xs, N) for xs in groups], [len(xs) for xs in groups]


def check(col, N, rows, labels, ngroups, **kw):
    """fold_groups over all of `rows` (the column's content) against the reference"""
    vals, counts = col.fold_groups(labels, ngroups, **kw)
    want, sizes = reference(rows, labels, ngroups, N)
    assert counts.dtype == np.uint64 and counts.tolist() == sizes
    assert vals == want


def few_groups(rng, count):
    """5 groups: 0..2 seeded, 3 left empty, 4 a singleton"""
    labels = [rng.randrange(3) for _ in range(count)]
    labels[count // 2] = 4
    return labels


def one_shape(eng, N, rng, count):
    rows = [rng.randrange(N) for _ in range(count)]
    rows[1] = N - 1
    labels = few_groups(rng, count)
    col = eng.column(N, count)
    try:
        col.append(rows)
        vals, counts = col.fold_groups(labels, 5)
        want, sizes = reference(rows, labels, 5, N)
        assert counts.tolist() == sizes and sizes[3] == 0 and sizes[4] == 1
        assert vals == want and vals[3] == 1 and vals[4] == rows[count // 2]
    finally:
        col.close()


@pytest.mark.parametrize("name", list(MODULI))
def test_one_modulus_per_key_shape(eng, keys, name):
    one_shape(eng, modulus(keys, name), random.Random(41), 40)


@pytest.mark.parametrize("bits", WIDE_BITS)
def test_one_modulus_per_wide_shape(eng, bits):
    rng = random.Random(bits)
    N = rng.getrandbits(bits) | (1 << (bits - 1)) | 1
    one_shape(eng, N, rng, 9)


SIZES = (1, 2, 31, 32, 33, 64, 1023, 1024, 1025)


@pytest.fixture(scope="module")
def base(eng, keys):
    """sum(SIZES) = 3,235 seeded rows below the committed RSA modulus in a resident column, and labels that give
    groups of exactly SIZES rows, shuffled"""
    N = modulus(keys, "rsa1024")
    rng = random.Random(52)
    rows = [rng.randrange(N) for _ in range(sum(SIZES))]
    labels = [g for g, c in enumerate(SIZES) for _ in range(c)]
    rng.shuffle(labels)
    col = eng.column(N, len(rows))
    col.append(rows)
    yield N, rows, labels, col
    col.close()


def test_group_sizes_around_the_fan(base):
    N, rows, labels, col = base
    vals, counts = col.fold_groups(labels, len(SIZES))
    assert counts.tolist() == list(SIZES)
    assert vals == reference(rows, labels, len(SIZES), N)[0]


def test_two_upper_levels_at_148_limbs(eng, keys):
    N = modulus(keys, "nsq2048")
    rng = random.Random(53)
    rows = [rng.randrange(N) for _ in range(1025 + 3)]
    labels = [1] * 1025 + [0, 2, 2]  # 1,025 rows: 33 chunks, 2 chunks, 1 chunk
    rng.shuffle(labels)
    col = eng.column(N, len(rows))
    try:
        col.append(rows)
        check(col, N, rows, labels, 3)
    finally:
        col.close()


def test_one_large_group_beside_singletons(eng, keys):
    N = modulus(keys, "nsq1024")
    rng = random.Random(54)
    rows = [rng.randrange(N) for _ in range(5300)]
    labels = [0] * 5000 + list(range(1, 301))
    rng.shuffle(labels)
    col = eng.column(N, len(rows))
    try:
        col.append(rows)
        check(col, N, rows, labels, 301)
    finally:
        col.close()


@pytest.mark.parametrize("ngroups", [256, 257])
def test_both_sides_of_the_sort_threshold(base, ngroups):
    N, rows, _, col = base
    rng = random.Random(ngroups)
    labels = [rng.randrange(ngroups) for _ in rows]
    labels[0], labels[1] = 0, ngroups - 1
    check(col, N, rows, labels, ngroups)


def test_mostly_empty_groups(base):
    """70,000 groups over 2,000 rows: the scan runs over more than one tile of counters"""
    N, rows, _, col = base
    rng = random.Random(55)
    labels = [rng.randrange(70000) for _ in range(2000)]
    labels[0], labels[1], labels[2] = 0, 69999, 69999
    check(col, N, rows[:2000], labels, 70000, first=0, count=2000)


def test_identities(base):
    N, rows, _, col = base
    vals, counts = col.fold_groups([0] * len(rows), 1)
    assert vals == [col.fold() % N] and counts.tolist() == [len(rows)]
    vals, counts = col.fold_groups(list(range(len(rows))), len(rows))
    assert vals == col.read(0, len(rows)) == rows and counts.tolist() == [1] * len(rows)


def test_row_ids_and_range_forms(base):
    N, rows, _, col = base
    rng = random.Random(56)
    ids = [rng.randrange(len(rows)) for _ in range(90)] + [17, 17, 17]  # a row listed more than once
    labels = [rng.randrange(4) for _ in ids]
    labels[-3:] = [2, 2, 3]
    vals, counts = col.fold_groups(labels, 4, row_ids=ids)
    want, sizes = reference([rows[i] for i in ids], labels, 4, N)
    assert vals == want and counts.tolist() == sizes
    labels = [rng.randrange(3) for _ in range(100)]
    vals, counts = col.fold_groups(labels, 3, first=1000, count=100)
    want, sizes = reference(rows[1000:1100], labels, 3, N)
    assert vals == want and counts.tolist() == sizes
    vals, counts = col.fold_groups([], 3, first=5, count=0)  # no row: every group empty
    assert vals == [1, 1, 1] and counts.tolist() == [0, 0, 0]
    assert col.fold_groups([], 0, first=0, count=0)[0] == []


def test_dead_rows_drop_out(eng, keys):
    N = modulus(keys, "nsq2048")
    rng = random.Random(57)
    rows = [rng.randrange(N) for _ in range(120)]
    labels = [rng.randrange(4) for _ in rows]
    dead = sorted(rng.sample(range(120), 30) + [i for i in range(120) if labels[i] == 3 and i > 10])
    dead = sorted(set(dead))
    col = eng.column(N, 120)
    try:
        col.append(rows)
        col.set_live(dead, 0)
        alive = [i for i in range(120) if i not in set(dead)]
        want, sizes = reference([rows[i] for i in alive], [labels[i] for i in alive], 4, N)
        vals, counts = col.fold_groups(labels, 4)
        assert vals == want and counts.tolist() == sizes
        ids = list(range(119, -1, -1))  # the row_ids form drops them with their labels too
        vals, counts = col.fold_groups([labels[i] for i in ids], 4, row_ids=ids)
        assert vals == want and counts.tolist() == sizes
        col.set_live(list(range(120)), 0)
        vals, counts = col.fold_groups(labels, 4)
        assert vals == [1] * 4 and counts.tolist() == [0] * 4
    finally:
        col.close()


def test_argument_errors(eng, keys):
    import ddshe
    N = modulus(keys, "nsq2048")
    rows = [random.Random(58).randrange(N) for _ in range(6)]
    src, out, small = eng.column(N, 8), eng.column(N, 8), eng.column(N, 3)
    other = eng.column(modulus(keys, "nsq1024"), 8)
    try:
        src.append(rows)
        out.append(rows[:2])
        small.append(rows[:1])
        bad = [lambda: out.append_fold_groups(src, [0, 1, 2, 3, 1, 0], 3),  # a label equal to ngroups
               lambda: src.fold_groups([0, 1, 2, 3, 1, 0], 3),
               lambda: other.append_fold_groups(src, [0] * 6, 1),  # out over another modulus
               lambda: small.append_fold_groups(src, [0, 1, 2, 0, 1, 2], 3),  # capacity short by one row
               lambda: out.append_fold_groups(src, [0, 0], 1, row_ids=[0, 6]),  # a row id out of range
               lambda: out.append_fold_groups(src, [0, 0], 1, first=5, count=2),  # rows past the end
               lambda: src.append_fold_groups(src, [0] * 6, 1)]  # out == col
        for call in bad:
            with pytest.raises(ddshe.DDSError) as ei:
                call()
            assert ei.value.status == ddshe.DDS_E_ARG
        with pytest.raises(ddshe.DDSError) as ei:
            src.fold_groups([0, 1, 2, 3, 1, 0], 3)
        assert "index 3" in str(ei.value)  # dds_last_error names the label's index
        assert len(out) == 2 and len(small) == 1 and len(other) == 0 and len(src) == 6
        assert out.read(0, 2) == rows[:2]
        small.append_fold_groups(src, [0, 1, 0, 1, 0, 1], 2)  # exactly the capacity
        assert len(small) == 3
    finally:
        for c in (src, out, small, other):
            c.close()


def test_append_fold_groups_stays_resident(eng, keys):
    N = modulus(keys, "nsq2048")
    rng = random.Random(59)
    rows = [rng.randrange(N) for _ in range(100)]
    labels = [rng.randrange(6) for _ in rows]
    src, out = eng.column(N, 100), eng.column(N, 64)  # different strides
    try:
        src.append(rows)
        out.append(rows[:3])
        counts = out.append_fold_groups(src, labels, 6)
        want, sizes = reference(rows, labels, 6, N)
        assert counts.tolist() == sizes
        assert len(out) == 9 and out.live_count == 9
        assert out.read(0, 3) == rows[:3] and out.read(3, 6) == want
        assert out.read_dec(3, 6) == [str(v) for v in want]
        assert out.fold(3, 6) == math.prod(want) % N  # the new rows are live
        counts = out.append_fold_groups(src, labels[:50], 6, first=50, count=50)  # behind those again
        assert len(out) == 15 and out.read(9, 6) == reference(rows[50:], labels[:50], 6, N)[0]
    finally:
        src.close()
        out.close()


def test_paillier_meaning(eng, keys):
    key = keys["paillier2048_committed"]
    n, nsq, g = key["n"], key["nsquare"], key["g"]
    rng = random.Random(60)
    ms = [rng.randrange(10000) for _ in range(200)]
    rs = [rng.randrange(1, n) for _ in ms]
    labels = [rng.randrange(7) for _ in ms]
    cs = eng.paillier_encrypt_batch(n, g, ms, rs)
    src, out = eng.column(nsq, 200), eng.column(nsq, 7)
    try:
        src.append(cs)
        counts = out.append_fold_groups(src, labels, 7)
        sums = [sum(m for m, lab in zip(ms, labels) if lab == k) % n for k in range(7)]
        assert counts.tolist() == [labels.count(k) for k in range(7)]
        assert out.decrypt_paillier(0, 7, key["p"], key["q"], g) == sums
    finally:
        src.close()
        out.close()


def _by_reference(rows, position, by_position, N):
    """the rows SumAll / MultAll fold (present, strict guard, first of equal contents), grouped by the text of the
    element at by_position among those that have one"""
    from ddshe.store import _elem_str
    seen, groups = set(), {}
    for row in rows:
        if row is None or not len(row) - 1 > position:
            continue
        sig = tuple(str(v) for v in row)
        if sig in seen:
            continue
        seen.add(sig)
        if len(row) > by_position:
            groups.setdefault(_elem_str(row[by_position]), []).append(int(row[position]))
    return {text: str(math.prod(xs) % N) for text, xs in groups.items()}


def test_store_sum_all_by_and_mult_all_by(eng, keys):
    from ddshe.routes import NotFound, ServerError
    from ddshe.store import ResidentStore
    nsq = modulus(keys, "nsq1024")
    rsa = keys["rsa1024_committed"]
    rng = random.Random(61)
    st = ResidentStore(eng, paillier={1: nsq}, rsa={2: rsa["n"]}, capacity=256, strings=False)
    try:
        with pytest.raises(NotFound):
            st.sum_all_by(1, 4, str(nsq))
        depts = ["ops", "dev", "ops", "hr", "dev", "ops", True, None, 7]
        sets = [[f"k{i}", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "x", d] for i, d in enumerate(depts)]
        sets.append(["short", str(rng.randrange(nsq))])  # fails both guards
        sets.append(["noby", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "x"])  # no element 4
        keys_ = st.put_sets(sets)
        st.write_element(keys_[5], 0, "k0")  # row 5 now repeats ... not yet: its ciphertexts differ
        for pos in (1, 2):
            st.write_element(keys_[5], pos, sets[0][pos])  # ... now it does: folded once
        want = _by_reference(st.rows(), 1, 4, nsq)
        assert set(want) == {"ops", "dev", "hr", "true", "None", "7"}
        assert st.sum_all_by(1, 4, str(nsq)) == want
        assert st.mult_all_by(2, 4, rsa["x509_hex"]) == _by_reference(st.rows(), 2, 4, rsa["n"])
        assert st.sum_all_by(1, 0, str(nsq)) == _by_reference(st.rows(), 1, 0, nsq)  # every row its own group
        assert st.sum_all_by(1, 9, str(nsq)) == {}  # no row holds the element
        for call in (lambda: st.sum_all_by(1, 4, str(nsq + 2)), lambda: st.sum_all_by(3, 4, str(nsq)),
                     lambda: st.sum_all_by(1, 4, "x"), lambda: st.mult_all_by(2, 4, "zz")):
            with pytest.raises(ServerError):
                call()
        st.put_set(["bad", "not a number", "1", "x", "ops"])  # makes sum_all answer 500
        with pytest.raises(ServerError):
            st.sum_all(1, str(nsq))
        with pytest.raises(ServerError):
            st.sum_all_by(1, 4, str(nsq))
    finally:
        st.close()


def test_two_threads_on_one_context(base):
    N, rows, labels, col = base
    rng = random.Random(62)
    jobs = [(labels, len(SIZES)), ([rng.randrange(300) for _ in rows], 300)]
    want = [reference(rows, lab, ng, N) for lab, ng in jobs]
    got = [None, None]

    def run(i):
        for _ in range(3):
            vals, counts = col.fold_groups(*jobs[i])
            got[i] = (vals, counts.tolist())

    ts = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert got == want
