"""The resident store's SELECT key, SUM(x) [WHERE ...] GROUP BY key (ResidentStore.sum_all_by_ope /
mult_all_by_ope) against a plain-Python restatement over the mirrored rows: a dozen sets with a removed one, one
lacking the grouping position, one that fails the fold's guard, equal contents folded once, "07" and "7" as one
key, with and without a WHERE served by a resident OPE column's search_mask."""
import math
import random

import pytest

pytestmark = pytest.mark.gpu

OPS = {"SearchGt": lambda a, b: a > b, "SearchGtEq": lambda a, b: a >= b, "SearchLt": lambda a, b: a < b,
       "SearchLtEq": lambda a, b: a <= b}


def by_reference(rows, position, by_position, N, where=None):
    """the rows SumAll / MultAll fold (present, strict guard, first of equal contents) that hold an element at
    by_position and pass the WHERE (Search's strict guard at its position), grouped by that element's value"""
    seen, groups = set(), {}
    for row in rows:
        if row is None or not len(row) - 1 > position:
            continue
        sig = tuple(str(v) for v in row)
        if sig in seen:
            continue
        seen.add(sig)
        if not len(row) > by_position:
            continue
        if where is not None:
            route, wpos, bound = where
            if not (len(row) - 1 > wpos and OPS[route](int(row[wpos]), int(bound))):
                continue
        groups.setdefault(int(row[by_position]), []).append(int(row[position]))
    return {k: str(math.prod(xs) % N) for k, xs in groups.items()}


def test_store_sum_all_by_ope_and_mult_all_by_ope(eng, keys):
    from ddshe.routes import NotFound, ServerError
    from ddshe.store import ResidentStore
    nsq = keys["paillier1024_seed1"]["nsquare"]
    rsa = keys["rsa1024_committed"]
    rng = random.Random(91)
    # contents: [name, Paillier c, RSA c, day (OPE), price band (OPE), tail]
    st = ResidentStore(eng, paillier={1: nsq}, rsa={2: rsa["n"]}, ope=(3, 4), capacity=64, strings=False)
    try:
        with pytest.raises(NotFound):
            st.sum_all_by_ope(1, 3, str(nsq))
        days = ["20260101", "20260102", "20260101", "7", "07", "20260102", "-5", "20260101", "7", "20260103"]
        sets = [[f"k{i}", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), d, str(rng.randrange(1, 6)), "x"]
                for i, d in enumerate(days)]
        sets.append(["short", str(rng.randrange(nsq))])  # fails both guards, lacks the grouping position
        sets.append(["noday", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"]))])  # folds in SumAll, no day
        sets.append(["gone", str(rng.randrange(nsq)), str(rng.randrange(rsa["n"])), "20260101", "3", "x"])
        keys_ = st.put_sets(sets)
        st.remove_set(keys_[12])
        st.put_set(list(sets[1]))  # known contents: the same key, nothing new
        for pos in range(6):
            st.write_element(keys_[5], pos, sets[0][pos])  # row 5 now repeats row 0: folded once
        want = by_reference(st.rows(), 1, 3, nsq)
        assert set(want) == {20260101, 20260102, 20260103, 7, -5}  # "07" and "7" are one key
        assert st.sum_all_by_ope(1, 3, str(nsq)) == want
        assert st.mult_all_by_ope(2, 3, rsa["x509_hex"]) == by_reference(st.rows(), 2, 3, rsa["n"])
        assert st.sum_all_by_ope(1, 4, str(nsq)) == by_reference(st.rows(), 1, 4, nsq)  # by price band
        for where in (("SearchGtEq", 3, "20260101"), ("SearchLt", 3, 8), ("SearchGt", 4, "2"),
                      ("SearchLtEq", 4, "0")):
            assert st.sum_all_by_ope(1, 3, str(nsq), where=where) == by_reference(st.rows(), 1, 3, nsq, where), where
        assert st.sum_all_by_ope(1, 3, str(nsq), where=("SearchLtEq", 4, "0")) == {}
        for call in (lambda: st.sum_all_by_ope(1, 5, str(nsq)),  # no OPE column resident there
                     lambda: st.sum_all_by_ope(1, 3, str(nsq), where=("SearchGt", 5, "1")),
                     lambda: st.sum_all_by_ope(1, 3, str(nsq + 2)), lambda: st.sum_all_by_ope(2, 3, str(nsq)),
                     lambda: st.sum_all_by_ope(1, 3, "x"), lambda: st.mult_all_by_ope(2, 3, "zz")):
            with pytest.raises(ServerError):
                call()
        st.put_set(["odd", str(rng.randrange(nsq)), "1", "a day", "1", "x"])  # a key that is no integer: 500
        with pytest.raises(ServerError):
            st.sum_all_by_ope(1, 3, str(nsq))
        assert st.sum_all_by_ope(1, 4, str(nsq)) == by_reference(st.rows(), 1, 4, nsq)  # the other key is fine
    finally:
        st.close()
