"""The two forms of every scan and grouped fold, one table: each of the eight pairs appends its result rows to a
resident column or writes them out as big-endian bytes, and nothing else may differ between the two. Per pair: the
rows and the side outputs of both forms against a Python big-integer restatement; the appending form refused for an
`out` over another modulus, from another context and one row short of capacity (status, text, `out` untouched, and
the same columns serving a valid call right after, so every lock was released); the bytes form refused for a `cap`
one short (nothing written, the need reported). One extra case: dds_col_append_pow refuses an `out` from another
context like every other append.

70 rows: past one 64-row stride (the bytes forms stage at 128) and more than two chunks of 32 (a second level runs).
"""
import ctypes as C
import random
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROWS, DEAD, NG = 70, 13, 5
KEYS = (-10 ** 9, -3, 0, 4, 10 ** 12)
TEXTS = ("pear", "apple", "apple pie", "Äpfel", "p")
SEG = (0, 5, 33, 64)
WIN = 5
UNSET = 99  # what the side arrays hold before a call
MODULUS_TEXT = "columns must be over the same modulus"
CONTEXT_TEXT = "columns must belong to one context"
CAPACITY_TEXT = "column capacity exceeded"


def prod(xs, N):
    r = 1
    for x in xs:
        r = r * x % N
    return r


def running(xs, N):
    out, r = [], 1
    for x in xs:
        r = r * x % N
        out.append(r)
    return out


@pytest.fixture(scope="module")
def w(eng, keys):
    """the shared columns and, per pair, want[name] = (result rows, side outputs) restated on Python integers"""
    import ddshe
    N, M = keys["paillier1024_seed1"]["nsquare"], keys["paillier2048_committed"]["nsquare"]
    rng = random.Random(2026)
    rows = [rng.randrange(N) for _ in range(ROWS)]
    kidx = list(range(NG)) * 2 + [rng.randrange(NG) for _ in range(ROWS - 2 * NG)]
    rng.shuffle(kidx)
    keyvals, texts = [KEYS[k] for k in kidx], [TEXTS[k] for k in kidx]
    labels = [rng.choice((0, 1, 2, 4)) for _ in range(ROWS)]  # five groups, group 3 without a row
    live = [i for i in range(ROWS) if i != DEAD]
    col, by, tab = eng.column(N, ROWS), eng.opecol(ROWS), eng.strtab([[t] for t in texts])
    col.append(rows)
    col.set_live([DEAD], 0)
    by.append(keyvals)
    eng2 = ddshe.Engine(0)

    want = {}
    want["fold_groups"] = ([prod((rows[i] for i in live if labels[i] == g), N) for g in range(NG)],
                           {"counts": [sum(labels[i] == g for i in live) for g in range(NG)]})
    by_key = {k: [i for i in live if keyvals[i] == k] for k in sorted(KEYS)}
    ks, sizes = list(by_key), [len(m) for m in by_key.values()]
    want["fold_by_ope"] = ([prod((rows[i] for i in m), N) for m in by_key.values()],
                           {"keys": ks, "counts": sizes, "ngroups": NG})
    by_text = {}
    for i in live:
        by_text.setdefault(texts[i], []).append(i)  # order of first occurrence
    want["fold_by_str"] = ([prod((rows[i] for i in m), N) for m in by_text.values()],
                           {"first_rows": [m[0] for m in by_text.values()],
                            "counts": [len(m) for m in by_text.values()], "ngroups": NG, "passes": 1})
    totals = want["fold_by_ope"][0]
    want["scan_by_ope"] = (running(totals[::-1], N)[::-1],  # suffix: the rows with key >= keys[g]
                           {"keys": ks, "counts": np.cumsum(sizes[::-1])[::-1].tolist(), "ngroups": NG})
    want["scan_part_by_ope"] = (sum((running((rows[i] for i in m), N) for m in by_key.values()), []),
                                {"rows": sum(by_key.values(), []), "keys": ks, "counts": sizes,
                                 "nrows": len(live), "ngroups": NG})
    want["scan"] = (running(rows, N), {})
    ends = list(SEG[1:]) + [ROWS]
    want["scan_seg"] = (sum((running(rows[a:b][::-1], N)[::-1] for a, b in zip(SEG, ends)), []), {})  # suffix
    want["window"] = ([prod(rows[max(0, j - WIN + 1):j + 1], N) for j in range(ROWS)], {})
    assert all(sizes) and len(by_text) == NG and 0 in want["fold_groups"][1]["counts"]

    yield types.SimpleNamespace(lib=ddshe._lib, dd=ddshe, eng=eng, eng2=eng2, N=N, M=M, rows=rows, col=col, by=by,
                                tab=tab, labels=np.array(labels, dtype=np.uint32), want=want,
                                seg=np.array(SEG, dtype=np.uint64))
    for c in (col, by, tab):
        c.close()
    eng2.close()


def side_arrays(**dtypes):
    return {k: np.full(ROWS, UNSET, dtype=t) for k, t in dtypes.items()}


def ptr(a):
    return a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def form(w, dst, name, name_be):
    """the entry point of the form `dst` asks for, and dst as its `out` argument"""
    if hasattr(dst, "_h"):
        return getattr(w.lib, name), dst._h
    return getattr(w.lib, name_be), ptr(dst)


# Every pair: call(w, dst, short) runs the appending form on a Column dst, the bytes form on a uint8 array dst (its
# cap `short` below the need), and returns (status, side outputs as lists cut to what the call reported).

def fold_groups(w, dst, short=0):
    s = side_arrays(counts=np.uint64)
    fn, out = form(w, dst, "dds_col_fold_groups", "dds_col_fold_groups_be")
    rc = fn(w.col._h, None, 0, ROWS, ptr(w.labels), NG, out, ptr(s["counts"]))
    return rc, {"counts": s["counts"][:NG].tolist()}


def keyed(name, suffix=None):
    def call(w, dst, short=0):
        s = side_arrays(keys=np.int64, counts=np.uint64)
        ng = C.c_size_t(UNSET)
        fn, out = form(w, dst, name, name + "_be")
        rc = fn(w.col._h, w.by._h, None, 0, *([] if suffix is None else [suffix]), out, ptr(s["keys"]),
                ptr(s["counts"]), NG - short, C.byref(ng))
        n = NG if rc else ng.value
        return rc, {"keys": s["keys"][:n].tolist(), "counts": s["counts"][:n].tolist(), "ngroups": ng.value}
    return call


def fold_by_str(w, dst, short=0):
    s = side_arrays(first_rows=np.uint64, counts=np.uint64)
    ng, passes = C.c_size_t(UNSET), C.c_int(UNSET)
    fn, out = form(w, dst, "dds_col_fold_by_str", "dds_col_fold_by_str_be")
    rc = fn(w.col._h, w.tab._h, 0, None, 0, out, ptr(s["first_rows"]), ptr(s["counts"]), NG - short, C.byref(ng),
            C.byref(passes))
    n = NG if rc else ng.value
    return rc, {"first_rows": s["first_rows"][:n].tolist(), "counts": s["counts"][:n].tolist(), "ngroups": ng.value,
                "passes": passes.value}


def scan_part_by_ope(w, dst, short=0):
    s = side_arrays(rows=np.uint64, keys=np.int64, counts=np.uint64)
    nr, ng = C.c_size_t(UNSET), C.c_size_t(UNSET)
    fn, out = form(w, dst, "dds_col_scan_part_by_ope", "dds_col_scan_part_by_ope_be")
    rc = fn(w.col._h, w.by._h, None, 0, 0, out, ptr(s["rows"]), ROWS - 1 - short, ptr(s["keys"]), ptr(s["counts"]), NG,
            C.byref(nr), C.byref(ng))
    n, g = (ROWS, NG) if rc else (nr.value, ng.value)
    return rc, {"rows": s["rows"][:n].tolist(), "keys": s["keys"][:g].tolist(), "counts": s["counts"][:g].tolist(),
                "nrows": nr.value, "ngroups": ng.value}


def scan(w, dst, short=0):
    if hasattr(dst, "_h"):
        return w.lib.dds_col_append_scan(dst._h, w.col._h, None, 0, ROWS, 0), {}
    return w.lib.dds_col_scan_be(w.col._h, None, 0, ROWS, 0, ptr(dst)), {}


def scan_seg(w, dst, short=0):
    if hasattr(dst, "_h"):
        return w.lib.dds_col_append_scan_seg(dst._h, w.col._h, None, 0, ROWS, ptr(w.seg), len(SEG), 1), {}
    return w.lib.dds_col_scan_seg_be(w.col._h, None, 0, ROWS, ptr(w.seg), len(SEG), 1, ptr(dst)), {}


def window(w, dst, short=0):
    if hasattr(dst, "_h"):
        return w.lib.dds_col_append_window(dst._h, w.col._h, None, 0, ROWS, WIN), {}
    return w.lib.dds_col_window_be(w.col._h, None, 0, ROWS, WIN, ptr(dst)), {}


PAIRS = {"fold_groups": fold_groups, "fold_by_ope": keyed("dds_col_fold_by_ope"), "fold_by_str": fold_by_str,
         "scan_by_ope": keyed("dds_col_scan_by_ope", suffix=1), "scan_part_by_ope": scan_part_by_ope, "scan": scan,
         "scan_seg": scan_seg, "window": window}
CAPPED = ("fold_by_ope", "fold_by_str", "scan_by_ope", "scan_part_by_ope")  # the pairs whose bytes form takes a cap


def unset(side):
    """no side array was written (the counters may have been: they are zeroed or report the need)"""
    return all(set(v) == {UNSET} for v in side.values() if isinstance(v, list))


def appended(w, name, out, at):
    """a valid appending call on `out`, which holds `at` rows: the status, the rows and the side outputs are right"""
    vals, side = w.want[name]
    rc, got = PAIRS[name](w, out)
    assert rc == w.dd.DDS_OK, w.lib.dds_last_error()
    assert got == side and len(out) == at + len(vals) and out.read(at, len(vals)) == vals


@pytest.mark.parametrize("name", list(PAIRS))
def test_both_forms_give_the_same_rows_and_side_outputs(w, name):
    vals, side = w.want[name]
    mb = w.col.mb
    buf = np.full(mb * len(vals), 0xA5, dtype=np.uint8)
    rc, got_be = PAIRS[name](w, buf)
    assert rc == w.dd.DDS_OK, w.lib.dds_last_error()
    raw = buf.tobytes()
    assert [int.from_bytes(raw[j * mb:(j + 1) * mb], "big") for j in range(len(vals))] == vals
    out = w.eng.column(w.N, len(vals) + 2)
    try:
        out.append(w.rows[:2])
        rc, got = PAIRS[name](w, out)
        assert rc == w.dd.DDS_OK, w.lib.dds_last_error()
        assert len(out) == 2 + len(vals) and out.read(0, 2) == w.rows[:2] and out.read(2, len(vals)) == vals
        assert got == got_be == side
    finally:
        out.close()


@pytest.mark.parametrize("refusal", ["modulus", "context", "capacity"])
@pytest.mark.parametrize("name", list(PAIRS))
def test_appending_form_refused_leaves_out_and_the_locks_as_they_were(w, name, refusal):
    vals, _ = w.want[name]
    pre = w.rows[3:5]
    out = {"modulus": lambda: w.eng.column(w.M, len(vals) + 2), "context": lambda: w.eng2.column(w.N, len(vals) + 2),
           "capacity": lambda: w.eng.column(w.N, len(vals) + 1)}[refusal]()
    good = w.eng.column(w.N, len(vals))
    try:
        out.append(pre)
        rc, side = PAIRS[name](w, out)
        assert rc == w.dd.DDS_E_ARG
        assert w.lib.dds_last_error().decode() == {"modulus": MODULUS_TEXT, "context": CONTEXT_TEXT,
                                                   "capacity": CAPACITY_TEXT}[refusal]
        assert len(out) == 2 and out.read(0, 2) == pre and unset(side)
        appended(w, name, good, 0)  # the sources serve the next call
        if refusal == "capacity":  # and so does out, once it has the room
            out.truncate(1)
            appended(w, name, out, 1)
            assert out.read(0, 1) == pre[:1]
        else:
            out.append(pre[:1])
            assert out.read(0, 3) == pre + pre[:1]
    finally:
        out.close()
        good.close()


@pytest.mark.parametrize("name", CAPPED)
def test_bytes_form_one_short_of_room_writes_nothing_and_reports_the_need(w, name):
    vals, side = w.want[name]
    buf = np.full(w.col.mb * len(vals), 0xA5, dtype=np.uint8)
    rc, got = PAIRS[name](w, buf, short=1)
    assert rc == w.dd.DDS_E_BUFSIZE
    assert set(buf.tolist()) == {0xA5} and unset(got)
    assert got["ngroups"] == NG and got.get("nrows", len(vals)) == len(vals)
    rc, got = PAIRS[name](w, buf)  # the same buffers at the size reported
    assert rc == w.dd.DDS_OK and got == side


def test_append_pow_refuses_an_out_of_another_context(w):
    """New with the shared append preamble: before it, dds_col_append_pow skipped this check of the other appends."""
    out = w.eng2.column(w.N, 4)
    try:
        with pytest.raises(w.dd.DDSError) as ei:
            out.append_pow(w.col, 0, 3, [1, 2, 3])
        assert ei.value.status == w.dd.DDS_E_ARG and CONTEXT_TEXT in str(ei.value) and len(out) == 0
    finally:
        out.close()
    good = w.eng.column(w.N, 4)
    try:
        good.append_pow(w.col, 0, 3, [1, 2, 3])
        assert good.read(0, 3) == [pow(x, e, w.N) for x, e in zip(w.rows, (1, 2, 3))]
    finally:
        good.close()
