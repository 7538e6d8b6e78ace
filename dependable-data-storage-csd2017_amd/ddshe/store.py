"""Resident store: the proxy's view of its stored sets kept on the GPU across requests.

The reference re-fetches every stored set on every aggregation request (``storedKeys.map(fetchSet)``,
``src/main/scala/dds/http/DDSRestServer.scala:401-403``) and folds / filters them on one core. Here
the proxy keeps one resident column per aggregated position instead — the Paillier column of SumAll,
the RSA column of MultAll, the OPE column of Search / Order — and updates it on each successful write
route, so every read route is one GPU call over rows already in HBM:

  PutSet      (:170-205)  a new key appends a row; known contents rewrite their key's row
  AddElement  (:220-255)  the set grows: the row's element at a position may appear, its guard class
                          may change (``length-1 > position`` is strict for SumAll/MultAll/Search)
  WriteElement(:281-321)  the element at a position changes (or the set grows)
  RemoveSet   (:207-218)  the set becomes None: the row leaves every fold, Search and Order

A row stands for one stored key. Per ciphertext column the row is LIVE when the route's loop would
fold it: the set is present, passes the strict guard, parses as an integer, and is the first row of
its content (SumAll/MultAll collapse equal sets: ``Future.sequence`` over a Set, ``:401-403``). The
C-ABI keeps the live mask on the device (``dds_col_set_live``) and folds only live rows; row values
change by ``dds_col_write_rows_dec``. The OPE column carries each row's class (lacks the position /
last element / elements follow) and a live flag (set present), ``dds_opecol_write_rows_dec`` /
``dds_opecol_set_live``. The string table (``dds_strtab``) holds every row's contents for the
deterministic-equality scans (SearchEq/NEq :607-681, SearchEntry/OR/AND :831-938, IsElement
:322-353): a write gives the row new contents (``dds_strtab_write_rows``), RemoveSet clears its live
byte (``dds_strtab_set_live``). Requests the resident columns cannot answer bit for bit (another
modulus than the column's, the plain add / multiply branch without ``nsqr`` / ``pubkey``, a position
without a column) go through ``ddshe.routes`` over the mirrored rows, which is the same batched engine
path the route would take without a resident column.
"""
from __future__ import annotations

import hashlib

import numpy as np

from . import DDSError, Engine, OPE_CLS_INNER, OPE_CLS_LACKS, OPE_CLS_LAST, StrTable
from . import NotFound as _EngineNotFound
from . import routes
from .routes import NotFound, ServerError, _dec_text, _value_key, entry_needle
from .x509 import rsa_modulus


def _elem_str(v) -> str:
    # toString of an AnyJsonFormat element (DDSJsonProtocol.scala:22-28)
    if v is None:
        return "None"
    if isinstance(v, bool):
        return "true" if v else "false"
    return str(v)


def key_from_set(contents) -> str:
    """Utils.getKeyFromSet (Utils.scala:15-18, SHA-512 per dds-system.conf:99): upper-case hex digest of
    ``DDSSet(contents).toString`` = ``DDSSet(List(e1, e2, ...))``."""
    text = "DDSSet(List(" + ", ".join(_elem_str(v) for v in contents) + "))"
    return hashlib.sha512(text.encode("utf-8")).hexdigest().upper()


def _bigint(v):
    """new BigInteger(v.toString) (any Unicode decimal digits, optional sign), or None if it throws."""
    s = _dec_text(v)
    body = s[1:] if s[:1] in "+-" else s
    if not body or not body.isascii() or not body.isdigit():
        return None
    x = int(body)
    return -x if s[:1] == "-" else x


class _CipherColumn:
    """One resident Paillier (SumAll) or RSA (MultAll) column at `position` under `modulus`."""

    def __init__(self, eng: Engine, position: int, modulus: int, capacity: int):
        self.position, self.modulus = position, int(modulus)
        self.col = eng.column(self.modulus, capacity)
        # limb capacity of the resident format: wider operands are stored reduced (the fold's result
        # is the same; a one-operand reply is answered from the host's copy)
        self.cap_bits = self.modulus.bit_length() + 2
        self.live = np.zeros(capacity, dtype=bool)  # per row: folds it (the engine's live mask)
        self.nlive = 0
        self.bad = set()    # rows that qualify but do not parse: the route answers 500

    def mark(self, r, live: bool, bad: bool):
        self.nlive += int(live) - int(self.live[r])
        self.live[r] = live
        (self.bad.add if bad else self.bad.discard)(r)

    def encode(self, value) -> tuple[str, bool]:
        """(engine text, parses) of an element"""
        x = _bigint(value)
        if x is None:
            return "1", False
        if x.bit_length() >= self.cap_bits:
            x %= self.modulus
        return str(x), True


class ResidentStore:
    """Host mirror of the proxy's stored sets with resident GPU columns (see the module docstring).

    paillier: {position: n^2} — SumAll columns (the client's ``nsqr``, DDSHttpClient.scala:228-240)
    rsa:      {position: n}   — MultAll columns (the modulus of the client's ``pubkey``)
    ope:      positions of OPE columns (Search{Gt,GtEq,Lt,LtEq}, OrderLS/OrderSL)
    strings:  keep a resident string table (SearchEq/NEq, SearchEntry/OR/AND, IsElement)
    Keys are derived as the reference derives them (SHA-512 of the set's text); the mirror's row order
    is insertion order.
    """

    def __init__(self, eng: Engine, paillier=None, rsa=None, ope=(), capacity: int = 1 << 16, strings: bool = True):
        self.eng, self.capacity = eng, capacity
        self.keys: list[str] = []
        self.row: dict[str, int] = {}
        self.val: list = []
        self.groups: dict[tuple, list[int]] = {}  # content signature -> rows holding it (ascending)
        self.cols = [_CipherColumn(eng, p, m, capacity) for p, m in (paillier or {}).items()]
        self.cols += [_CipherColumn(eng, p, m, capacity) for p, m in (rsa or {}).items()]
        self.by_pos_sum = {c.position: c for c in self.cols[:len(paillier or {})]}
        self.by_pos_mult = {c.position: c for c in self.cols[len(paillier or {}):]}
        self.ope = {p: eng.opecol(capacity) for p in ope}
        self.tab = StrTable(eng, []) if strings else None

    def close(self):
        for c in self.cols:
            c.col.close()
        for oc in self.ope.values():
            oc.close()
        if self.tab is not None:
            self.tab.close()

    # ---- row state ----
    @staticmethod
    def _sig(contents):
        return None if contents is None else tuple(_value_key(v) for v in contents)

    def _canonical(self, r) -> bool:
        s = self._sig(self.val[r])
        return s is not None and self.groups[s][0] == r

    def _cipher_state(self, c: _CipherColumn, r):
        """(engine text, live, bad) of row r in column c"""
        row = self.val[r]
        if row is None or len(row) <= c.position:
            return "1", False, False
        text, ok = c.encode(row[c.position])
        qualifies = len(row) - 1 > c.position and self._canonical(r)  # DDSRestServer.scala:415 / :509
        return text, qualifies and ok, qualifies and not ok

    def _ope_state(self, p, r):
        """(text, class, is_string, live) of row r in the OPE column at p"""
        row = self.val[r]
        if row is None:
            return None, OPE_CLS_LACKS, 0, False
        last = len(row) - 1
        cls = OPE_CLS_INNER if last > p else OPE_CLS_LAST if last == p else OPE_CLS_LACKS
        if cls == OPE_CLS_LACKS:
            return None, cls, 0, True
        v = row[p]
        return _dec_text(v), cls, 1 if isinstance(v, str) else 0, True

    def _regroup(self, r, old, new):
        """move row r between content groups; rows whose canonical status may have changed"""
        touched = {r}
        so, sn = self._sig(old), self._sig(new)
        if so == sn:
            return touched
        if so is not None:
            g = self.groups[so]
            if g[0] == r and len(g) > 1:
                touched.add(g[1])
            g.remove(r)
            if not g:
                del self.groups[so]
        if sn is not None:
            g = self.groups.setdefault(sn, [])
            if g and r < g[0]:
                touched.add(g[0])
            g.append(r)
            g.sort()
        return touched

    def _apply(self, rows):
        """push the current state of `rows` (existing rows) into every resident column"""
        rows = sorted(rows)
        ids = np.asarray(rows, dtype=np.uint64)
        for c in self.cols:
            st = [self._cipher_state(c, r) for r in rows]
            c.col.write_rows_dec(ids, [t for t, _, _ in st])
            c.col.set_live(ids, [1 if lv else 0 for _, lv, _ in st])
            for r, (_, lv, bad) in zip(rows, st):
                c.mark(r, lv, bad)
        for p, oc in self.ope.items():
            st = [self._ope_state(p, r) for r in rows]
            oc.write_rows_dec(ids, [t for t, _, _, _ in st], [k for _, k, _, _ in st], [s for _, _, s, _ in st])
            oc.set_live(ids, [1 if lv else 0 for _, _, _, lv in st])

    def _append(self, keys, contents):
        """new rows for new keys (one batched append per column); a failed append leaves the store and
        every column as they were"""
        r0 = len(self.keys)
        if r0 + len(keys) > self.capacity:
            raise ServerError("resident store capacity exceeded")
        for k, cont in zip(keys, contents):
            self.row[k] = len(self.keys)
            self.keys.append(k)
            self.val.append(None if cont is None else list(cont))
        touched = set()
        for i, cont in enumerate(contents):
            touched |= self._regroup(r0 + i, None, self.val[r0 + i])
        new = range(r0, r0 + len(keys))
        try:
            for c in self.cols:
                st = [self._cipher_state(c, r) for r in new]
                c.col.append_dec([t for t, _, _ in st])
                for r, (_, lv, bad) in zip(new, st):
                    c.mark(r, lv, bad)
                dead = [r for r, (_, lv, _) in zip(new, st) if not lv]
                if dead:
                    c.col.set_live(np.asarray(dead, dtype=np.uint64), 0)
            for p, oc in self.ope.items():
                st = [self._ope_state(p, r) for r in new]
                oc.append_dec([t for t, _, _, _ in st], [k for _, k, _, _ in st], [s for _, _, s, _ in st])
                dead = [r for r, (_, _, _, lv) in zip(new, st) if not lv]
                if dead:
                    oc.set_live(np.asarray(dead, dtype=np.uint64), 0)
            if self.tab is not None:
                self.tab.append([self.val[r] or [] for r in new])
                dead = [r for r in new if self.val[r] is None]
                if dead:
                    self.tab.set_live(np.asarray(dead, dtype=np.uint64), 0)
        except Exception:
            self._rollback(r0)
            raise
        old = touched - set(new)  # (a new row never displaces an earlier group member; kept general)
        if old:
            self._apply(old)

    def _rollback(self, r0):
        """drop rows r0.. from the mirror and from every device column (an append that raised)"""
        for r in range(len(self.keys) - 1, r0 - 1, -1):
            s = self._sig(self.val[r])
            if s is not None:
                g = self.groups[s]
                g.remove(r)
                if not g:
                    del self.groups[s]
            del self.row[self.keys[r]]
            for c in self.cols:
                if r < len(c.live):
                    c.mark(r, False, False)
        del self.keys[r0:]
        del self.val[r0:]
        for c in self.cols:
            c.col.truncate(r0)
        for oc in self.ope.values():
            oc.truncate(r0)
        if self.tab is not None:
            self.tab.truncate(r0)

    def _set(self, r, contents):
        old = self.val[r]
        self.val[r] = None if contents is None else list(contents)
        self._apply(self._regroup(r, old, self.val[r]))
        if self.tab is not None:
            ids = np.asarray([r], dtype=np.uint64)
            if self.val[r] is None:
                self.tab.set_live(ids, 0)  # RemoveSet: the register holds None
            else:
                self.tab.write_rows(ids, [self.val[r]])

    # ---- write routes ----
    def put_sets(self, sets) -> list[str]:
        """POST /PutSet for each set (DDSRestServer.scala:170-188); new keys are appended in one batch."""
        keys = [key_from_set(s) for s in sets]
        fresh, seen = [], {}
        for k, s in zip(keys, sets):
            if k in self.row:
                self._set(self.row[k], s)
            elif k in seen:
                fresh[seen[k]] = (k, s)
            else:
                seen[k] = len(fresh)
                fresh.append((k, s))
        if fresh:
            self._append([k for k, _ in fresh], [s for _, s in fresh])
        return keys

    def put_set(self, contents) -> str:
        return self.put_sets([contents])[0]

    def put_empty(self, key: str) -> str:
        """POST /PutSet without a body (:190-205): the key (random in the reference) holds None."""
        if key in self.row:
            self._set(self.row[key], None)
        else:
            self._append([key], [None])
        return key

    def remove_set(self, key: str):
        """DELETE /RemoveSet/{key} (:207-218)"""
        if key in self.row and self.val[self.row[key]] is not None:
            self._set(self.row[key], None)

    def add_element(self, key: str, value):
        """PUT /AddElement/{key} (:220-255): 404 for a missing / removed set"""
        r = self.row.get(key)
        if r is None or self.val[r] is None:
            raise NotFound()
        self._set(r, self.val[r] + [value])

    def write_element(self, key: str, position: int, value):
        """PUT /WriteElement/{key}?position (:281-321): replace, or append past the end; 404 for a
        missing / removed set, 500 for a negative position (IndexOutOfBoundsException)"""
        r = self.row.get(key)
        if r is None or self.val[r] is None:
            raise NotFound()
        cur = self.val[r]
        if position > len(cur) - 1:
            self._set(r, cur + [value])
        elif position < 0:
            raise ServerError("IndexOutOfBoundsException")
        else:
            nxt = list(cur)
            nxt[position] = value
            self._set(r, nxt)

    # ---- read routes ----
    def rows(self):
        return list(self.val)

    def keyed_rows(self):
        return list(zip(self.keys, self.val))

    def _fold(self, c: _CipherColumn, modulus_text, modulus_of):
        """the resident fold of column c: 404 / 500 / one-operand reply / GPU fold of the live rows.
        modulus_of(text) parses the request's modulus (raising ServerError), only when >= 2 rows
        qualify, as the route does (:422, :515-517)."""
        if c.bad:
            raise ServerError("NumberFormatException: a qualifying element is not an integer")
        n = c.nlive
        if n == 0:
            raise NotFound()
        if n == 1:  # the first operand, unreduced (:416-417 / :510-511), no modulus parse
            r = int(np.flatnonzero(c.live)[0])
            return str(_bigint(self.val[r][c.position]))
        if modulus_text is None or modulus_of(modulus_text) != c.modulus:
            return None  # not this column's modulus: the caller takes the per-request path
        try:
            return c.col.fold_dec()
        except _EngineNotFound as e:
            raise NotFound() from e
        except DDSError as e:
            raise ServerError(str(e)) from e

    def sum_all(self, position: int, nsqr: str | None = None) -> str:
        """GET /SumAll?position&nsqr (DDSRestServer.scala:397-446)"""
        c = self.by_pos_sum.get(position)
        if c is not None and nsqr is not None:
            def parse(t):
                x = _bigint(t)
                if x is None:
                    raise ServerError("NumberFormatException: nsqr")
                return x
            got = self._fold(c, nsqr, parse)
            if got is not None:
                return got
        return routes.sum_all(self.eng, self.rows(), position, nsqr)

    def mult_all(self, position: int, pubkey: str | None = None) -> str:
        """GET /MultAll?position&pubkey (DDSRestServer.scala:491-539)"""
        c = self.by_pos_mult.get(position)
        if c is not None and pubkey is not None:
            def parse(t):
                try:
                    return rsa_modulus(t)
                except ValueError as e:
                    raise ServerError(f"InvalidKeySpecException: {e}") from e
            got = self._fold(c, pubkey, parse)
            if got is not None:
                return got
        return routes.mult_all(self.eng, self.rows(), position, pubkey=pubkey)

    def _fold_by(self, c: _CipherColumn | None, by_position: int, modulus: int) -> dict[str, str]:
        """the grouped fold of column c: the rows its resident fold takes (c.live; a qualifying element that does
        not parse answers 500 and no qualifying row 404, as _fold does) that also hold an element at by_position,
        grouped by that element's text; every value a canonical residue, also a one-row group's"""
        if c is None or modulus != c.modulus:
            raise ServerError("no resident column at this position under this modulus")
        if c.bad:
            raise ServerError("NumberFormatException: a qualifying element is not an integer")
        if c.nlive == 0:
            raise NotFound()
        rows = [int(r) for r in np.flatnonzero(c.live) if len(self.val[r]) > by_position]
        code: dict[str, int] = {}
        labels = [code.setdefault(_elem_str(self.val[r][by_position]), len(code)) for r in rows]
        if not rows:
            return {}
        try:
            vals, counts = c.col.fold_groups(labels, len(code), row_ids=rows)
        except DDSError as e:
            raise ServerError(str(e)) from e
        return {text: str(vals[g]) for text, g in code.items() if counts[g]}

    def sum_all_by(self, position: int, by_position: int, nsqr: str) -> dict[str, str]:
        """SumAll per group: {text of the element at by_position: Enc(sum of the group's m) as decimal text} over
        the rows sum_all(position, nsqr) folds that hold an element at by_position. One grouped fold on the GPU
        (dds_col_fold_groups_be); there is no plain branch, so nsqr is required."""
        x = _bigint(nsqr)
        if x is None:
            raise ServerError("NumberFormatException: nsqr")
        return self._fold_by(self.by_pos_sum.get(position), by_position, x)

    def mult_all_by(self, position: int, by_position: int, pubkey: str) -> dict[str, str]:
        """MultAll per group, as sum_all_by, under the modulus of pubkey."""
        try:
            n = rsa_modulus(pubkey)
        except ValueError as e:
            raise ServerError(f"InvalidKeySpecException: {e}") from e
        return self._fold_by(self.by_pos_mult.get(position), by_position, n)

    def _fold_by_str(self, c: _CipherColumn | None, by_position: int, modulus: int, where) -> dict[str, str]:
        """_fold_by with the labels made on the GPU from the resident string table (dds_col_fold_by_str_be): the same
        rows, groups and 500 / 404 answers, no per-row host work; `where` as _fold_by_ope's. The key texts come back
        from the table (dds_strtab_read_elems of each group's first row)."""
        if c is None or modulus != c.modulus:
            raise ServerError("no resident column at this position under this modulus")
        if self.tab is None:
            raise ServerError("no resident string table")
        if c.bad:
            raise ServerError("NumberFormatException: a qualifying element is not an integer")
        if c.nlive == 0:
            raise NotFound()
        try:
            first, vals, _, _ = c.col.fold_by_str(self.tab, by_position, self._where_mask(where))
            texts = self.tab.read_elems(first, by_position)
        except DDSError as e:
            raise ServerError(str(e)) from e
        return {t.decode(): str(v) for t, v in zip(texts, vals)}

    def sum_all_by_str(self, position: int, by_position: int, nsqr: str, where=None) -> dict[str, str]:
        """sum_all_by with the grouping done on the GPU from the resident string table: the same result, groups in
        order of first occurrence; where: (route, position, value) as sum_all_by_ope's. Raises ServerError when no
        string table is resident."""
        x = _bigint(nsqr)
        if x is None:
            raise ServerError("NumberFormatException: nsqr")
        return self._fold_by_str(self.by_pos_sum.get(position), by_position, x, where)

    def mult_all_by_str(self, position: int, by_position: int, pubkey: str, where=None) -> dict[str, str]:
        """MultAll per group, as sum_all_by_str, under the modulus of pubkey."""
        try:
            n = rsa_modulus(pubkey)
        except ValueError as e:
            raise ServerError(f"InvalidKeySpecException: {e}") from e
        return self._fold_by_str(self.by_pos_mult.get(position), by_position, n, where)

    def _fold_by_ope(self, c: _CipherColumn | None, by_position: int, modulus: int, where,
                     descending: bool | None = None) -> dict[int, str]:
        """the grouped fold of column c keyed by the resident OPE column at by_position: the rows its resident
        fold takes (500 / 404 as _fold_by) that hold an element at by_position and pass `where`, grouped by that
        element's VALUE on the GPU (dds_col_fold_by_ope_be): no per-row host work, the mask is the only per-row
        upload. descending (not None): the cumulative values instead (dds_col_scan_by_ope_be): over the keys up to
        each key (False), or from each key on (True)"""
        oc = self._by_ope_column(c, by_position, modulus)
        try:
            mask = self._where_mask(where)
            if descending is None:
                keys, vals, _ = c.col.fold_by_ope(oc, mask)
            else:
                keys, vals, _ = c.col.scan_by_ope(oc, mask, suffix=descending)
        except DDSError as e:
            raise ServerError(str(e)) from e
        return {int(k): str(v) for k, v in zip(keys, vals)}

    def _by_ope_column(self, c: _CipherColumn | None, by_position: int, modulus: int):
        """the resident OPE column a keyed call over column c groups by; 500 / 404 as _fold_by"""
        if c is None or modulus != c.modulus:
            raise ServerError("no resident column at this position under this modulus")
        oc = self.ope.get(by_position)
        if oc is None:
            raise ServerError("no resident OPE column at the grouping position")
        if c.bad:
            raise ServerError("NumberFormatException: a qualifying element is not an integer")
        if c.nlive == 0:
            raise NotFound()
        return oc

    def _where_mask(self, where):
        """the row mask of a keyed call's `where` (route, position, value), or None; DDSError from the search"""
        if where is None:
            return None
        route, position, value = where
        wc = self.ope.get(position)
        if wc is None:
            raise ServerError("no resident OPE column at the WHERE position")
        mask, _ = wc.search_mask(_dec_text(value), routes._ROUTE_OP[route])
        return mask

    def _scan_part_by_ope(self, c: _CipherColumn | None, by_position: int, modulus: int, where,
                          descending: bool) -> dict[int, list]:
        """the running totals of column c inside each key of the resident OPE column at by_position
        (dds_col_scan_part_by_ope_be): the rows _fold_by_ope takes, with its errors; {key: [(stored-set key,
        decimal text), ...]} in row order"""
        oc = self._by_ope_column(c, by_position, modulus)
        try:
            rows, vals, keys, counts = c.col.scan_part_by_ope(oc, self._where_mask(where), suffix=descending)
        except DDSError as e:
            raise ServerError(str(e)) from e
        out, at = {}, 0
        for k, cnt in zip(keys, counts):
            out[int(k)] = [(self.keys[int(rows[t])], str(vals[t])) for t in range(at, at + int(cnt))]
            at += int(cnt)
        return out

    def running_sum_partition_by_ope(self, position: int, by_position: int, nsqr: str, where=None,
                                     descending: bool = False) -> dict[int, list]:
        """SELECT row, SUM(x) OVER (PARTITION BY key ORDER BY row) [WHERE ...]: {value of the OPE element at
        by_position: [(stored-set key, Enc(sum of m over the partition's rows up to this one) as decimal text),
        ...] in row order}, over the rows sum_all_by_ope groups and with its `where`. descending: the rows from
        this one on. One labelling and one segmented scan on the GPU."""
        x = _bigint(nsqr)
        if x is None:
            raise ServerError("NumberFormatException: nsqr")
        return self._scan_part_by_ope(self.by_pos_sum.get(position), by_position, x, where, bool(descending))

    def running_mult_partition_by_ope(self, position: int, by_position: int, pubkey: str, where=None,
                                      descending: bool = False) -> dict[int, list]:
        """The running MultAll inside each key, as running_sum_partition_by_ope, under the modulus of pubkey."""
        try:
            n = rsa_modulus(pubkey)
        except ValueError as e:
            raise ServerError(f"InvalidKeySpecException: {e}") from e
        return self._scan_part_by_ope(self.by_pos_mult.get(position), by_position, n, where, bool(descending))

    def sum_all_by_ope(self, position: int, by_position: int, nsqr: str, where=None) -> dict[int, str]:
        """SELECT key, SUM(x) [WHERE ...] GROUP BY key: {value of the OPE element at by_position: Enc(sum of the
        group's m) as decimal text} over the rows sum_all(position, nsqr) folds that hold an element at
        by_position. where: (route, position, value) of a Search{Gt,GtEq,Lt,LtEq} on a resident OPE column,
        whose row mask goes straight into the fold. Unlike sum_all_by, which groups by element text, "07" and "7"
        are one group here. Raises ServerError when no OPE column is resident at by_position."""
        x = _bigint(nsqr)
        if x is None:
            raise ServerError("NumberFormatException: nsqr")
        return self._fold_by_ope(self.by_pos_sum.get(position), by_position, x, where)

    def mult_all_by_ope(self, position: int, by_position: int, pubkey: str, where=None) -> dict[int, str]:
        """MultAll per key, as sum_all_by_ope, under the modulus of pubkey."""
        try:
            n = rsa_modulus(pubkey)
        except ValueError as e:
            raise ServerError(f"InvalidKeySpecException: {e}") from e
        return self._fold_by_ope(self.by_pos_mult.get(position), by_position, n, where)

    def running_sum_by_ope(self, position: int, by_position: int, nsqr: str, where=None,
                           descending: bool = False) -> dict[int, str]:
        """SELECT key, SUM(x) OVER (ORDER BY key) [WHERE ...]: {value of the OPE element at by_position:
        Enc(sum of m over the rows whose key is <= it) as decimal text}, over the rows sum_all_by_ope groups and
        with its `where`. descending: the rows whose key is >= it (ORDER BY key DESC). One labelling, one
        segmented fold and one scan of the key totals on the GPU (dds_col_scan_by_ope_be)."""
        x = _bigint(nsqr)
        if x is None:
            raise ServerError("NumberFormatException: nsqr")
        return self._fold_by_ope(self.by_pos_sum.get(position), by_position, x, where, descending=bool(descending))

    def running_mult_by_ope(self, position: int, by_position: int, pubkey: str, where=None,
                            descending: bool = False) -> dict[int, str]:
        """The running MultAll by key, as running_sum_by_ope, under the modulus of pubkey."""
        try:
            n = rsa_modulus(pubkey)
        except ValueError as e:
            raise ServerError(f"InvalidKeySpecException: {e}") from e
        return self._fold_by_ope(self.by_pos_mult.get(position), by_position, n, where, descending=bool(descending))

    def search(self, route: str, position: int, value) -> list[str]:
        """POST /Search{Gt,GtEq,Lt,LtEq}?position (:682-830): matching keys in row order (the
        reference's order is unspecified). The match set comes back as a row bitmask."""
        oc = self.ope.get(position)
        if oc is None:
            return routes.search(self.eng, route, self.keyed_rows(), position, value)
        try:
            words, _ = oc.search_mask(_dec_text(value), routes._ROUTE_OP[route])
        except DDSError as e:
            raise ServerError(str(e)) from e
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")[: len(self.keys)]
        return [self.keys[i] for i in np.flatnonzero(bits)]

    def order(self, route: str, position: int) -> list[str]:
        """GET /OrderLS|/OrderSL?position (:541-606)"""
        if route not in ("OrderLS", "OrderSL"):
            raise ValueError(route)
        oc = self.ope.get(position)
        if oc is None:
            return routes.order(self.eng, route, self.keyed_rows(), position)
        try:
            idx = oc.order(route == "OrderLS")
        except DDSError as e:
            raise ServerError(str(e)) from e
        return [self.keys[i] for i in idx]

    def search_eq(self, route: str, position: int, value) -> list[str]:
        """POST /SearchEq|/SearchNEq?position (:607-681): keys in row order (the reference's order is
        unspecified)"""
        if route not in ("SearchEq", "SearchNEq"):
            raise ValueError(route)
        if self.tab is None:
            return routes.search_eq(self.eng, route, self.keyed_rows(), position, value)
        try:
            idx = self.tab.search_eq(position, value, route == "SearchNEq")
        except DDSError as e:
            raise ServerError(str(e)) from e
        return [self.keys[i] for i in idx]

    def search_entry(self, route: str, values) -> list[str]:
        """POST /SearchEntry (one value, compared as ``DDSItem(value)``, :845) | /SearchEntryOR |
        /SearchEntryAND (three, :831-938)"""
        if route not in ("SearchEntry", "SearchEntryOR", "SearchEntryAND"):
            raise ValueError(route)
        if self.tab is None:
            return routes.search_entry(self.eng, route, self.keyed_rows(), values)
        needles = [entry_needle(values[0])] if route == "SearchEntry" else list(values)
        try:
            idx = self.tab.search_entry(needles, route == "SearchEntryAND")
        except DDSError as e:
            raise ServerError(str(e)) from e
        return [self.keys[i] for i in idx]

    def is_element(self, key: str, value) -> bool:
        """POST /IsElement/{key} (:322-353): 404 for an unknown key or a removed set"""
        r = self.row.get(key)
        if r is None or self.val[r] is None:
            raise NotFound()
        if self.tab is None:
            return routes.is_element(self.eng, self.val[r], value)
        try:
            return self.tab.is_element(r, value)
        except _EngineNotFound as e:
            raise NotFound() from e
        except DDSError as e:
            raise ServerError(str(e)) from e
