"""Engine: one fsm_ctx (HIP stream + device buffers) and its flattened DBs."""
import ctypes
import weakref

import numpy as np

from . import _lib
from ._lib import MODE_SPADE, MODE_TSR, KEEP_CLOSED, KEEP_MAXIMAL, check

_KEEP = {"closed": KEEP_CLOSED, "maximal": KEEP_MAXIMAL}


class _ResultOwner:
    """Keeps a libfsm result struct alive while numpy views of its arrays exist:
    every view's buffer holds a reference to this object, whose finalizer calls
    the library's free function once the last view is gone."""

    def __init__(self, free_fn, ptr):
        weakref.finalize(self, free_fn, ptr)

    def view(self, ptr, n, dtype):
        dt = np.dtype(dtype)
        if n <= 0 or not ptr:
            return np.zeros(0, dtype=dt)
        buf = (np.ctypeslib.as_ctypes_type(dt) * int(n)).from_address(ctypes.addressof(ptr.contents))
        buf._owner = self
        arr = np.frombuffer(buf, dtype=dt)
        arr.flags.writeable = False  # library memory: read-only views
        return arr


class Engine:
    """Owns a libfsm context on one gfx950 device."""

    def __init__(self, device=0, verbose=False, mem_budget=0, nranks=1, rank=0, unique_id=None, host_comm=None,
                 devices=None):
        """nranks > 1: sharded SPADE, one Engine per rank, collectives over RCCL
        (unique_id from dist.comm_unique_id() on rank 0) or over host_comm
        (a dist.TorchHostComm; kept alive by this Engine).
        devices=[d0, d1, ...] (more than one): ONE Engine whose calls shard over
        in-process ranks, rank r on HIP device d_r (a device may repeat), the way the
        JVM drop-in shards (fsm_opts.ndevices); every call returns the whole result."""
        L = _lib.load()
        opts = _lib.Opts()
        opts.device = device
        if devices is not None and len(devices) > 1:
            if len(devices) > _lib.MAX_DEVICES:
                raise ValueError("at most %d in-process ranks" % _lib.MAX_DEVICES)
            opts.ndevices = len(devices)
            for r, d in enumerate(devices):
                opts.devices[r] = int(d)
        elif devices is not None and len(devices) == 1:
            opts.device = int(devices[0])
        opts.nranks = int(nranks)
        opts.rank = int(rank)
        opts.verbose = 1 if verbose else 0
        opts.mem_budget = int(mem_budget)
        if unique_id is not None:
            ctypes.memmove(opts.unique_id, bytes(unique_id), 128)
        self._host_comm = host_comm
        if host_comm is not None:
            opts.host_comm = ctypes.pointer(host_comm.struct)
        self._ctx = ctypes.c_void_p()
        check(L.fsm_ctx_create(ctypes.byref(opts), ctypes.byref(self._ctx)), None)
        self._L = L

    def close(self):
        if getattr(self, "_ctx", None):
            self._L.fsm_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ------------------------------------------------------------ DBs
    def db_from_spmf(self, records, mode):
        """records: sequence of (sid, spmf_line) — the RDD[(Int,String)]."""
        n = len(records)
        sids = (ctypes.c_int32 * max(n, 1))(*[int(s) for s, _ in records])
        enc = [l.encode("utf-8") if isinstance(l, str) else bytes(l) for _, l in records]
        lines = (ctypes.c_char_p * max(n, 1))(*enc)
        lens = (ctypes.c_int64 * max(n, 1))(*[len(b) for b in enc])
        db = ctypes.c_void_p()
        check(self._L.fsm_db_from_spmf(self._ctx, mode, sids, lines, lens, n, ctypes.byref(db)), self._ctx)
        return DB(self, db, mode)

    def db_from_tokens(self, sids, seq_off, tokens, mode):
        sids = np.ascontiguousarray(sids, dtype=np.int32)
        seq_off = np.ascontiguousarray(seq_off, dtype=np.int64)
        tokens = np.ascontiguousarray(tokens, dtype=np.int64)
        n = len(sids)
        db = ctypes.c_void_p()
        P = ctypes.POINTER
        check(self._L.fsm_db_from_tokens(
            self._ctx, mode, sids.ctypes.data_as(P(ctypes.c_int32)), seq_off.ctypes.data_as(P(ctypes.c_int64)),
            tokens.ctypes.data_as(P(ctypes.c_int64)), n, ctypes.byref(db)), self._ctx)
        return DB(self, db, mode)

    def db_export(self, db):
        """fsm_db_export: the flattened DB as it sits in HBM, as numpy arrays."""
        out = ctypes.POINTER(_lib.DbImage)()
        check(self._L.fsm_db_export(self._ctx, db.handle, ctypes.byref(out)), self._ctx)
        try:
            m = out.contents

            def arr(ptr, n):
                # an empty field keeps its ctypes element type (uint32 / uint64 / int32)
                dt = np.dtype(ptr._type_)
                return np.ctypeslib.as_array(ptr, shape=(max(n, 1),))[:n].copy() if n else np.zeros(0, dtype=dt)

            img = {"mode": m.mode, "mask_words": m.mask_words, "rows": m.rows, "entries": m.entries,
                   "items": m.items, "max_occ": m.max_occ, "row_off": arr(m.row_off, m.rows + 1),
                   "item": arr(m.item, m.entries), "item_val": arr(m.item_val, m.items)}
            if m.mode == MODE_SPADE:
                img["mask"] = arr(m.mask, m.entries * m.mask_words)
            else:
                img["first"] = arr(m.first, m.entries)
                img["last"] = arr(m.last, m.entries)
        finally:
            self._L.fsm_db_image_free(out)
        return img

    # ------------------------------------------------------------ mining
    def _views(self, out, copy=False):
        """A library-owned fsm_patterns -> the four CSR arrays (views sharing one owner, or copies)."""
        owner = _ResultOwner(self._L.fsm_patterns_free, out)
        p = out.contents
        csr = (owner.view(p.support, p.n, np.int32), owner.view(p.pat_off, p.n + 1, np.int64),
               owner.view(p.set_off, p.n_sets + 1, np.int64), owner.view(p.items, p.n_items, np.int32))
        return tuple(a.copy() for a in csr) if copy else csr

    def _filter(self, pats, keep, copy=False):
        """fsm_patterns_filter on a _lib.Patterns (by reference) -> (csr, kept_idx)."""
        code = _KEEP.get(keep)
        if code is None:
            raise ValueError("keep must be 'closed' or 'maximal' (got %r)" % (keep,))
        out = ctypes.POINTER(_lib.Patterns)()
        idx = np.empty(max(int(pats.n), 1), np.int64)
        check(self._L.fsm_patterns_filter(self._ctx, ctypes.byref(pats), code, ctypes.byref(out),
                                          idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))), self._ctx)
        kept = idx[:out.contents.n].copy()
        return self._views(out, copy), kept

    def filter_patterns(self, csr, keep, copy=False):
        """fsm_patterns_filter: the closed ("closed") or maximal ("maximal") patterns of a
        COMPLETE frequent set, computed on the GPU.

        csr is the (support, pat_off, set_off, items) tuple of spade_csr, or any numpy
        arrays of that form.  Returns ((support, pat_off, set_off, items), kept_idx): the
        kept patterns in input order, with spade_csr's view and ownership rules, and
        their indexes in the input (int64, ascending)."""
        sup, po, so, it = csr
        sup = np.ascontiguousarray(sup, np.int32)
        po = np.ascontiguousarray(po, np.int64)
        so = np.ascontiguousarray(so, np.int64)
        it = np.ascontiguousarray(it, np.int32)
        if len(po) != len(sup) + 1 or len(so) < 1:
            raise ValueError("pat_off must have n + 1 entries and set_off at least one")
        P = ctypes.POINTER
        pats = _lib.Patterns(len(sup), sup.ctypes.data_as(P(ctypes.c_int32)), po.ctypes.data_as(P(ctypes.c_int64)),
                             so.ctypes.data_as(P(ctypes.c_int64)), it.ctypes.data_as(P(ctypes.c_int32)),
                             len(so) - 1, len(it), 0, 0)
        return self._filter(pats, keep, copy)

    @staticmethod
    def _patterns_arg(patterns):
        """The accepted forms of a GIVEN pattern set -> (_lib.Patterns, n, keep): a CSR tuple
        (support_or_None, pat_off, set_off, items) like spade_csr's (the supports are
        ignored), a list of itemset tuples such as ((1,), (3, 4)), or a list of (itemsets,
        support) pairs as Engine.spade returns them.  keep holds the arrays the struct
        points into."""
        flat = (np.ndarray, list)
        if (isinstance(patterns, tuple) and len(patterns) == 4 and (patterns[0] is None or isinstance(patterns[0], flat))
                and isinstance(patterns[1], flat) and (len(patterns[1]) == 0 or not hasattr(patterns[1][0], "__len__"))):
            _sup, po, so, it = patterns
        else:
            po, so, it = [0], [0], []
            for pat in patterns:
                # (itemsets, support) pairs carry an int second; an itemset tuple holds tuples only
                sets = pat[0] if len(pat) == 2 and not hasattr(pat[1], "__len__") else pat
                for X in sets:
                    it.extend(X)
                    so.append(len(it))
                po.append(len(so) - 1)
        po = np.ascontiguousarray(po, np.int64)
        so = np.ascontiguousarray(so, np.int64)
        it = np.ascontiguousarray(it, np.int32)
        if len(po) < 1 or len(so) < 1:
            raise ValueError("pat_off and set_off must have at least one entry")
        n = len(po) - 1
        P = ctypes.POINTER
        pats = _lib.Patterns(n, None, po.ctypes.data_as(P(ctypes.c_int64)), so.ctypes.data_as(P(ctypes.c_int64)),
                             it.ctypes.data_as(P(ctypes.c_int32)), len(so) - 1, len(it), 0, 0)
        return pats, n, (po, so, it)

    def pattern_supports(self, db, patterns):
        """fsm_patterns_support: the supports of GIVEN patterns in a resident SPADE DB,
        counted on the GPU by definition -> np.ndarray[int32], one count per pattern.

        patterns is a CSR tuple (support_or_None, pat_off, set_off, items) like spade_csr's
        (the supports are ignored), or a list of itemset tuples such as ((1,), (3, 4)), or
        a list of (itemsets, support) pairs as Engine.spade returns them.  Items are item
        values; a pattern that cannot match (an unknown item, more itemsets than the DB
        has eids) counts 0.  The first call on a DB builds its item -> rows index."""
        pats, n, keep = self._patterns_arg(patterns)
        out = np.zeros(n, np.int32)
        buf = out if n else np.zeros(1, np.int32)
        check(self._L.fsm_patterns_support(self._ctx, db.handle, ctypes.byref(pats),
                                           buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))), self._ctx)
        del keep
        return out

    def pattern_sids(self, db, patterns, max_sids=0, copy=False):
        """fsm_patterns_sids: the sequence ids of the rows that hold GIVEN patterns in a
        resident SPADE DB -> (off int64[n + 1], sid int32[n_sids]); pattern p's ids are
        sid[off[p]:off[p + 1]], strictly ascending, as the DB's records named them, so
        np.diff(off) are the supports.

        patterns takes the forms of pattern_supports; a pattern that cannot match gets an
        empty list.  max_sids > 0 caps the ids over all patterns: a larger result raises
        FsmError (FSM_ELIMIT, the total needed in its message) before anything is
        allocated for it.  The arrays are read-only views of the library's result with
        spade_csr's ownership rules; copy=True returns independent, writable copies.  The
        first call on a DB orders its item -> rows index."""
        pats, _n, keep = self._patterns_arg(patterns)
        out = ctypes.POINTER(_lib.SidLists)()
        check(self._L.fsm_patterns_sids(self._ctx, db.handle, ctypes.byref(pats), int(max_sids), ctypes.byref(out)),
              self._ctx)
        del keep
        owner = _ResultOwner(self._L.fsm_sidlists_free, out)
        r = out.contents
        res = (owner.view(r.off, r.n + 1, np.int64), owner.view(r.sid, r.n_sids, np.int32))
        return tuple(a.copy() for a in res) if copy else res

    def spade_csr(self, db, support, dfs=True, copy=False, keep="all"):
        """fsm_spade_mine -> CSR numpy arrays (support, pat_off, set_off, items), meta.

        keep="closed" / "maximal": the mined set goes through fsm_patterns_filter and
        only the closed / maximal patterns are returned (meta["n"] counts them,
        meta["n_mined"] the complete set).

        By default the arrays are read-only views of the library's result
        buffers (no copy of the hundreds of MB a dense mine returns).  The four
        views share ONE lifetime: fsm_patterns_free runs when the last of them
        is garbage-collected, so keeping any one of them (say only `support`)
        keeps every result buffer of the mine alive.  copy=True returns
        independent, writable copies and frees the library's buffers at once."""
        if keep != "all" and keep not in _KEEP:
            raise ValueError("keep must be 'all', 'closed' or 'maximal' (got %r)" % (keep,))
        out = ctypes.POINTER(_lib.Patterns)()
        check(self._L.fsm_spade_mine(self._ctx, db.handle, float(support), 1 if dfs else 0,
                                     ctypes.byref(out)), self._ctx)
        p = out.contents
        meta = {"total": p.total, "minsup": p.minsup, "n": p.n}
        if keep != "all":
            try:
                csr, _kept = self._filter(p, keep, copy)
            finally:
                self._L.fsm_patterns_free(out)  # the complete set is not returned
            meta["n_mined"] = meta["n"]
            meta["n"] = len(csr[0])
            return csr, meta
        return self._views(out, copy), meta

    def spade(self, db, support, dfs=True, keep="all"):
        """-> (patterns: list[(itemsets tuple-of-tuples, support)], meta dict)."""
        (sup, po, so, it), meta = self.spade_csr(db, support, dfs, keep=keep)
        n = meta["n"]
        itl = it.tolist()
        sol = so.tolist()
        pats = []
        for i in range(n):
            sets = tuple(tuple(itl[sol[s]:sol[s + 1]]) for s in range(po[i], po[i + 1]))
            pats.append((sets, int(sup[i])))
        return pats, meta

    def tsr(self, db, k, minconf):
        """-> (rules: list[(antecedent, consequent, support, confidence)], meta)."""
        out = ctypes.POINTER(_lib.Rules)()
        check(self._L.fsm_tsr_mine(self._ctx, db.handle, int(k), float(minconf), ctypes.byref(out)), self._ctx)
        try:
            r = out.contents
            rules = []
            for i in range(r.n):
                x = tuple(r.ante[q] for q in range(r.ante_off[i], r.ante_off[i + 1]))
                y = tuple(r.cons[q] for q in range(r.cons_off[i], r.cons_off[i + 1]))
                rules.append((x, y, r.support[i], r.confidence[i]))
            meta = {"total": r.total, "final_minsup": r.final_minsup}
        finally:
            self._L.fsm_rules_free(out)
        return rules, meta

    def tsr_mined(self, db, k, minconf):
        """fsm_tsr_mine -> MinedRules: the library's rule set kept as mined (no copy), for
        the rule queries and documents that run on it through the C ABI."""
        out = ctypes.POINTER(_lib.Rules)()
        check(self._L.fsm_tsr_mine(self._ctx, db.handle, int(k), float(minconf), ctypes.byref(out)), self._ctx)
        return MinedRules(self._L, out)

    def rule_supports(self, db, rules):
        """fsm_rules_support: what GIVEN rules score in a resident TSR DB, counted on the GPU
        by definition -> (support int32[n], ante int32[n], confidence float64[n]); ante is the
        number of sequences holding the whole antecedent, confidence support / ante (0.0 when
        ante is 0).

        rules is a list of (X, Y) tuples, a list of (X, Y, support, confidence) tuples as
        Engine.tsr returns them, a MinedRules, or a 4-tuple (ante_off, ante, cons_off, cons)
        of arrays (see rules_csr).  Items are item values, ascending inside a side, no item on
        both sides; an item the DB does not hold scores 0, and a side may be of any length."""
        P = ctypes.POINTER
        if isinstance(rules, MinedRules):
            keep, n, ref = rules, rules.n, rules._p  # the library's own struct, borrowed
        else:
            xo, xs, yo, ys = keep = rules_csr(rules)
            n = len(xo) - 1
            ref = ctypes.byref(_lib.Rules(n, None, None, xo.ctypes.data_as(P(ctypes.c_int64)),
                                          xs.ctypes.data_as(P(ctypes.c_int32)), yo.ctypes.data_as(P(ctypes.c_int64)),
                                          ys.ctypes.data_as(P(ctypes.c_int32)), 0, 0))
        sup, ante, conf = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.float64)
        check(self._L.fsm_rules_support(self._ctx, db.handle, ref, sup.ctypes.data_as(P(ctypes.c_int32)),
                                        ante.ctypes.data_as(P(ctypes.c_int32)),
                                        conf.ctypes.data_as(P(ctypes.c_double))), self._ctx)
        del keep
        return sup[:n], ante[:n], conf[:n]

    def rule_predictions(self, db, rules, topn, copy=False):
        """fsm_rules_predict: per row of a resident TSR DB, the items GIVEN scored rules say
        should come next -> (off int64[n + 1], item int32[n_preds], rule int32[n_preds]); row
        s's entries are item[off[s]:off[s + 1]] (item values) with rule[...] the index of the
        entry's best rule.

        A rule X => Y fires in a row that holds all of X; an item of Y is open there if the
        row does not hold it or holds it last no later than the itemset that completes X.  An
        item's best rule is the first, by (confidence descending, support descending, index
        ascending), under which it is open; a row lists its items by their best rule's rank,
        then by value, topn at most.

        rules is a MinedRules, a list of (X, Y, support, confidence) tuples as Engine.tsr
        returns them, or a 6-tuple (ante_off, ante, cons_off, cons, support, confidence) of
        arrays (see scored_rules_csr); a form without scores raises ValueError.  The arrays
        are read-only views of the library's result with pattern_sids' ownership rules;
        copy=True returns independent, writable copies."""
        P = ctypes.POINTER
        if isinstance(rules, MinedRules):
            keep, ref = rules, rules._p  # the library's own struct, borrowed
        else:
            xo, xs, yo, ys, sup, conf = keep = scored_rules_csr(rules)
            ref = ctypes.byref(_lib.Rules(len(xo) - 1, sup.ctypes.data_as(P(ctypes.c_int32)),
                                          conf.ctypes.data_as(P(ctypes.c_double)), xo.ctypes.data_as(P(ctypes.c_int64)),
                                          xs.ctypes.data_as(P(ctypes.c_int32)), yo.ctypes.data_as(P(ctypes.c_int64)),
                                          ys.ctypes.data_as(P(ctypes.c_int32)), 0, 0))
        out = P(_lib.Predictions)()
        check(self._L.fsm_rules_predict(self._ctx, db.handle, ref, int(topn), ctypes.byref(out)), self._ctx)
        del keep
        owner = _ResultOwner(self._L.fsm_predictions_free, out)
        r = out.contents
        res = (owner.view(r.off, r.n + 1, np.int64), owner.view(r.item, r.n_preds, np.int32),
               owner.view(r.rule, r.n_preds, np.int32))
        return tuple(a.copy() for a in res) if copy else res

    def kernel_stats(self):
        """[{name, launches, alg_bytes, survey_bytes, ms}] of the last mine or filter call (device time, HIP
        events; alg_bytes: the kernel's own layout, survey_bytes: SURVEY §8(d) units)."""
        n = ctypes.c_int32()
        check(self._L.fsm_get_kernel_stats(self._ctx, None, 0, ctypes.byref(n)), self._ctx)
        arr = (_lib.KernelStat * max(n.value, 1))()
        check(self._L.fsm_get_kernel_stats(self._ctx, arr, n.value, ctypes.byref(n)), self._ctx)
        return [{"name": k.name.decode(), "launches": k.launches, "alg_bytes": k.alg_bytes,
                 "survey_bytes": k.survey_bytes, "ms": k.ms} for k in arr[:n.value]]

    def stats(self):
        st = _lib.Stats()
        check(self._L.fsm_get_stats(self._ctx, ctypes.byref(st)), self._ctx)
        return st.as_dict()


class MinedRules:
    """A mined fsm_rules (library-owned, freed with the object): its rules, and the
    rule queries (fsm_rules_query, FSMQuestor.scala:46-98) and json4s document
    (fsm_rules_json) computed on it by the library."""

    def __init__(self, L, ptr):
        self._L, self._p = L, ptr
        weakref.finalize(self, L.fsm_rules_free, ptr)
        r = ptr.contents
        self.total, self.final_minsup, self.n = r.total, r.final_minsup, r.n

    def rules(self):
        """[(antecedent, consequent, support, confidence)] in the library's order."""
        r = self._p.contents
        out = []
        for i in range(r.n):
            x = tuple(r.ante[q] for q in range(r.ante_off[i], r.ante_off[i + 1]))
            y = tuple(r.cons[q] for q in range(r.cons_off[i], r.cons_off[i + 1]))
            out.append((x, y, r.support[i], r.confidence[i]))
        return out

    def query(self, side, items):
        """Indexes (ascending) of the rules whose antecedent (side 0) / consequent (side 1)
        items all occur in `items`."""
        q = np.ascontiguousarray(list(items), np.int32)
        idx = np.zeros(max(self.n, 1), np.int64)
        n = ctypes.c_int64()
        check(self._L.fsm_rules_query(self._p, int(side), q.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(q),
                                      idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), ctypes.byref(n)))
        return idx[:n.value].tolist()

    def to_json(self):
        out, n = ctypes.c_void_p(), ctypes.c_int64()
        check(self._L.fsm_rules_json(self._p, ctypes.byref(out), ctypes.byref(n)))
        try:
            return ctypes.string_at(out, n.value).decode("utf-8")
        finally:
            self._L.fsm_buffer_free(out)


def rules_csr(rules):
    """The accepted forms of a rule set -> (ante_off int64[n+1], ante int32, cons_off
    int64[n+1], cons int32), the four arrays fsm_rules_support reads.  rules is a 4-tuple of
    such arrays (or lists), a MinedRules, or a list of (X, Y) or (X, Y, support, confidence)
    tuples (anything after Y is ignored)."""
    flat = (np.ndarray, list)
    if isinstance(rules, MinedRules):
        rules = [r[:2] for r in rules.rules()]
    if (isinstance(rules, tuple) and len(rules) == 4 and all(isinstance(a, flat) for a in rules)
            and (len(rules[0]) == 0 or not hasattr(rules[0][0], "__len__"))):
        xo, xs, yo, ys = rules
    else:
        xo, xs, yo, ys = [0], [], [0], []
        for r in rules:
            xs.extend(r[0])
            ys.extend(r[1])
            xo.append(len(xs))
            yo.append(len(ys))
    xo = np.ascontiguousarray(xo, np.int64)
    yo = np.ascontiguousarray(yo, np.int64)
    xs = np.ascontiguousarray(xs, np.int32)
    ys = np.ascontiguousarray(ys, np.int32)
    if len(xo) < 1 or len(xo) != len(yo):
        raise ValueError("ante_off and cons_off must have the same n + 1 >= 1 entries")
    return xo, xs, yo, ys


def scored_rules_csr(rules):
    """The accepted forms of a SCORED rule set -> (ante_off int64[n+1], ante int32, cons_off
    int64[n+1], cons int32, support int32[n], confidence float64[n]), the six arrays
    fsm_rules_predict reads.  rules is a 6-tuple of such arrays (or lists), a MinedRules, or a
    list of (X, Y, support, confidence) tuples.  A form without scores ((X, Y) pairs, the
    4-tuple of rules_csr) raises ValueError."""
    flat = (np.ndarray, list)
    if isinstance(rules, MinedRules):
        rules = rules.rules()
    if (isinstance(rules, tuple) and len(rules) in (4, 6) and all(isinstance(a, flat) for a in rules)
            and (len(rules[0]) == 0 or not hasattr(rules[0][0], "__len__"))):
        if len(rules) == 4:
            raise ValueError("rule predictions need scored rules: (ante_off, ante, cons_off, cons, support, confidence)")
        xo, xs, yo, ys = rules_csr(tuple(rules[:4]))
        sup, conf = rules[4], rules[5]
    else:
        rules = list(rules)
        if any(len(r) < 4 for r in rules):
            raise ValueError("rule predictions need scored rules: (X, Y, support, confidence) tuples")
        xo, xs, yo, ys = rules_csr(rules)
        sup, conf = [r[2] for r in rules], [r[3] for r in rules]
    sup = np.ascontiguousarray(sup, np.int32)
    conf = np.ascontiguousarray(conf, np.float64)
    if len(sup) != len(xo) - 1 or len(conf) != len(xo) - 1:
        raise ValueError("support and confidence must have one entry per rule")
    return xo, xs, yo, ys, sup, conf


class DB:
    def __init__(self, engine, handle, mode):
        self.engine = engine
        self.handle = handle
        self.mode = mode

    def free(self):
        if self.handle:
            self.engine._L.fsm_db_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


_default = None


def default_engine():
    global _default
    if _default is None:
        _default = Engine(0)
    return _default
