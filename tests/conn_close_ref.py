"""TEST INFRASTRUCTURE: rsk_conn_close_batch (include/rsk_codec.h) restated in numpy, the checkers and the
scenarios the CPU and GPU tests share (the device is a parameter: "cpu" drives the host twin, a cuda device the
batch call of a Codec).

  close_ref     the contract: a marked LIVE row loses ALIVE (INetConn::NotifyErr, conn/INetConn.cpp:49-52); with
                REMOVE it leaves the table, with SWEEP every LIVE row without ALIVE does (INetGroup::RemoveConn from
                IGroup::Flush, conn/INetGroup.cpp:94-101, conn/IGroup.cpp:81-111); the two lists in row order.
  Harness       a table on the device under test with its numpy image; every close is followed by the checkers:
                state and the lists against close_ref, every other column bytewise, the lookups against
                conn_ref on the new state (index as left, then rebuilt), the picks against pick_ref.rule_ref
                (which reads no index) and against a freshly built pick index, and nothing written where nothing
                changed.
Every comparison is exact."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from rsock_amd import _abi as A
from tests import conn_ref as CR
from tests import control_golden as G
from tests import control_ref as C
from tests import pick_ref as P
from tests.collide import group_home

NONE = A.CONN_NONE
NO_RST = 0xFFFFFFFF
LIVE, ALIVE, NEW, UP = A.CONN_LIVE, A.CONN_ALIVE, A.CONN_NEW, CR.UP
SENT = 0x6E
SENT32 = 0x6E6E6E6E
# the row-tile edges of the count pass and of the 1024-entry pick tiles
CAPACITIES = (1, 2, 257, 1023, 1024, 1025, 4097, 65536)
GROUP_SIZES = (1, 2, 63, 64, 65, 1024, 1025)
PATTERNS = ("nothing", "one_row", "lowest_candidate", "whole_group", "every_row", "every_second_row")
WALK_CASES = G.names("walk")
TIMER_CASES = G.names("timer")
SEND_CASES = G.names("send")


# ---- the restatement ---------------------------------------------------------------------------------------
def list_marks(capacity, close_rows, n_close, m_max):
    """The rows a list marks: the first min(n_close, m_max) entries that are rows of the table."""
    mask = np.zeros(capacity, bool)
    rows = np.asarray(close_rows, np.uint64)[: min(int(n_close), int(m_max))]
    mask[rows[rows < capacity].astype(np.int64)] = True
    return mask


def close_ref(state, mask, remove=False, sweep=False):
    """-> dict(state, marked_rows, closed_rows) of a close whose marks are the rows of `mask`."""
    st = np.asarray(state, np.uint8).copy()
    live = (st & LIVE) != 0
    hit = live & mask
    marked = hit & ((st & ALIVE) != 0)
    st[hit] &= np.uint8(~ALIVE & 0xFF)
    gone = np.zeros(len(st), bool)
    if remove:
        gone |= hit
    if sweep:
        gone |= live & ((st & ALIVE) == 0)
    st[gone] &= np.uint8(~(LIVE | ALIVE | NEW) & 0xFF)
    return {"state": st, "marked_rows": np.nonzero(marked)[0].astype(np.uint32),
            "closed_rows": np.nonzero(gone)[0].astype(np.uint32)}


# ---- the harness -------------------------------------------------------------------------------------------
def host(t, dt):
    return t.cpu().numpy().view(dt)


def filled(n, dtype, device):
    t = torch.empty(n, dtype=dtype, device=device)
    t.view(torch.uint8).fill_(SENT)
    return t


class Harness:
    """A ConnTable on `device` ("cpu": the host twins) with both indexes built, and its numpy image."""

    def __init__(self, rc, cols, by_id, device, codec=None):
        self.rc, self.by_id, self.device, self.codec = rc, by_id, device, codec
        self.cols = {k: (None if v is None else v.copy()) for k, v in cols.items()}
        self.cap = len(cols["state"])
        self.tab = P.make_table(rc, cols, by_id, device, codec)
        self.work = self.tab.close_work()
        self.killed, self.removed = set(), set()
        self.keep_index = False
        self.sync()

    def moved(self, device, codec=None):
        """This table copied to the other side, both indexes as they stand (they have one layout on host and
        device): -> a Harness over the copy."""
        h = Harness.__new__(Harness)
        h.rc, h.by_id, h.device, h.codec, h.cap = self.rc, self.by_id, device, codec, self.cap
        h.cols = {k: (None if v is None else v.copy()) for k, v in self.cols.items()}
        h.tab = self.tab.to(device)
        h.work = h.tab.close_work()
        h.killed, h.removed = set(self.killed), set(self.removed)
        h.keep_index = False
        return h

    def sync(self):
        if self.codec is not None:
            torch.cuda.synchronize()

    def t(self, a, dt):
        return None if a is None else P.tensor(np.ascontiguousarray(a, dt), self.device)

    def rebuild(self):
        self.tab.rebuild(self.codec)
        self.tab.rebuild_pick(self.codec)
        self.sync()

    def host_edit(self, state):
        """The host writes `state` and rebuilds both indexes (a revival, or the parent's way to close)."""
        self.cols["state"] = np.asarray(state, np.uint8).copy()
        self.tab.load(state=self.cols["state"])
        self.rebuild()

    def raw_close(self, close_rows=None, n_close=None, m_max=None, rst_first=None, remove=False, sweep=False, pick=True,
                  lists=True, stream=None, work=None):
        """One close; -> dict of the outputs as numpy (lists whole, slack behind them)."""
        cap, dev = self.cap, self.device
        o = {"marked_rows": filled(cap + 3, torch.int32, dev) if lists else None, "n_marked": filled(1, torch.int32, dev),
             "closed_rows": filled(cap + 3, torch.int32, dev) if lists else None, "n_closed": filled(1, torch.int32, dev),
             "pick_counts": filled(2, torch.int32, dev) if pick else None}
        kw = dict(o, remove=remove, sweep=sweep, pick=pick)
        if close_rows is not None:
            kw.update(close_rows=self.t(close_rows, np.uint32) if len(close_rows) else torch.zeros(1, dtype=torch.int32, device=dev),
                      n_close=self.t(np.array([n_close]), np.uint32), m_max=len(close_rows) if m_max is None else m_max)
        elif rst_first is not None:
            kw.update(rst_first=self.t(rst_first, np.uint32))
        w = self.work if work is None else work
        if self.codec is None:
            self.rc.conn_close_host(self.tab, w, **kw)
        else:
            self.codec.conn_close_batch(self.tab, w, stream=stream, **kw)
            torch.cuda.synchronize()
        return {k: host(v, np.uint32) for k, v in o.items() if v is not None}

    def close(self, close_rows=None, n_close=None, m_max=None, rst_first=None, remove=False, sweep=False, pick=True,
              picks=True):
        """A close with every checker behind it; -> the restatement's dict."""
        cap = self.cap
        if close_rows is not None:
            n_close = len(close_rows) if n_close is None else n_close
            m_max = len(close_rows) if m_max is None else m_max
            mask = list_marks(cap, close_rows, n_close, m_max)
        elif rst_first is not None:
            mask = np.asarray(rst_first, np.uint32) != NO_RST
        else:
            mask = np.zeros(cap, bool)
        ref = close_ref(self.cols["state"], mask, remove, sweep)
        index0, pick0 = self.tab.index.clone(), self.tab.pick.clone()
        got = self.raw_close(close_rows, n_close, m_max, rst_first, remove, sweep, pick)
        for lst, cnt in (("marked_rows", "n_marked"), ("closed_rows", "n_closed")):
            k = len(ref[lst])
            assert got[cnt][0] == k, (cnt, got[cnt][0], k)
            assert np.array_equal(got[lst][:k], ref[lst]), lst
            assert bool((got[lst][k:] == SENT32).all()), lst + ": written behind its count"
        self.killed |= set(ref["marked_rows"].tolist())
        self.removed |= set(ref["closed_rows"].tolist())
        self.cols["state"] = ref["state"]
        self.compare_columns()
        if len(ref["closed_rows"]) == 0:
            assert bool((self.tab.index == index0).all()), "the conn index was written though nothing was removed"
        if len(ref["closed_rows"]) == 0 and len(ref["marked_rows"]) == 0:
            assert bool((self.tab.pick == pick0).all()), "the pick index was written though nothing changed"
        if pick:
            groups = P.candidates(self.cols["state"], self.cols["id"], self.by_id)
            total = sum(len(g) for g in groups.values())
            n_groups = sum(1 for g in groups.values() if len(g))
            assert got["pick_counts"].tolist() == [n_groups, total], (got["pick_counts"], n_groups, total)
            assert host(self.tab.pick[:4], np.uint32).tolist() == [total, n_groups, 0, 0]
        self.check_lookups()
        if pick and picks:
            self.check_picks()
        return ref

    def compare_columns(self):
        for k, v in self.cols.items():
            if v is not None:
                got = host(getattr(self.tab, k), v.dtype)
                assert np.array_equal(got, v), (k, np.nonzero(got != v)[0][:8])

    # -- lookups --------------------------------------------------------------------------------------------
    def resolve(self, key, id):
        n = len(key)
        status = np.ones(n, np.int8)
        if self.codec is None:
            return self.rc.conn_resolve_host(self.tab, status, key, id=id if self.by_id else None)[0]
        conn = torch.zeros(n, dtype=torch.int32, device=self.device)
        self.codec.conn_resolve_batch(self.tab, self.t(status, np.int8), self.t(key, np.uint64), conn,
                                      id=self.t(id, np.uint8) if self.by_id else None)
        torch.cuda.synchronize()
        return host(conn, np.uint32)

    def check_lookups(self):
        """Every key of the table and absent keys: conn_ref on the new state, on the index as the call left it and
        on a rebuilt one (the rebuild leaves the same lookups, so the harness goes on with it)."""
        cols, cap = self.cols, self.cap
        rng = np.random.default_rng(cap)
        key = np.concatenate([cols["conn_key"], rng.integers(1, 2**63, 16, dtype=np.uint64)])
        idb = None
        if self.by_id:
            w = CR.id_words(cols["id"], cap)
            idb = P.id_bytes(np.concatenate([w, w[rng.integers(0, cap, 16)]]))
        tmap, _ = CR.table_map(cols["state"], cols["conn_key"], cols["id"] if self.by_id else None)
        want = CR.resolve_ref(tmap, np.ones(len(key), np.int8), key, id=idb)[0]
        got = self.resolve(key, idb)
        assert np.array_equal(got, want), ("index as left", np.nonzero(got != want)[0][:8])
        self.check_index("index as left")
        if self.keep_index:  # the scenario goes on with the index as the call left it
            return
        self.tab.rebuild(self.codec)
        self.sync()
        got = self.resolve(key, idb)
        assert np.array_equal(got, want), ("index rebuilt", np.nonzero(got != want)[0][:8])
        self.check_index("index rebuilt")

    def check_index(self, what):
        """rsk_conn.h's contract on the index as it stands (tests/collide.index_invariant), up to 4097 rows."""
        if self.cap <= 4097:
            CR.check_index(self.tab, self.cols, self.by_id, what=what)

    # -- picks ----------------------------------------------------------------------------------------------
    def pick_batch(self):
        """A batch that covers every group (also the ids whose last candidate went, and absent ids): per group the
        draws 0 .. m (the first of them for a large m), the multiples' edges and pick_ref.EDGE_DRAWS, and avoid
        keys naming a survivor, a killed row, a removed row, an absent key and a key of another id."""
        cols, cap, by_id = self.cols, self.cap, self.by_id
        rng = np.random.default_rng(cap * 3 + len(self.killed))
        w = CR.id_words(cols["id"] if by_id else None, cap)
        ids = np.unique(w).tolist() if by_id else [0]
        if by_id:
            ids += [int(x) for x in rng.integers(1, 2**63, 2, dtype=np.uint64)]
        groups = P.candidates(cols["state"], cols["id"], by_id)
        killed = np.array(sorted(self.killed - self.removed), np.int64)
        removed = np.array(sorted(self.removed), np.int64)
        per = max(14, min(4097 // max(len(ids), 1), 2200))
        wi, draw, avoid = [], [], []
        for idw in ids:
            g = groups.get(idw, np.zeros(0, np.int64))
            m = len(g)
            d = np.concatenate([np.arange(min(m + 1, per - 12)), [max(m - 1, 0), m, m + 1, 2 * m + 1], P.EDGE_DRAWS,
                                rng.integers(0, 2**32, 2)]).astype(np.uint64).astype(np.uint32)[:per]
            mine = lambda rows: rows[w[rows] == np.uint64(idw)] if len(rows) else rows  # noqa: E731
            pools = [g, mine(killed), mine(removed), None, np.nonzero(w != np.uint64(idw))[0]]
            a = np.zeros(len(d), np.uint64)
            for j in range(len(d)):
                kind = j % 6  # 5: no avoid key
                if kind == 3:
                    a[j] = rng.integers(1, 2**63, dtype=np.uint64)
                elif kind < 5 and pools[kind] is not None and len(pools[kind]):
                    a[j] = cols["conn_key"][pools[kind][rng.integers(0, len(pools[kind]))]]
            wi.append(np.full(len(d), idw, np.uint64))
            draw.append(d)
            avoid.append(a)
        wi, draw, avoid = np.concatenate(wi), np.concatenate(draw), np.concatenate(avoid)
        return {"id": P.id_bytes(wi) if by_id else None, "draw": draw, "avoid_key": avoid}, len(draw)

    def check_picks(self):
        b, n = self.pick_batch()
        got = P.run_pick(self.rc, self.tab, n, self.device, self.codec, **b)
        P.compare(got, P.rule_ref(self.cols, self.by_id, n, **b), "maintained index against the rule")
        fresh = self.tab.to(self.device)
        fresh.rebuild_pick(self.codec)
        self.sync()
        P.compare(got, P.run_pick(self.rc, fresh, n, self.device, self.codec, **b), "maintained against fresh index")
        assert bool((self.tab.pick[:4] == fresh.pick[:4]).all()), "header words"
        return got


# ---- tables ------------------------------------------------------------------------------------------------
def grouped_table(capacity, by_id, seed=0):
    """Random LIVE / ALIVE / NEW bits over `capacity` rows, a few duplicate keys (the lowest row is the key's conn;
    when it goes the next one is found).  BY_ID: groups of GROUP_SIZES candidates as far as they fit, the rest of
    the rows in at most ~60 further groups, every group's rows interleaved with the others'.  -> cols."""
    rng = np.random.default_rng(9000 + capacity * 2 + by_id + seed)
    cols = CR.random_columns(rng, capacity, by_id=by_id)
    cols["state"][:] = rng.choice(np.array([UP, UP, UP, UP | NEW, LIVE, LIVE | NEW, ALIVE, 0], np.uint8), capacity)
    if by_id:
        w = np.zeros(capacity, np.uint64)
        rows = rng.permutation(capacity)
        at, gid = 0, 1
        for m in GROUP_SIZES:
            if at + m > capacity:
                continue
            w[rows[at:at + m]] = gid
            cols["state"][rows[at:at + m]] = UP
            at, gid = at + m, gid + 1
        rest = rows[at:]
        if len(rest):
            w[rest] = gid + rng.integers(0, min(60, len(rest)), len(rest)).astype(np.uint64)
        w = (w * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x1234)  # spread ids; one group gets an odd word
        cols["id"][:] = P.id_bytes(w)
    if capacity >= 8:  # duplicates of a key inside one group
        src = rng.integers(0, capacity, max(2, capacity // 64))
        dst = rng.integers(0, capacity, len(src))
        cols["conn_key"][dst] = cols["conn_key"][src]
        if by_id:
            cols["id"].reshape(-1, 8)[dst] = cols["id"].reshape(-1, 8)[src]
    return cols


def pattern_rows(cols, by_id, pattern):
    """The rows a closing pattern names."""
    cap = len(cols["state"])
    groups = P.candidates(cols["state"], cols["id"], by_id)
    big = max(groups.values(), key=len) if groups else np.zeros(0, np.int64)
    if pattern == "nothing":
        return np.zeros(0, np.int64)
    if pattern == "one_row":
        return big[len(big) // 2: len(big) // 2 + 1] if len(big) else np.array([cap - 1])
    if pattern == "lowest_candidate":
        return big[:1] if len(big) else np.array([0])
    if pattern == "whole_group":
        if not by_id:
            return np.nonzero(cols["state"] & LIVE)[0]
        w = CR.id_words(cols["id"], cap)
        return np.nonzero(w == w[big[0]])[0] if len(big) else np.array([0])
    if pattern == "every_row":
        return np.arange(cap)
    return np.arange(0, cap, 2)


def as_column(cap, rows):
    rst = np.full(cap, NO_RST, np.uint32)
    rst[rows] = (np.arange(len(rows)) * 7 % 5000).astype(np.uint32)  # packet indices, 0 among them
    return rst


# ---- scenario 1: capacities x closing patterns -----------------------------------------------------------------
def scenario_patterns(rc, capacity, by_id, device, codec=None):
    cols = grouped_table(capacity, by_id)
    done = 0
    for j, pattern in enumerate(PATTERNS):
        rows = pattern_rows(cols, by_id, pattern)
        for form, remove in (("list", True), ("column", False)) + ((("column", True),) if pattern == "every_second_row" else ()):
            h = Harness(rc, cols, by_id, device, codec)
            if form == "list":
                ref = h.close(close_rows=np.random.default_rng(j).permutation(rows).astype(np.uint32), remove=remove)
            else:
                ref = h.close(rst_first=as_column(capacity, rows), remove=remove)
            done += len(ref["marked_rows"]) + len(ref["closed_rows"])
            if pattern == "nothing":
                assert len(ref["marked_rows"]) == len(ref["closed_rows"]) == 0
    return done


# ---- scenario 2: the list form's edges ---------------------------------------------------------------------------
def scenario_list_edges(rc, capacity, by_id, device, codec=None):
    cols = grouped_table(capacity, by_id, seed=1)
    cap = capacity
    rng = np.random.default_rng(cap)
    m = 2 * cap + 5
    lst = rng.integers(0, cap, m).astype(np.uint32)  # repeats, rows that are not LIVE
    lst[rng.permutation(m)[:4]] = np.array([cap, cap + 1, 2**31, 0xFFFFFFFF], np.uint32)
    h = Harness(rc, cols, by_id, device, codec)
    assert h.close(close_rows=lst, n_close=0, remove=True)["closed_rows"].size == 0
    assert h.close(close_rows=lst, n_close=7, m_max=0, remove=True)["closed_rows"].size == 0
    half = h.close(close_rows=lst, n_close=m + 100, m_max=max(cap // 3, 1), remove=True)  # n_close above m_max
    full = h.close(close_rows=lst, n_close=0xFFFFFFFF, remove=False)
    h.close(close_rows=lst, remove=True)
    return len(half["closed_rows"]), len(full["marked_rows"])


# ---- scenario 3: sweep -----------------------------------------------------------------------------------------
def scenario_sweep(rc, capacity, by_id, device, codec=None):
    cols = grouped_table(capacity, by_id, seed=2)
    cap = capacity
    dead_before = np.nonzero((cols["state"] & UP) == LIVE)[0]
    new_up = np.nonzero((cols["state"] & (UP | NEW)) == (UP | NEW))[0]
    rows = np.arange(1, cap, 3)
    if len(new_up):
        rows = np.union1d(rows, new_up[:1])  # a row with NEW set is marked and removed: it loses NEW too
    # sweep alone: IGroup::Flush
    h = Harness(rc, cols, by_id, device, codec)
    ref = h.close(sweep=True)
    assert np.array_equal(ref["closed_rows"], dead_before.astype(np.uint32)) and len(ref["marked_rows"]) == 0
    # rows dead before the call mixed with rows marked now, both forms
    for form in ("list", "column"):
        h = Harness(rc, cols, by_id, device, codec)
        kw = dict(close_rows=rows.astype(np.uint32)) if form == "list" else dict(rst_first=as_column(cap, rows))
        ref = h.close(sweep=True, **kw)
        assert set(dead_before.tolist()) <= set(ref["closed_rows"].tolist())
        assert not (ref["state"][ref["closed_rows"].astype(np.int64)] & (LIVE | ALIVE | NEW)).any()
    return len(dead_before)


# ---- scenario 4: sequences -------------------------------------------------------------------------------------
def scenario_sequences(rc, capacity, by_id, device, codec=None):
    cols = grouped_table(capacity, by_id, seed=3)
    cap = capacity
    rng = np.random.default_rng(cap + 5)
    # three closes in a row on one pick index, no rebuild of it between them
    h = Harness(rc, cols, by_id, device, codec)
    h.close(close_rows=rng.integers(0, cap, max(cap // 5, 1)).astype(np.uint32), remove=True)
    h.close(rst_first=as_column(cap, np.nonzero(rng.random(cap) < 0.3)[0]), remove=False)
    h.close(close_rows=rng.integers(0, cap, max(cap // 2, 1)).astype(np.uint32), remove=True, sweep=True)
    # kill only, then SWEEP
    h = Harness(rc, cols, by_id, device, codec)
    kill = h.close(close_rows=np.arange(0, cap, 2, dtype=np.uint32))
    assert len(kill["closed_rows"]) == 0
    swept = h.close(sweep=True)
    assert set(kill["marked_rows"].tolist()) <= set(swept["closed_rows"].tolist())
    # a close, a host-side revival of a row plus both rebuilds, a close again
    h = Harness(rc, cols, by_id, device, codec)
    first = h.close(rst_first=as_column(cap, np.arange(0, cap, 3)), remove=True)
    state = h.cols["state"].copy()
    back = first["closed_rows"][: max(len(first["closed_rows"]) // 2, 1)].astype(np.int64)
    state[back] |= UP
    h.host_edit(state)
    h.killed -= set(back.tolist())
    h.removed -= set(back.tolist())
    h.check_lookups()
    h.check_picks()
    h.close(close_rows=np.concatenate([back[::2], rng.integers(0, cap, 5)]).astype(np.uint32), remove=True)


# ---- scenario 4b: an emptied group must not cut other ids' probe chains ------------------------------------------
def scenario_probe_chains(rc, capacity, device, codec=None):
    """Every row its own group.  Two ids that share a home: the one placed later probes past the other's entry,
    whichever that is, so closing each half of the rows in turn (on a fresh table) makes a surviving id probe past
    an emptied group's entry in one of the two runs."""
    rng = np.random.default_rng(capacity + 77)
    cols = CR.random_columns(rng, capacity, by_id=True)
    cols["state"][:] = UP
    w = CR.id_words(cols["id"], capacity)
    homes = {}
    for r in range(capacity):
        homes.setdefault(group_home(int(w[r]), capacity), []).append(r)
    split = sum(1 for rows in homes.values() if len({r % 2 for r in rows}) == 2)
    assert split >= 3, "no two ids of different halves share a home: the table is badly chosen"
    for half in (0, 1):
        h = Harness(rc, cols, True, device, codec)
        ref = h.close(close_rows=np.arange(half, capacity, 2, dtype=np.uint32), remove=bool(half))
        assert len(ref["marked_rows"]) == len(range(half, capacity, 2))
        h.close(close_rows=np.arange(half, capacity, 4, dtype=np.uint32), remove=True)  # emptied entries are met again
    return split


# ---- scenario 4c: constructed clusters (tests/collide.py) ---------------------------------------------------------
COLLIDE_LENGTHS = CR.CLUSTER_LENGTHS  # the close runs on a full table: the run is as long as the table has rows


def collide_table(capacity, by_id, home, groups=7, live=None):
    """`live` rows (default: half of them) UP in random places, every key probing from `home`; BY_ID: over `groups`
    IdBufs whose group entries in the pick index probe from `home` too.  -> (cols, the groups' id words)."""
    from tests import collide as X

    rng = np.random.default_rng(capacity * 2 + by_id)
    cols = CR.random_columns(rng, capacity, by_id=by_id)
    rows = np.sort(rng.permutation(capacity)[: capacity // 2 if live is None else live])
    gids = X.ids_at(home, groups) if by_id else np.zeros(1, np.uint64)
    idw = gids[np.concatenate([np.arange(len(gids)), rng.integers(0, len(gids), len(rows))])[: len(rows)]]
    CR.place(cols, rows, X.keys_at(home, len(rows), idw), id=P.id_bytes(idw) if by_id else None)
    return cols, gids


def check_clusters(h, home, run):
    """The read-back proof that a harness's table is what the scenario says: the conn index one run of `run` entries
    from `home`, and (BY_ID, on a pick index that was just built) the groups' entries one run from `home` too."""
    from tests import collide as X

    X.one_run(h.tab.index.cpu().numpy(), home, run)
    if h.by_id:
        P.check_group_run(h.tab, h.cols, home)


def scenario_collide_close(rc, length, by_id, wrap, device, codec=None):
    """A full table of `length` rows that is ONE run of the index: every second row closed without and with REMOVE,
    then the rest; BY_ID: the groups of one pick home emptied one by one, so the groups behind them in the chain are
    picked past emptied entries."""
    from tests import collide as X

    home = CR.WRAP_HOME if wrap else CR.INNER_HOME
    cols, gids = collide_table(length, by_id, home, groups=9, live=length)
    live = np.arange(length)
    for remove in (False, True):
        h = Harness(rc, cols, by_id, device, codec)
        check_clusters(h, home, length)
        h.close(close_rows=live[0::2].astype(np.uint32), remove=remove)
        X.one_run(h.tab.index.cpu().numpy(), home, length - (len(live[0::2]) if remove else 0))
        h.close(close_rows=live[1::2].astype(np.uint32), remove=remove)
        h.close(sweep=True)
        assert not (h.cols["state"] & LIVE).any()
    if by_id:
        h = Harness(rc, cols, True, device, codec)
        w = CR.id_words(cols["id"], length)
        for j, g in enumerate(gids[::2].tolist() + gids[1::2].tolist()):
            h.close(close_rows=np.nonzero(w == np.uint64(g))[0].astype(np.uint32), remove=bool(j % 2))
        assert not ((h.cols["state"] & UP) == UP).any()
    return length


# ---- scenario 5: the reference's recorded control walk ---------------------------------------------------------
def scenario_walk_golden(rc, name, device, codec=None):
    """resolve -> control -> conn_close (column form, with pick) -> pick for the messages: no message travels on a
    row whose rst_first is set, and marked_rows are the conns the reference notified (EV_NOTIFY)."""
    c = G.case("walk", name)
    by_id = int(c["shape"]) == G.SERVER
    n, pool = len(c["cmd"]), c["pool"]
    cols, cap, row = G.walk_table(c)
    h = Harness(rc, cols, by_id, device, codec)
    b = dict(status=c["status"], cmd=c["cmd"], id=np.tile(np.ascontiguousarray(c["id"], np.uint8), n), conn_key=pool[c["ck"]],
             tcp_sp=None, tcp_dp=None, miss=None)
    b.update(G.frames(c, wild=codec is None))
    tries0 = np.full(cap, A.KA_NONE, np.uint8)
    got = C.run_control(rc, h.tab, b, device, codec, ka_tries=tries0)
    rf = got["rst_first"]
    ref = h.close(rst_first=rf)
    notified = np.unique(row[c["nt_conn"].astype(np.int64)]).astype(np.uint32)
    assert np.array_equal(ref["marked_rows"], notified)
    k = got["n_msg"]
    m = got["msgs"]
    draw = G.case_draws(c)[:k] if len(G.case_draws(c)) >= k else np.arange(k, dtype=np.uint32)
    idcol = np.ascontiguousarray(m["id"], np.uint8).ravel() if by_id else None
    conn, _nn, _used = P.run_pick(rc, h.tab, k, device, codec, id=idcol, avoid_key=m["avoid_key"], draw=draw)
    P.compare((conn, _nn, _used), P.rule_ref(h.cols, by_id, k, id=idcol, avoid_key=m["avoid_key"], draw=draw))
    sent = conn[conn != NONE].astype(np.int64)
    assert bool((rf[sent] == NO_RST).all()), "a message travels on a conn that a reset of the batch killed"
    return {"marked": len(notified), "msgs": k}


# ---- scenario 6: the reference's recorded keepalive timer ------------------------------------------------------
def scenario_timer_golden(rc, name, device, codec=None):
    """control_golden.scenario_timer's script with the table's state living on the device: the host's edit at "a
    timed-out conn is dead" is the list form on the flush's dead rows, the removals (rm_conn at rm_step, OP_REMOVE)
    the list form with REMOVE; every flush still gives the golden's requests, timeouts and mReqMap."""
    c = G.case("timer", name)
    by_id = int(c["shape"]) == G.SERVER
    nk, ne = len(c["keys"]), len(c["extra"])
    cap = nk + ne + 2
    rng = np.random.default_rng(nk)
    cols = CR.random_columns(rng, cap, by_id=by_id)
    row = rng.permutation(cap)[:nk + ne].astype(np.int64)
    cols["conn_key"][row] = np.concatenate([c["keys"], c["extra"]])
    fl = c["flags"].astype(np.uint8)
    cols["state"][row[:nk]] = LIVE | np.where(fl & G.F_ALIVE, ALIVE, 0) | np.where(fl & G.F_NEW, NEW, 0)
    if by_id:
        cols["id"].reshape(-1, 8)[:] = np.ascontiguousarray(c["id"], np.uint8)
    est = rng.integers(0, 2**62, cap, dtype=np.uint64)
    est[row[:nk]] = c["est"]
    tries = np.full(cap, A.KA_NONE, np.uint8)
    tries[row[c["req_key"]]] = c["req_tries"]
    h = Harness(rc, cols, by_id, device, codec)
    tab = h.tab
    online = bool(c["online"])
    conn_of_row = np.full(cap, -1, np.int64)
    conn_of_row[row] = np.arange(nk + ne)

    def clear_new(rows):  # INetConn::Output clears mNew: the host's, no index depends on it
        rows = np.asarray(rows, np.int64)
        h.cols["state"][rows] &= np.uint8(~NEW & 0xFF)
        tab.state[torch.from_numpy(rows).to(tab.state.device)] &= (~NEW & 0xFF)

    flushes = dead_total = removed_total = 0
    for s, (op, arg) in enumerate(zip(c["op"].tolist(), c["arg"].tolist())):
        if op == G.OP_FLUSH:
            tries, msgs, dead = C.run_flush(rc, tab, tries, est, int(arg), device, codec, online=online)
            want = c["snd_key"][c["snd_step"] == s]
            got_rows = msgs["src"].astype(np.int64)
            assert sorted(conn_of_row[got_rows].tolist()) == sorted(want.tolist()), s
            C.check_flush_msgs(msgs, got_rows, h.cols)
            to = c["nt_conn"][(c["nt_step"] == s) & (c["nt_code"] == G.ERR_TIMEOUT)]
            assert sorted(conn_of_row[dead.astype(np.int64)].tolist()) == sorted(to.tolist()), s
            want_tries = np.full(cap, A.KA_NONE, np.uint8)
            at = c["snap_step"] == s
            want_tries[row[c["snap_key"][at]]] = c["snap_tries"][at]
            assert np.array_equal(tries, want_tries), s
            ref = h.close(close_rows=dead.astype(np.uint32), n_close=len(dead), m_max=cap, picks=False)  # NotifyErr(ERR_TIMEOUT)
            assert len(ref["closed_rows"]) == 0
            clear_new(row[c["snd_conn"][(c["snd_step"] == s) & (c["snd_conn"] >= 0)]])
            flushes += 1
            dead_total += len(to)
        elif op == G.OP_RESP:
            tries[row[arg]] = A.KA_NONE
        elif op == G.OP_REMOVE:
            removed_total += len(h.close(close_rows=np.array([row[arg]], np.uint32), remove=True, picks=False)["closed_rows"])
        elif op == G.OP_CLEAR_NEW:
            clear_new([row[arg]])
        elif op == G.OP_ONLINE:
            online = bool(arg)
            tries[:] = A.KA_NONE
        rm = row[c["rm_conn"][c["rm_step"] == s]]
        if len(rm):
            removed_total += len(h.close(close_rows=rm.astype(np.uint32), remove=True, picks=False)["closed_rows"])
    h.check_picks()
    return {"flushes": flushes, "dead": dead_total, "removed": removed_total}


# ---- scenario 7: the reference's recorded doSend ---------------------------------------------------------------
def scenario_send_golden(rc, name, device, codec=None):
    """The table starts all LIVE | ALIVE with a built pick index; the reference's dead conns are killed by the list
    form with pick; control_golden.scenario_send's checks hold on the maintained index."""
    c = G.case("send", name)
    by_id = int(c["shape"]) == G.SERVER
    n, nk = len(c["avoid"]), len(c["keys"])
    avoid, draw = G.send_inputs(c)
    idcol = np.tile(np.ascontiguousarray(c["id"], np.uint8), n) if by_id else None
    sender = c["sender"].astype(np.int64)
    cols, row = G.send_table(c, c["order"])
    start = dict(cols, state=np.full(nk, UP, np.uint8))
    h = Harness(rc, start, by_id, device, codec)
    dead = np.nonzero((cols["state"] & UP) != UP)[0]
    ref = h.close(close_rows=np.random.default_rng(nk).permutation(dead).astype(np.uint32))
    assert np.array_equal(ref["state"], cols["state"]) and np.array_equal(ref["marked_rows"], dead.astype(np.uint32))
    conn, n_none, used = P.run_pick(rc, h.tab, n, device, codec, id=idcol, avoid_key=avoid, draw=draw)
    P.compare((conn, n_none, used), P.rule_ref(cols, by_id, n, id=idcol, avoid_key=avoid, draw=draw))
    exact = G.is_exact_send(c)
    if exact:
        want = np.where(sender >= 0, row[np.maximum(sender, 0)], NONE).astype(np.uint32)
        assert bool((c["consumed"] == 1).all()) and np.array_equal(conn, want)
    assert not np.isin(conn, dead).any()
    inside = (c["avoid"] >= 0) & (c["avoid"] < nk)
    assert not bool((conn[inside] == row[c["avoid"][inside]]).any())
    assert np.array_equal(conn == NONE, sender < 0) and n_none == int((sender < 0).sum())
    return {"dead": len(dead), "exact": exact}


# ---- scenario 8: arguments ---------------------------------------------------------------------------------------
def check_einval(rc, device, codec=None):
    """Every RSK_EINVAL of the close, with the outputs and the table untouched by a rejected call."""
    L = rc.lib()
    hs = {by_id: Harness(rc, grouped_table(300, by_id, seed=4), by_id, device, codec) for by_id in (False, True)}
    server, client = hs[True].tab, hs[False].tab
    ctx = () if codec is None else (codec._ctx,)
    tail = (1,) if codec is None else (None,)
    fn = L.rsk_conn_close_host if codec is None else L.rsk_conn_close_batch
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    lst = P.tensor(np.array([3, 0, 2, 2], np.uint32), device)
    ncl = P.tensor(np.array([4], np.uint32), device)
    rst = P.tensor(np.full(300, NO_RST, np.uint32), device)
    lists = filled(2 * 303, torch.int32, device)
    cnt = filled(4, torch.int32, device)
    work = hs[True].work

    def cin(form, **kw):
        d = dict(close_rows=None, n_close=None, m_max=0, rst_first=None, work=work.data_ptr(), flags=0)
        if form == "list":
            d.update(close_rows=lst.data_ptr(), n_close=ncl.data_ptr(), m_max=4)
        elif form == "column":
            d.update(rst_first=rst.data_ptr())
        d.update(kw)
        return A.ConnCloseIn(*[d[f] for f, _ in A.ConnCloseIn._fields_])

    def cout(**kw):
        d = dict(marked_rows=lists.data_ptr(), n_marked=cnt.data_ptr(), closed_rows=lists.data_ptr() + 4 * 303,
                 n_closed=cnt.data_ptr() + 4, pick=server.pick.data_ptr(), pick_counts=cnt.data_ptr() + 8)
        d.update(kw)
        return A.ConnCloseOut(*[d[f] for f, _ in A.ConnCloseOut._fields_])

    S, SR, E = server.abi, server.abi_rows, A.EINVAL
    sweep = A.CONN_CLOSE_SWEEP
    cases = [("null tab", None, SR(), cin("list"), cout()), ("null rows", S(), None, cin("list"), cout()),
             ("null in", S(), SR(), None, cout()), ("null out", S(), SR(), cin("list"), None),
             ("null work", S(), SR(), cin("list", work=None), cout()),
             ("rows not the table's", S(), A.ConnRows(client.state.data_ptr()), cin("list"), cout()),
             ("rows NULL", S(), A.ConnRows(None), cin("list"), cout()),
             ("both sources", S(), SR(), cin("list", rst_first=rst.data_ptr()), cout()),
             ("both sources, sweep", S(), SR(), cin("list", rst_first=rst.data_ptr(), flags=sweep), cout()),
             ("no source without SWEEP", S(), SR(), cin("none"), cout()),
             ("no source, REMOVE only", S(), SR(), cin("none", flags=A.CONN_CLOSE_REMOVE), cout()),
             ("unknown flags", S(), SR(), cin("list", flags=4), cout()),
             ("unknown flags high", S(), SR(), cin("column", flags=0x80000001), cout()),
             ("list without n_close", S(), SR(), cin("list", n_close=None), cout()),
             ("marked_rows without n_marked", S(), SR(), cin("list"), cout(n_marked=None)),
             ("closed_rows without n_closed", S(), SR(), cin("column"), cout(n_closed=None)),
             ("work misaligned", S(), SR(), cin("list", work=work.data_ptr() + 8), cout()),
             ("pick misaligned", S(), SR(), cin("list"), cout(pick=server.pick.data_ptr() + 4))]
    for field, val in (("flags", 2), ("flags", 0x80000001), ("capacity", 0), ("capacity", A.CONN_MAX_ROWS + 1),
                       ("state", None), ("conn_key", None), ("index", None), ("id", None)):
        t = S()
        setattr(t, field, val)
        cases.append((f"tab.{field}={val}", t, SR(), cin("list"), cout()))  # id NULL: pick on a BY_ID table without id
    t = S()
    t.index += 4
    cases.append(("tab.index misaligned", t, SR(), cin("list"), cout()))
    t = S()
    t.id += 4
    cases.append(("tab.id misaligned", t, SR(), cin("list"), cout()))
    before = {k: host(getattr(server, k), np.uint8).copy() for k in ("state", "index", "pick")}

    def untouched():
        if codec is not None:
            torch.cuda.synchronize()
        return (all(bool((x.cpu().view(torch.uint8) == SENT).all()) for x in (lists, cnt))
                and all(np.array_equal(host(getattr(server, k), np.uint8), v) for k, v in before.items()))

    for label, t, r, i, o in cases:
        if codec is None and "id misaligned" in label:  # the host twin reads ids bytewise
            continue
        assert fn(*ctx, ref(t), ref(r), ref(i), ref(o), *tail) == E, label
        assert untouched(), label
    if codec is not None:
        assert L.rsk_conn_close_batch(None, ref(S()), ref(SR()), ref(cin("list")), ref(cout()), None) == E
    # the valid calls do run, and change nothing here: rows 0, 2, 3 made not LIVE first
    for h in hs.values():
        st = h.cols["state"].copy()
        st[[0, 2, 3]] = 0
        h.host_edit(st)
    for k in before:
        before[k] = host(getattr(server, k), np.uint8).copy()
    for i, o in ((cin("list"), cout()), (cin("column"), cout()), (cin("list", m_max=0), cout(marked_rows=None, n_marked=None)),
                 (cin("column"), cout(pick=None, pick_counts=None, closed_rows=None, n_closed=None))):
        assert fn(*ctx, ref(S()), ref(SR()), ref(i), ref(o), *tail) == A.OK
    crow = A.ConnRows(client.state.data_ptr())
    assert fn(*ctx, ref(client.abi()), ref(crow), ref(cin("list", work=hs[False].work.data_ptr())),
              ref(cout(pick=client.pick.data_ptr())), *tail) == A.OK
    if codec is not None:
        torch.cuda.synchronize()
    assert host(cnt, np.uint32)[:2].tolist() == [0, 0] and bool((lists.cpu().view(torch.uint8) == SENT).all())
    assert all(np.array_equal(host(getattr(server, k), np.uint8), v) for k, v in before.items())
    assert L.rsk_conn_close_bytes(0, 0) == 0 and L.rsk_conn_close_bytes(A.CONN_MAX_ROWS + 1, 0) == 0
    assert L.rsk_conn_close_bytes(16, 2) == 0
    for cap in (1, 15, 17, 1024, 1025, A.CONN_MAX_ROWS):
        small, large = L.rsk_conn_close_bytes(cap, 0), L.rsk_conn_close_bytes(cap, A.CONN_BY_ID)
        assert small % 16 == 0 and large % 16 == 0 and large - small == 4 * ((cap + 3) // 4 * 4)
