"""TEST INFRASTRUCTURE: the four rules of the tuple pool (include/rsk_codec.h, rsk_pool_*) in numpy / Python, written
from the reference's TcpAckPool (net/TcpAckPool.cpp: AddInfoFromPeer :17-33, Wait2TransferInfo :35-60, OnFlush
:85-95) and ServerNetManager (server/ServerNetManager.cpp: GetTcp :52-75, OnFlush :82-103, add2Pool :105-117), and
`Lib`, which runs the same four calls through the library (the host twins, or the batch calls of a Codec) with
sentinel-filled outputs.

A pool is a dict of columns (state, src, dst, sp, dp, seq, ack, expiry; the model also keeps the handshake's flag,
which the library's pool has no column for).  Every *_ref returns new columns and leaves its arguments alone.

`mutant` bends one rule, to show that a fixture sees it:
  last_syn_wins              a later handshake of a pooled tuple replaces its seq / ack
  socket_touch_moves_expiry  an add without TOUCH moves the expiry of a pooled tuple all the same
  zero_ports_kept            a row with a zero port is pooled
  ack_from_seq               an offer's ack is the record's seq
  flag_from_syn              an offer's flag is the handshake's
  no_purge                   the settle skips rule (b)
  purge_whole_offers         rule (b) also removes a tuple that both pools hold
  expiry_strict              the flush compares expiry < now"""
from __future__ import annotations

import numpy as np

from rsock_amd import _abi as A

MUTANTS = ("last_syn_wins", "socket_touch_moves_expiry", "zero_ports_kept", "ack_from_seq", "flag_from_syn", "no_purge",
           "purge_whole_offers", "expiry_strict")
NONE = A.CONN_NONE
LIVE = A.POOL_LIVE
TH_ACK = 0x10
SENTINEL = 0xA5A5A5A5
COLS = (("state", np.uint8), ("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
        ("seq", np.uint32), ("ack", np.uint32), ("expiry", np.uint64))
TUPLE = ("src", "sp", "dst", "dp")  # TcpCmpFn's order


def empty(capacity: int, vals: bool = True, rng=None) -> dict:
    """A pool without a LIVE row; with rng every other bit and column random."""
    c = {k: np.zeros(capacity, dt) for k, dt in COLS if vals or k not in ("seq", "ack")}
    if rng is not None:
        for k, dt in COLS:
            if k in c:
                c[k] = rng.integers(0, np.iinfo(dt).max, capacity, dtype=dt, endpoint=True)
        c["state"] &= np.uint8(~LIVE & 0xFF)
    c["flag"] = np.zeros(capacity, np.uint8)
    return c


def key_for_tcp(sp, dp):
    return np.uint64(0x10000000) | (np.asarray(dp, np.uint64) << np.uint64(16)) | np.asarray(sp, np.uint64)


def tuples(c, rows=None):
    rows = range(len(c["src"])) if rows is None else rows
    return [tuple(int(c[k][r]) for k in TUPLE) for r in rows]


def live_map(c) -> dict:
    """tuple -> its lowest LIVE row."""
    m = {}
    for r in np.nonzero(c["state"] & LIVE)[0].tolist():
        m.setdefault(tuple(int(c[k][r]) for k in TUPLE), r)
    return m


def snapshot(c) -> tuple:
    """The LIVE rows sorted by (src, sp, dst, dp): ([k, 6] src, dst, sp, dp, seq, ack -- 4 columns without seq /
    ack -- and the expiries)."""
    rows = sorted(np.nonzero(c["state"] & LIVE)[0].tolist(), key=lambda r: tuple(int(c[k][r]) for k in TUPLE))
    names = ("src", "dst", "sp", "dp") + (("seq", "ack") if "seq" in c else ())
    a = np.array([[int(c[k][r]) for k in names] for r in rows], np.uint32).reshape(-1, len(names))
    return a, np.array([int(c["expiry"][r]) for r in rows], np.uint64)


def _copy(c):
    return {k: v.copy() for k, v in c.items()}


def add_ref(c, inp, expiry, u_max, touch, parse_status=None, mutant=None):
    """-> (columns, outputs).  inp: src, dst, sp, dp and, for a pool with records, seq, ack (flag optional)."""
    c = _copy(c)
    n = len(inp["src"])
    m = live_map(c)
    vacant = iter(np.nonzero((c["state"] & LIVE) == 0)[0].tolist())
    new_rows, new_first, refused = [], [], set()
    n_again = n_zero = taken = 0
    for i in range(n):
        if parse_status is not None and parse_status[i] != A.PARSE_SYN:
            continue
        if (int(inp["sp"][i]) == 0 or int(inp["dp"][i]) == 0) and mutant != "zero_ports_kept":
            n_zero += 1
            continue
        if taken == u_max:
            continue
        taken += 1
        k = tuple(int(inp[f][i]) for f in TUPLE)
        r = m.get(k)
        if r is not None:
            n_again += 1
            if touch or mutant == "socket_touch_moves_expiry":
                c["expiry"][r] = expiry
            if mutant == "last_syn_wins" and "seq" in c:
                c["seq"][r], c["ack"][r] = inp["seq"][i], inp["ack"][i]
            continue
        if k in refused:
            n_again += 1
            continue
        r = next(vacant, None)
        if r is None:
            refused.add(k)
            continue
        for f in ("src", "dst", "sp", "dp"):
            c[f][r] = inp[f][i]
        if "seq" in c:
            c["seq"][r], c["ack"][r] = inp["seq"][i], inp["ack"][i]
        c["flag"][r] = inp["flag"][i] if "flag" in inp else 0
        c["expiry"][r] = expiry
        c["state"][r] = LIVE
        m[k] = r
        new_rows.append(r)
        new_first.append(i)
    row = np.full(n, NONE, np.uint32)
    for i in range(n):
        if parse_status is not None and parse_status[i] != A.PARSE_SYN:
            continue
        if (int(inp["sp"][i]) == 0 or int(inp["dp"][i]) == 0) and mutant != "zero_ports_kept":
            continue
        row[i] = m.get(tuple(int(inp[f][i]) for f in TUPLE), NONE)
    return c, {"row": row, "new_rows": np.array(new_rows, np.uint32), "new_first": np.array(new_first, np.uint32),
               "n_new": len(new_rows), "n_again": n_again, "n_full": len(refused), "n_zero_port": n_zero}


def offers_ref(ca, cs, m_max, conn_key=False, mutant=None):
    ms = live_map(cs)
    rows = [(r, ms[t]) for r, t in ((r, tuple(int(ca[k][r]) for k in TUPLE)) for r in np.nonzero(ca["state"] & LIVE)[0].tolist())
            if t in ms]
    total = len(rows)
    rows = rows[:m_max]
    ar = np.array([a for a, _ in rows], np.int64)
    o = {k: ca[k][ar] for k in ("src", "dst", "sp", "dp")}
    o["ack"] = ca["seq" if mutant == "ack_from_seq" else "ack"][ar]
    o["flag"] = ca["flag"][ar] if mutant == "flag_from_syn" else np.full(len(ar), TH_ACK, np.uint8)
    if conn_key:
        o["conn_key"] = key_for_tcp(o["sp"], o["dp"])
    o.update(n_offer=len(rows), n_over=total - len(rows), offer_ack_row=ar.astype(np.uint32),
             offer_sock_row=np.array([s for _, s in rows], np.uint32))
    return o


def settle_ref(ca, cs, new_offer, n_new, offer_ack_row, offer_sock_row, miss, pk, mutant=None):
    """pk: the packets' src, dst, sp, dp.  -> (ack columns, socket columns, outputs)."""
    ca, cs = _copy(ca), _copy(cs)
    taken = []
    for j in range(min(int(n_new), len(new_offer))):
        o = int(new_offer[j])
        ar, sr = int(offer_ack_row[o]), int(offer_sock_row[o])
        ca["state"][ar] &= np.uint8(~LIVE & 0xFF)
        cs["state"][sr] &= np.uint8(~LIVE & 0xFF)
        taken.append(sr)
    ma, ms = live_map(ca), live_map(cs)
    closed, purged = set(), set()
    if mutant != "no_purge":
        for i in np.nonzero(np.asarray(miss) == A.RECV_VALID)[0].tolist():
            k = tuple(int(pk[f][i]) for f in TUPLE)
            if k in ma and k in ms and mutant != "purge_whole_offers":
                continue
            if k in ma:
                purged.add(ma[k])
            if k in ms:
                closed.add(ms[k])
    for r in purged:
        ca["state"][r] &= np.uint8(~LIVE & 0xFF)
    for r in closed:
        cs["state"][r] &= np.uint8(~LIVE & 0xFF)
    return ca, cs, {"taken_sock_rows": np.array(taken, np.uint32), "closed_sock_rows": np.array(sorted(closed), np.uint32),
                    "n_closed": len(closed), "n_purged_ack": len(purged)}


def flush_ref(c, now, mutant=None):
    c = _copy(c)
    live = (c["state"] & LIVE) != 0
    dead = live & ((c["expiry"] < np.uint64(now)) if mutant == "expiry_strict" else (c["expiry"] <= np.uint64(now)))
    c["state"][dead] &= np.uint8(~LIVE & 0xFF)
    rows = np.nonzero(dead)[0].astype(np.uint32)
    return c, {"dead_rows": rows, "n_dead": len(rows)}


class RefPools:
    """The two pools of a server in the model, behind the interface tests/pool_golden.py drives."""

    def __init__(self, cap_ack, cap_sock, mutant=None):
        self.a, self.s, self.mutant = empty(cap_ack), empty(cap_sock, vals=False), mutant

    def harvest(self, t, expiry):
        self.a, o = add_ref(self.a, t, expiry, max(len(t["src"]), 1), True, t["parse_status"], self.mutant)
        return o

    def accept(self, inp, expiry):
        self.s, o = add_ref(self.s, inp, expiry, max(len(inp["src"]), 1), False, None, self.mutant)
        return o

    def offers(self, m_max, conn_key=False):
        return offers_ref(self.a, self.s, m_max, conn_key, self.mutant)

    def settle(self, off, got, pk):
        self.a, self.s, o = settle_ref(self.a, self.s, got["new_offer"], int(got["n_new"][0]), off["offer_ack_row"],
                                       off["offer_sock_row"], got["miss"], pk, self.mutant)
        return o

    def flush(self, which, now):
        if which == 0:
            self.a, o = flush_ref(self.a, now, self.mutant)
        else:
            self.s, o = flush_ref(self.s, now, self.mutant)
        return o

    def columns(self):
        return self.a, self.s

    def check_indexes(self, what=""):
        pass


# ---- the library ---------------------------------------------------------------------------------------------------
def _host(t, dt):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)
    return a.view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else a.astype(dt)


class Lib:
    """The four calls through the library: device "cpu" = the host twins, a cuda device = the batch calls of
    `codec`.  Every output is sentinel-filled first and checked to be untouched behind its list's end."""

    def __init__(self, rc, device="cpu", codec=None):
        self.rc, self.device, self.codec = rc, device, codec

    def t(self, a, dt=None):
        import torch

        a = np.ascontiguousarray(a if dt is None else np.asarray(a).astype(dt))
        v = a.view(np.uint8 if a.dtype.itemsize == 1 and a.dtype != np.int8 else f"i{a.dtype.itemsize}")
        return torch.from_numpy(v.copy()).to(self.device)

    def fill(self, k, dt=np.uint32):
        return self.t(np.full(max(k, 1), SENTINEL & np.iinfo(dt).max, dt))

    def sync(self):
        if self.codec is not None:
            import torch

            torch.cuda.synchronize()

    def table(self, c, rebuild=True):
        vals = "seq" in c
        tab = self.rc.PoolTable.alloc(len(c["state"]), self.device, vals=vals)
        tab.load(**{k: c[k] for k, _ in COLS if k in c})
        if rebuild:
            tab.rebuild(self.codec)
            self.sync()
        return tab

    @staticmethod
    def columns(tab) -> dict:
        return {k: tab.column(k) for k, _ in COLS if getattr(tab, k) is not None}

    def _tail(self, t, used, dt, what):
        a = _host(t, dt)
        assert bool((a[used:] == (SENTINEL & np.iinfo(dt).max)).all()), (what, "written behind the list's end", used)
        return a[:used].copy()

    def add(self, tab, inp, expiry, u_max, touch, parse_status=None, work=None, stream=None):
        n = len(inp["src"])
        m = min(u_max, tab.capacity)
        work = tab.add_work(u_max) if work is None else work
        col = lambda k, dt: self.t(inp[k], dt) if k in inp and getattr(tab, k, True) is not None else None  # noqa: E731
        row, nr, nf = self.fill(n), self.fill(m + 3), self.fill(m + 3)
        cnt = self.fill(4)
        kw = dict(seq=col("seq", np.uint32), ack=col("ack", np.uint32),
                  parse_status=None if parse_status is None else self.t(parse_status, np.int8), touch=touch, row=row,
                  new_rows=nr, new_first=nf, n_new=cnt[0:1], n_again=cnt[1:2], n_full=cnt[2:3], n_zero_port=cnt[3:4])
        args = (tab, self.t(inp["src"], np.uint32), self.t(inp["dst"], np.uint32), self.t(inp["sp"], np.uint16),
                self.t(inp["dp"], np.uint16), expiry, u_max, work)
        if self.codec is None:
            self.rc.pool_add_host(*args, **kw)
        else:
            self.codec.pool_add_batch(*args, stream=stream, **kw)
            self.sync()
        c = _host(cnt, np.uint32)
        k = int(c[0])
        assert k <= m
        return {"row": _host(row, np.uint32)[:n].copy(), "new_rows": self._tail(nr, k, np.uint32, "new_rows"),
                "new_first": self._tail(nf, k, np.uint32, "new_first"), "n_new": k, "n_again": int(c[1]), "n_full": int(c[2]),
                "n_zero_port": int(c[3])}

    def offer_buffers(self, m_max, conn_key=False):
        b = {"src": self.fill(m_max), "dst": self.fill(m_max), "sp": self.fill(m_max, np.uint16), "dp": self.fill(m_max, np.uint16),
             "ack": self.fill(m_max), "flag": self.fill(m_max, np.uint8), "n_offer": self.fill(1), "n_over": self.fill(1),
             "offer_ack_row": self.fill(m_max), "offer_sock_row": self.fill(m_max)}
        if conn_key:
            b["conn_key"] = self.t(np.full(m_max, 0xA5A5A5A5A5A5A5A5, np.uint64))
        return b

    def conn_offers(self, b, m_max):
        return self.rc.ConnOffers(b["src"], b["dst"], b["sp"], b["dp"], b["ack"], b["flag"], b["n_offer"],
                                  conn_key=b.get("conn_key"), m_max=m_max)

    def offers(self, ta, ts, m_max, conn_key=False, stream=None):
        b = self.offer_buffers(m_max, conn_key)
        kw = dict(offer_ack_row=b["offer_ack_row"], offer_sock_row=b["offer_sock_row"], n_over=b["n_over"])
        if self.codec is None:
            self.rc.pool_offers_host(ta, ts, self.conn_offers(b, m_max), **kw)
        else:
            self.codec.pool_offers(ta, ts, self.conn_offers(b, m_max), stream=stream, **kw)
            self.sync()
        k = int(_host(b["n_offer"], np.uint32)[0])
        assert k <= m_max
        o = {"n_offer": k, "n_over": int(_host(b["n_over"], np.uint32)[0])}
        for name, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16), ("ack", np.uint32),
                         ("flag", np.uint8), ("offer_ack_row", np.uint32), ("offer_sock_row", np.uint32)):
            o[name] = self._tail(b[name], k, dt, name)
        if conn_key:
            ck = _host(b["conn_key"], np.uint64)
            assert bool((ck[k:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()), "conn_key written behind the list's end"
            o["conn_key"] = ck[:k].copy()
        return o

    def settle(self, ta, ts, new_offer, n_new, offer_ack_row, offer_sock_row, miss, pk, work=None, stream=None):
        m_max, new_max = max(len(offer_ack_row), 1), len(new_offer)
        work = ta.settle_work(ts) if work is None else work
        taken, closed, cnt = self.fill(new_max + 3), self.fill(ts.capacity + 3), self.fill(2)
        pad = lambda a: np.concatenate([np.asarray(a, np.uint32), np.zeros(1, np.uint32)])[:max(len(a), 1)]  # noqa: E731
        kw = dict(new_offer=self.t(pad(new_offer), np.uint32) if new_max else None,
                  n_new=self.t(np.array([n_new], np.uint32)) if new_max else None,
                  offer_ack_row=self.t(pad(offer_ack_row), np.uint32), offer_sock_row=self.t(pad(offer_sock_row), np.uint32),
                  m_max=m_max, new_max=new_max, taken_sock_rows=taken, closed_sock_rows=closed, n_closed=cnt[0:1],
                  n_purged_ack=cnt[1:2])
        if len(miss):
            kw.update(miss=self.t(miss, np.int8), src=self.t(pk["src"], np.uint32), dst=self.t(pk["dst"], np.uint32),
                      sp=self.t(pk["sp"], np.uint16), dp=self.t(pk["dp"], np.uint16))
        if self.codec is None:
            self.rc.pool_settle_host(ta, ts, work, **kw)
        else:
            self.codec.pool_settle_batch(ta, ts, work, stream=stream, **kw)
            self.sync()
        c = _host(cnt, np.uint32)
        return {"taken_sock_rows": self._tail(taken, min(int(n_new), new_max), np.uint32, "taken_sock_rows"),
                "closed_sock_rows": self._tail(closed, int(c[0]), np.uint32, "closed_sock_rows"), "n_closed": int(c[0]),
                "n_purged_ack": int(c[1])}

    def flush(self, tab, now, stream=None):
        dead, cnt = self.fill(tab.capacity + 3), self.fill(1)
        if self.codec is None:
            self.rc.pool_flush_host(tab, now, dead_rows=dead, n_dead=cnt)
        else:
            self.codec.pool_flush(tab, now, dead_rows=dead, n_dead=cnt, stream=stream)
            self.sync()
        k = int(_host(cnt, np.uint32)[0])
        return {"dead_rows": self._tail(dead, k, np.uint32, "dead_rows"), "n_dead": k}


def index_check(tab, what=""):
    """rsk_conn.h's contract on a pool's index (tests/collide.py)."""
    from tests import collide

    c = Lib.columns(tab)
    key = (c["src"].astype(np.uint64) << np.uint64(32)) | c["dst"].astype(np.uint64)
    ports = (c["sp"].astype(np.uint64) << np.uint64(16)) | c["dp"].astype(np.uint64)
    return collide.index_invariant(tab.column("index"), tab.capacity, c["state"], key, ports, by_id=True, what=what)


class LibPools:
    """The two pools of a server in the library, behind the interface tests/pool_golden.py drives."""

    def __init__(self, lib: Lib, cap_ack, cap_sock):
        self.lib = lib
        self.ta = lib.table(empty(cap_ack, rng=np.random.default_rng(cap_ack)))
        self.ts = lib.table(empty(cap_sock, vals=False, rng=np.random.default_rng(cap_sock + 1)))

    def harvest(self, t, expiry):
        return self.lib.add(self.ta, t, expiry, max(len(t["src"]), 1), True, t["parse_status"])

    def accept(self, inp, expiry):
        return self.lib.add(self.ts, inp, expiry, max(len(inp["src"]), 1), False)

    def offers(self, m_max, conn_key=False):
        return self.lib.offers(self.ta, self.ts, m_max, conn_key)

    def settle(self, off, got, pk):
        return self.lib.settle(self.ta, self.ts, got["new_offer"], int(got["n_new"][0]), off["offer_ack_row"],
                               off["offer_sock_row"], got["miss"], pk)

    def flush(self, which, now):
        return self.lib.flush(self.ta if which == 0 else self.ts, now)

    def columns(self):
        return Lib.columns(self.ta), Lib.columns(self.ts)

    def check_indexes(self, what=""):
        index_check(self.ta, what + " ack pool")
        index_check(self.ts, what + " socket pool")


# ---- property cases: the library against the rules ---------------------------------------------------------------
def same_columns(tab, want, what):
    got = Lib.columns(tab)
    for k, v in got.items():
        assert np.array_equal(v, want[k]), (what, "column", k, np.nonzero(v != want[k])[0][:8])


def same_outputs(got, want, what):
    for k, v in want.items():
        if k in got:
            assert np.array_equal(np.asarray(got[k]), np.asarray(v)), (what, k, np.asarray(got[k]).tolist()[:8], np.asarray(v).tolist()[:8])


def universe(rng, k, home=None):
    """k distinct 4-tuples with non-zero ports: random, or (home given) all probing from one index entry."""
    if home is not None:
        from tests import collide

        src, dst, sp, dp = collide.tuples_at(home, k)
        assert bool((sp != 0).all() and (dp != 0).all())
        return {"src": src, "dst": dst, "sp": sp, "dp": dp}
    sp = rng.integers(1, 65536, k).astype(np.uint16)
    return {"src": rng.integers(0, 2**32, k, dtype=np.uint64).astype(np.uint32), "dst": np.arange(k, dtype=np.uint32) * np.uint32(2654435761),
            "sp": sp, "dp": rng.integers(1, 65536, k).astype(np.uint16)}


def filled(rng, capacity, live_rows, uni, first, vals):
    """A pool whose rows live_rows hold the tuples uni[first:], every other bit and column random."""
    c = empty(capacity, vals, rng)
    r = np.asarray(live_rows, np.int64)
    for f in ("src", "dst", "sp", "dp"):
        c[f][r] = uni[f][first:first + len(r)]
    c["state"][r] |= np.uint8(LIVE)
    c["expiry"][r] = rng.integers(100, 200, len(r)).astype(np.uint64)
    return c


def property_case(libs, seed, n, capacity, fill, kind, u_short=False, m_short=False, n_new_zero=False, home=None):
    """One chain add (ack pool, TOUCH, parse_status) -> add (socket pool, list form) -> offers -> settle -> flush on
    every lib of `libs`, each step compared with the rule (integer-exact outputs and tables, rsk_conn.h's contract on
    every index).  fill: "empty" / "half" / "full" (the adds run out of rows: n_full); kind: "same" (every row one
    tuple), "different" (every row another) or "mixed"."""
    rng = np.random.default_rng(seed)
    k_live = {"empty": 0, "half": capacity // 2, "full": capacity}[fill]
    n_uni = max(n, 1) + 2 * capacity + 8
    uni = universe(rng, n_uni, home)
    rows_a = np.sort(rng.choice(capacity, k_live, replace=False))
    rows_s = np.sort(rng.choice(capacity, k_live, replace=False))
    ca = filled(rng, capacity, rows_a, uni, 0, True)
    cs = filled(rng, capacity, rows_s, uni, k_live // 2, False)  # the pools share half of their tuples
    # the rows of the batch
    if kind == "same":
        pick = np.full(n, n_uni - 1, np.int64)
    elif kind == "different":
        pick = 2 * capacity + np.arange(n, dtype=np.int64)
    else:
        pick = rng.integers(0, n_uni, n)
    inp = {f: uni[f][pick].copy() for f in ("src", "dst", "sp", "dp")}
    inp["seq"], inp["ack"] = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    inp["flag"] = np.full(n, 0x02, np.uint8)
    status = np.full(n, A.PARSE_SYN, np.int8)
    if n > 3 and kind != "same":
        z = rng.choice(n, max(1, n // 16), replace=False)
        inp["sp"][z[::2]] = 0
        inp["dp"][z[1::2]] = 0
        status[rng.choice(n, max(1, n // 8), replace=False)] = rng.choice(np.array([0, 1, 3], np.int8), max(1, n // 8))
    considered = int(((status == A.PARSE_SYN) & (inp["sp"] != 0) & (inp["dp"] != 0)).sum())
    u_max = max(1, considered // 2) if u_short else max(n, 1)
    want_a, wo_a = add_ref(ca, inp, 1000, u_max, True, status)
    acc = {f: inp[f][::-1].copy() for f in ("src", "dst", "sp", "dp")}  # the accepted tuples: the same, the other way round
    want_s, wo_s = add_ref(cs, acc, 2000, u_max, False)
    if fill == "full":
        assert wo_a["n_new"] == 0
    matches = offers_ref(want_a, want_s, 1 << 21)["n_offer"]
    m_max = max(1, matches // 2) if m_short else max(matches, 1)
    w_off = offers_ref(want_a, want_s, m_max, conn_key=True)
    assert w_off["n_over"] == matches - w_off["n_offer"]
    # the create's outputs: some offers became conns; some packets still miss, with tuples of every kind
    k_off = w_off["n_offer"]
    new_offer = rng.permutation(k_off)[: k_off // 2].astype(np.uint32)
    n_new = 0 if n_new_zero else len(new_offer)
    npk = n
    ppick = rng.integers(0, n_uni, npk)
    pk = {f: uni[f][ppick].copy() for f in ("src", "dst", "sp", "dp")}
    miss = rng.choice(np.array([A.RECV_VALID, A.RECV_DROP], np.int8), npk)
    want_a2, want_s2, w_st = settle_ref(want_a, want_s, new_offer, n_new, w_off["offer_ack_row"], w_off["offer_sock_row"], miss, pk)
    now = 150
    want_a3, w_fa = flush_ref(want_a2, now)
    want_s3, w_fs = flush_ref(want_s2, now)
    for lib in libs:
        what = f"{lib.device} seed {seed}"
        ta, ts = lib.table(ca), lib.table(cs)
        same_outputs(lib.add(ta, inp, 1000, u_max, True, status), wo_a, what + " add ack")
        same_columns(ta, want_a, what + " add ack")
        index_check(ta, what + " add ack")
        same_outputs(lib.add(ts, acc, 2000, u_max, False), wo_s, what + " add sock")
        same_columns(ts, want_s, what + " add sock")
        index_check(ts, what + " add sock")
        off = lib.offers(ta, ts, m_max, conn_key=True)
        same_outputs(off, w_off, what + " offers")
        st = lib.settle(ta, ts, new_offer, n_new, off["offer_ack_row"], off["offer_sock_row"], miss, pk)
        same_outputs(st, w_st, what + " settle")
        same_columns(ta, want_a2, what + " settle ack")
        same_columns(ts, want_s2, what + " settle sock")
        index_check(ta, what + " settle ack")
        index_check(ts, what + " settle sock")
        same_outputs(lib.flush(ta, now), w_fa, what + " flush ack")
        same_outputs(lib.flush(ts, now), w_fs, what + " flush sock")
        same_columns(ta, want_a3, what + " flush ack")
        same_columns(ts, want_s3, what + " flush sock")
        index_check(ta, what + " flush ack")
        index_check(ts, what + " flush sock")
    return {"n_new": wo_a["n_new"], "n_full": wo_a["n_full"] + wo_s["n_full"], "n_again": wo_a["n_again"], "n_zero": wo_a["n_zero_port"],
            "offers": k_off, "n_over": w_off["n_over"], "closed": w_st["n_closed"], "purged": w_st["n_purged_ack"],
            "dead": w_fa["n_dead"] + w_fs["n_dead"], "taken": n_new}


GARBAGE = 0xA5A5A5A5  # no row of any table, and not the free entry: a lookup ends at it, a rebuild would replace it


def nothing_changes_case(lib, capacity=67):
    """add, settle and flush calls that change nothing write no byte of an index: pools without a LIVE row whose
    indexes hold garbage (which a rebuild would clear), and pools with LIVE rows and a built index."""
    rng = np.random.default_rng(capacity)
    uni = universe(rng, capacity + 16)
    for live in (0, capacity // 2):
        rows = np.arange(live) * 2
        ta = lib.table(filled(rng, capacity, rows, uni, 0, True))
        ts = lib.table(filled(rng, capacity, rows, uni, 0, False))
        if live == 0:
            for t in (ta, ts):
                t.index.fill_(int(np.array(GARBAGE, np.uint32).view(np.int32)))
        before = (ta.column("index").copy(), ts.column("index").copy())
        ca, cs = Lib.columns(ta), Lib.columns(ts)
        n = 130
        inp = {f: uni[f][rng.integers(live, live + 8, n)].copy() for f in ("src", "dst", "sp", "dp")}
        inp["seq"] = inp["ack"] = np.zeros(n, np.uint32)
        inp["sp"][::2] = 0  # a zero port, or no SYN: nothing is considered
        status = np.where(np.arange(n) % 2 == 0, A.PARSE_SYN, A.PARSE_DELIVER).astype(np.int8)
        o = lib.add(ta, inp, 5, n, True, status)
        assert o["n_new"] == 0 and o["n_zero_port"] == n // 2 and bool((o["row"] == NONE).all())
        if live:  # every tuple pooled already: touched, nothing added
            pooled = {f: uni[f][:live].copy() for f in ("src", "dst", "sp", "dp")}
            o = lib.add(ts, pooled, 5, live, False)
            assert o["n_new"] == 0 and o["n_again"] == live and o["row"].tolist() == rows.tolist()
        # a settle without new conns whose missing packets name whole offers, or nothing pooled
        pk = {f: uni[f][np.arange(n) % (live + 8)].copy() for f in ("src", "dst", "sp", "dp")}
        st = lib.settle(ta, ts, np.zeros(0, np.uint32), 0, np.zeros(0, np.uint32), np.zeros(0, np.uint32), np.full(n, A.RECV_VALID, np.int8), pk)
        assert st["n_closed"] == 0 and st["n_purged_ack"] == 0
        assert lib.flush(ta, 99)["n_dead"] == 0 and lib.flush(ts, 99)["n_dead"] == 0
        same_columns(ta, ca, "nothing changes")
        same_columns(ts, cs, "nothing changes")
        assert np.array_equal(ta.column("index"), before[0]) and np.array_equal(ts.column("index"), before[1]), \
            "a call that changed nothing wrote to an index"


# The cases tests/test_pool_host.py (twin against rule) and tests/test_gpu_pool.py (device against twin and rule) run:
# the full cross NS x CAPS x FILLS x KINDS, and the named edges.
NS = (0, 1, 63, 64, 65, 2047, 2048, 2049, 4097)
CAPS = (1, 2, 67, 1025)
FILLS = ("empty", "half", "full")
KINDS = ("same", "different", "mixed")
# name -> (arguments of property_case, the least each count must reach for the case to be the one it is named for)
CASES = {
    "u_max_below_the_considered_rows": (dict(n=2049, capacity=1025, fill="half", kind="mixed", u_short=True), {"n_new": 1}),
    "m_max_below_the_matches": (dict(n=65, capacity=1025, fill="half", kind="mixed", m_short=True), {"n_over": 1}),
    "n_new_of_zero": (dict(n=65, capacity=67, fill="half", kind="mixed", n_new_zero=True), {"offers": 2, "purged": 1}),
    "pool_full": (dict(n=2048, capacity=67, fill="full", kind="different"), {"n_full": 2048 - 128}),
    "every_packet_the_same_tuple": (dict(n=4097, capacity=1025, fill="empty", kind="same"), {"n_again": 4096, "n_new": 1}),
    "every_packet_different": (dict(n=4097, capacity=1025, fill="empty", kind="different"), {"n_new": 1025, "n_full": 2000}),
}
