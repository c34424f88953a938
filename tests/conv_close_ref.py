"""TEST INFRASTRUCTURE: rsk_conv_close_batch / rsk_conv_close_host (include/rsk_codec.h) restated with numpy
and a dict on top of tests/conv_ref.py and tests/conv_create_ref.py, the scenarios the CPU and GPU tests share
(side "cpu" = the host twin, a device = the kernels), and the driver that runs either side with every output
pre-filled with a sentinel.

The reference closes a conv from IGroup::Flush (conn/IGroup.cpp:81-107) and from ConnReset::OnRecvConvRst
inside the packet walk (callbacks/ConnReset.cpp:67-77), both through IGroup::CloseConn (conn/IGroup.cpp:126-137);
a DATA packet of the closed key then gets a new SConn (SubGroup::OnRecv -> newConn, server/SubGroup.cpp:31-68)."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import torch

from rsock_amd import _abi as A
from tests import control_golden as G
from tests import conv_create_ref as C
from tests import conv_ref as R

NONE, NO_RST, SENT, SENT32 = R.NONE, R.NO_RST, R.SENT, C.SENT32
VALID, DROP, LIVE = A.RECV_VALID, A.RECV_DROP, A.CONN_LIVE
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4097)
CAPACITIES = (1, 2, 1023, 1024, 1025, 4097, 65536)
OPTIONAL = ("unknown", "n_unknown", "closed_rows", "closed_at", "n_closed", "n_reopened", "n_rst_again")
FLUSH_CASES = G.names("flush")


# ---- the restatement -------------------------------------------------------------------------------------
def close_ref(state, hold=False, rst_first=None, ctl_kind=None, conv_row=None, unknown=None, n_unknown=0,
              close_rows=None, n_close=0, m_max=0):
    """-> dict(state = the column afterwards, lookup_state = the state whose rebuild gives the lookups afterwards,
    conv_row, unknown, n_unknown, closed_rows, closed_at, n_closed, n_reopened, n_rst_again)."""
    state = np.asarray(state, np.uint8)
    cap = len(state)
    if rst_first is None:
        mark = np.zeros(cap, bool)
        lst = np.asarray(close_rows, np.uint32)[:min(int(n_close), int(m_max))]
        mark[lst[lst < cap].astype(np.int64)] = True
        at = np.full(cap, NO_RST, np.uint32)
    else:
        at = np.asarray(rst_first, np.uint32)
        mark = at != NO_RST
    closed = mark & ((state & LIVE) != 0)
    rows = np.nonzero(closed)[0]
    lookup_state = state.copy()
    lookup_state[rows] &= np.uint8(0xFF ^ LIVE)
    o = {"state": state.copy() if hold else lookup_state, "lookup_state": lookup_state, "closed_rows": rows.astype(np.uint32),
         "closed_at": at[rows], "n_closed": len(rows), "n_reopened": 0, "n_rst_again": 0, "n_unknown": int(n_unknown)}
    if conv_row is not None:
        conv_row = np.array(conv_row, np.uint32)
        n = len(conv_row)
        inside = conv_row < cap
        rr = np.where(inside, conv_row, 0).astype(np.int64)
        tail = inside & closed[rr] & (np.arange(n, dtype=np.uint64) > at[rr])
        again = tail & (np.asarray(ctl_kind)[:n] == A.CTL_CONV_RST) if n else tail
        re = tail & ~again
        conv_row[tail] = NONE
        o.update(conv_row=conv_row, n_reopened=int(re.sum()), n_rst_again=int(again.sum()), n_unknown=int(n_unknown) + int(re.sum()),
                 tail=tail, reopened=re)
        if unknown is not None:
            unknown = np.array(unknown, np.int8)
            unknown[re] = VALID
            o["unknown"] = unknown
    return o


def walk_ref(cols, by_dst, by_id, c, server=True):
    """The reference's per-packet walk over a table: conv_ref.sequential_ref plus SubGroup::newConn.  A hitting
    CONV_RST deletes its key; a DATA packet of an absent key on a server makes a new leaf.  Leaves of the starting
    table are their rows, new ones count up from the capacity.  -> dict(leaf [n] (-1: routed nowhere), closes =
    [(leaf, packet)], reopened [n] bool: a DATA packet of a key that a reset closed earlier in the batch,
    exact: every hitting reset hit a leaf of the starting table)."""
    cap = len(cols["state"])
    tmap, _ = R.table_map(cols, by_dst, by_id)
    ex, rst, keys = R.packet_keys(c, by_dst, by_id)
    n = len(keys)
    leaf = np.full(n, -1, np.int64)
    reopened = np.zeros(n, bool)
    closes, closed_keys, nxt, exact = [], set(), cap, True
    for i, k in enumerate(keys):
        if k is None:
            continue
        if rst[i]:
            if k in tmap:
                leaf[i] = tmap.pop(k)
                closes.append((int(leaf[i]), i))
                closed_keys.add(k)
                exact &= leaf[i] < cap
        elif k in tmap:
            leaf[i] = tmap[k]
            reopened[i] = k in closed_keys
        elif server:
            tmap[k] = leaf[i] = nxt
            nxt += 1
            reopened[i] = k in closed_keys
    return {"leaf": leaf, "closes": closes, "reopened": reopened, "exact": bool(exact), "data": ex}


# ---- the driver ------------------------------------------------------------------------------------------
def run_close(rc, tab, device, codec=None, hold=False, rst_first=None, ctl_kind=None, conv_row=None, unknown=None,
              n_unknown=0, close_rows=None, n_close=None, m_max=None, work=None, want=OPTIONAL, stream=None, slack=3):
    """One close on `device` ("cpu": the host twin) from numpy inputs, with every output named in `want`
    pre-filled with SENT and `slack` spare entries behind each list and column: -> dict of numpy outputs,
    "tail_ok" and the lists whole ("closed_rows_all")."""
    cap = tab.capacity
    n = 0 if conv_row is None else len(conv_row)
    t = lambda a, dt: None if a is None else R.tensor(np.asarray(a, dt), device)  # noqa: E731
    o = {"closed_rows": R.filled(cap + slack, torch.int32, device), "closed_at": R.filled(cap + slack, torch.int32, device),
         "n_closed": R.filled(1, torch.int32, device), "n_reopened": R.filled(1, torch.int32, device),
         "n_rst_again": R.filled(1, torch.int32, device)}
    if conv_row is not None:
        o["conv_row"] = R.filled(n + slack, torch.int32, device)
        o["conv_row"][:n] = t(conv_row, np.uint32)
        if unknown is not None:
            o["unknown"] = R.filled(n + slack, torch.int8, device)
            o["unknown"][:n] = t(unknown, np.int8)
        o["n_unknown"] = t(np.array([n_unknown]), np.uint32)
    o = {k: (v if k in want or k == "conv_row" else None) for k, v in o.items()}
    kw = {k: (None if v is None else v[:n] if k in ("conv_row", "unknown") else v) for k, v in o.items()}
    if close_rows is not None:
        work = tab.close_work() if work is None else work
        kw.update(close_rows=t(close_rows, np.uint32), n_close=t(np.array([n_close]), np.uint32),
                  m_max=len(close_rows) if m_max is None else m_max, work=work)
    else:
        kw.update(rst_first=t(rst_first, np.uint32), ctl_kind=t(ctl_kind, np.uint8))
    if codec is None:
        rc.conv_close_host(tab, hold=hold, **kw)
    else:
        codec.conv_close_batch(tab, hold=hold, stream=stream, **kw)
        torch.cuda.synchronize()
    got, ok = {}, True
    for k in ("n_unknown", "n_closed", "n_reopened", "n_rst_again"):
        if o.get(k) is not None:
            got[k] = int(R.host(o[k], np.uint32)[0])
    for k in ("closed_rows", "closed_at"):
        if o[k] is not None:
            got[k + "_all"] = R.host(o[k], np.uint32)
    if o.get("conv_row") is not None:
        got["conv_row"] = R.host(o["conv_row"], np.uint32)[:n]
        ok &= bool((R.host(o["conv_row"], np.uint32)[n:] == SENT32).all())
    if o.get("unknown") is not None:
        got["unknown"] = R.host(o["unknown"], np.int8)[:n]
        ok &= bool((R.host(o["unknown"], np.uint8)[n:] == SENT).all())
    got["tail_ok"] = ok
    return got


def compare(got, want):
    assert got["tail_ok"]
    for k in ("conv_row", "unknown"):
        if k in got:
            assert np.array_equal(got[k], want[k]), k
    for k in ("n_unknown", "n_closed", "n_reopened", "n_rst_again"):
        if k in got:
            assert got[k] == want[k], (k, got[k], want[k])
    for k in ("closed_rows", "closed_at"):
        if k + "_all" in got:
            a = got[k + "_all"]
            assert np.array_equal(a[:want["n_closed"]], want[k]), k
            assert bool((a[want["n_closed"]:] == SENT32).all()), k + ": written past n_closed"


def check_lookups(rc, tab, cols, lookup_state, by_dst, by_id, device, codec=None):
    """The key of every row that is LIVE in `cols` resolves, on the index as it stands, to what a rebuild over
    `lookup_state` gives: the key's lowest row that stays, or unknown; the index itself is a build's over
    `lookup_state` (rsk_conn.h's contract; under HOLD it forgets rows that stay LIVE)."""
    R.check_index(tab, cols, by_dst, by_id, live=(lookup_state & LIVE) != 0, what="index as it stands")
    live = np.nonzero(cols["state"] & LIVE)[0]
    if len(live) == 0:
        return
    tmap, _ = R.table_map(dict(cols, state=lookup_state), by_dst, by_id)
    idw = R.id_words(cols["id"] if by_id else None, len(cols["state"]))
    want = np.array([tmap.get(R.row_key(cols, r, by_dst, by_id, idw), NONE) for r in live.tolist()], np.uint32)
    c = {"status": np.ones(len(live), np.int8), "cmd": None, "hit": None, "conv": cols["conv"][live],
         "dst": cols["dst"][live] if by_dst else None, "id": cols["id"].reshape(-1, 8)[live].ravel() if by_id else None,
         "ctl_kind": None, "ctl_arg": None}
    saved = None if tab.cur_in is None else tab.cur_in.clone()
    got = R.run_resolve(rc, tab, c, device, codec, want=("n_unknown",), msg_mode="none")
    if saved is not None:
        tab.cur_in.copy_(saved)
    assert np.array_equal(got["conv_row"], want) and got["n_unknown"] == int((want == NONE).sum())


def check_table(rc, tab, cols, ref, by_dst, by_id, device, codec=None, hold=False):
    """state as the restatement's, every other column bytewise `cols`', the lookups as a rebuild's -- on the index
    as left and (without HOLD, where a rebuild is the same thing) after a rebuild."""
    C.compare_table(tab, dict(cols, state=ref["state"]))
    check_lookups(rc, tab, cols, ref["lookup_state"], by_dst, by_id, device, codec)
    if not hold:
        tab.rebuild(codec)
        check_lookups(rc, tab, cols, ref["lookup_state"], by_dst, by_id, device, codec)


# ---- scenario 1: the reference's recorded IGroup::Flush -> CloseConn ---------------------------------------
def scenario_flush_golden(rc, name, device, codec=None):
    """control_golden.scenario_flush's rounds with the host's state edit + rebuild replaced by the close, fed by
    the flush's dead_rows / n_dead where they lie."""
    c = G.case("flush", name)
    server = int(c["shape"]) == G.SERVER
    nc = len(c["convs"])
    cap = nc + 3
    rng = np.random.default_rng(nc)
    cols = R.random_columns(rng, cap, by_dst=server, by_id=server)
    row = np.sort(rng.permutation(cap)[:nc]).astype(np.int64) if nc % 2 else rng.permutation(cap)[:nc].astype(np.int64)
    cols["conv"][row] = c["convs"]
    if server:
        cols["dst"][row] = G.DST
        cols["id"].reshape(-1, 8)[row] = np.ascontiguousarray(c["id"], np.uint8)
    cols["state"][row] = LIVE
    for k in R.COUNTERS:
        cols[k][:] = 0
    tab = R.make_table(rc, cols, device, server, server, codec)
    leaf_of_row = np.full(cap, -1, np.int64)
    leaf_of_row[row] = np.arange(nc)
    work = tab.close_work()
    gone = np.zeros(nc, bool)
    closed_total = 0

    def batch(leaf):
        k = len(leaf)
        return {"status": np.ones(k, np.int8), "cmd": np.zeros(k, np.uint8), "conv": c["convs"][leaf],
                "id": np.tile(np.ascontiguousarray(c["id"], np.uint8), k) if server else None,
                "dst": np.full(k, G.DST, np.uint32) if server else None, "hit": None, "ctl_kind": None, "ctl_arg": None}

    for r in range(len(c["now"])):
        lo, hi = int(c["in_off"][r]), int(c["in_off"][r + 1])
        if hi > lo:
            leaf = c["in_leaf"][lo:hi].astype(np.int64)
            got = R.run_resolve(rc, tab, batch(leaf), device, codec, msg_mode="count")
            assert got["tail_ok"] and np.array_equal(got["conv_row"], row[leaf].astype(np.uint32)) and got["n_unknown"] == 0
        lo, hi = int(c["out_off"][r]), int(c["out_off"][r + 1])
        if hi > lo:
            R.run_send(rc, tab, row[c["out_leaf"][lo:hi].astype(np.int64)].astype(np.uint32), device, codec,
                       sent=c["out_ret"][lo:hi].astype(np.int32), cols=())
        dead, n_dead = R.filled(cap, torch.int32, device), R.filled(1, torch.int32, device)
        o = {"closed_rows": R.filled(cap + 2, torch.int32, device), "closed_at": R.filled(cap + 2, torch.int32, device),
             "n_closed": R.filled(1, torch.int32, device)}
        if codec is None:
            rc.conv_flush_host(tab, dead_rows=dead, n_dead=n_dead)
            rc.conv_close_host(tab, close_rows=dead, n_close=n_dead, work=work, **o)
        else:  # flush -> close, one device chain: nothing is read in between
            codec.conv_flush(tab, dead_rows=dead, n_dead=n_dead)
            codec.conv_close_batch(tab, close_rows=dead, n_close=n_dead, work=work, **o)
            torch.cuda.synchronize()
        closed = c["cl_leaf"][c["cl_round"] == r].astype(np.int64)
        k = int(R.host(o["n_closed"], np.uint32)[0])
        rows_closed = R.host(o["closed_rows"], np.uint32)
        assert k == len(closed) == int(R.host(n_dead, np.uint32)[0])
        assert np.array_equal(rows_closed[:k], R.host(dead, np.uint32)[:k]) and bool((rows_closed[k:] == SENT32).all())
        assert bool((R.host(o["closed_at"], np.uint32)[:k] == NO_RST).all())
        assert sorted(leaf_of_row[rows_closed[:k].astype(np.int64)].tolist()) == sorted(closed.tolist()), r
        gone[closed] = True
        alive = c["alive"][r]
        there = alive >= 0
        assert not there[closed].any()
        assert np.array_equal(tab.column("alive")[row[there]], alive[there].astype(np.uint8)), r
        for j, name_ in enumerate(("cur_in", "cur_out", "prev_in", "prev_out")):
            assert np.array_equal(tab.column(name_)[row[there]], c["counters"][r][there, j]), (r, name_)
        assert np.array_equal((tab.column("state")[row] & LIVE) != 0, ~gone), r
        closed_total += k
        if k:  # every closed conv is unknown now, every surviving one keeps its row
            saved = tab.cur_in.clone()
            got = R.run_resolve(rc, tab, batch(np.arange(nc)), device, codec, msg_mode="none")
            tab.cur_in.copy_(saved)
            assert np.array_equal(got["conv_row"], np.where(gone, NONE, row).astype(np.uint32)), r
            assert np.array_equal(got["unknown"] == VALID, gone), r
    return {"closed": closed_total}


# ---- scenario 2: timer form, random ------------------------------------------------------------------------
def scenario_timer_random(rc, capacity, by_dst, by_id, device, codec=None):
    rng = np.random.default_rng(7000 + capacity + 7 * by_dst + 13 * by_id)
    cols, _c = R.random_case(rng, 1, capacity, by_dst, by_id, live=0.7, pool=min(capacity, 300))
    m = 2 * capacity + 5
    lst = rng.integers(0, capacity, m).astype(np.uint32)  # repeats, LIVE and not
    odd = rng.random(m) < 0.1
    lst[odd] = rng.choice(np.array([capacity, capacity + 1, 2**31, NONE], np.uint32), int(odd.sum()))
    for n_close, m_max in ((m, m), (max(1, capacity // 3), m), (m + 100, max(1, capacity // 2)), (0, m), (5, 0), (1, 1)):
        tab = R.make_table(rc, cols, device, by_dst, by_id, codec)
        ref = close_ref(cols["state"], close_rows=lst, n_close=n_close, m_max=m_max)
        got = run_close(rc, tab, device, codec, close_rows=lst, n_close=n_close, m_max=m_max)
        compare(got, ref)
        assert got["n_reopened"] == 0 and got["n_rst_again"] == 0
        assert bool((got["closed_at_all"][:ref["n_closed"]] == NO_RST).all())
        check_table(rc, tab, cols, ref, by_dst, by_id, device, codec)


# ---- scenario 3: receive form against the per-packet walk ------------------------------------------------
IDS = np.array([[1, 2, 3, 4, 5, 6, 7, 8], [1, 2, 3, 4, 5, 6, 7, 9], [129, 2, 3, 4, 5, 6, 7, 8]], np.uint8)
DSTS = np.array([0x0A000001, 0x8A000001, 0x0A000003], np.uint32)


def key_universe(rng, count, by_id=True):
    """`count` distinct keys: distinct convs that differ in few bits, dst and IdBuf from small sets."""
    conv = (rng.permutation(1 << 21)[:count].astype(np.uint32) << np.uint32(3)) | np.uint32(1)
    return {"conv": conv, "dst": DSTS[rng.integers(0, len(DSTS), count)],
            "id": IDS[rng.integers(0, len(IDS), count)] if by_id else None}


def packets(rng, keys, pick, is_rst, by_id=True, noise=0.0):
    """A batch: packet i names key pick[i], as a DATA packet or (is_rst) as a CONV_RST whose body holds the conv;
    `noise`: the share of packets turned into dropped or other control packets."""
    n = len(pick)
    is_rst = np.asarray(is_rst, bool)
    junk = rng.integers(0, 2**32, n, dtype=np.uint64)
    kc = keys["conv"][pick]
    c = {"status": np.ones(n, np.int8), "cmd": np.where(is_rst, A.CMD_CONV_RST, A.CMD_DATA).astype(np.uint8),
         "conv": np.where(is_rst, junk.astype(np.uint32), kc), "dst": keys["dst"][pick].copy(),
         "id": keys["id"][pick].ravel().copy() if by_id else None, "hit": None,
         "ctl_kind": np.where(is_rst, A.CTL_CONV_RST, A.CTL_NONE).astype(np.uint8),
         "ctl_arg": np.where(is_rst, kc.astype(np.uint64) | ((junk & np.uint64(1)) << np.uint64(40)), junk)}
    if noise:
        x = rng.random(n)
        c["status"][x < noise / 2] = DROP
        ka = (x >= noise / 2) & (x < noise) & ~is_rst
        c["cmd"][ka], c["ctl_kind"][ka] = A.CMD_KEEP_ALIVE_REQ, A.CTL_KA_REQ
        c["ctl_kind"][c["status"] != VALID] = A.CTL_NONE
    return c


def table_of(rng, keys, capacity, live_rows, by_id=True):
    """Rows 0 .. capacity-1 hold keys 0 .. capacity-1; `live_rows` are LIVE; the other state bits are random."""
    cols = R.random_columns(rng, capacity, True, by_id)
    cols["conv"][:], cols["dst"][:] = keys["conv"][:capacity], keys["dst"][:capacity]
    if by_id:
        cols["id"][:] = keys["id"][:capacity].ravel()
    cols["state"][:] = rng.integers(0, 2, capacity).astype(np.uint8) << 1
    cols["state"][live_rows] |= LIVE
    return cols


def recv_case(rng, n, capacity, by_id=True, live=0.6, resets=0.3, double=0.3, noise=0.1):
    """A server table and a batch whose resets hit only leaves of the starting table, each key once; some are
    followed at once by a second reset of the key (which finds nothing), most by DATA packets (a reborn conv).
    New keys (DATA only) and ghost keys (CONV_RST only) fill the rest; the convs born fit the vacant rows."""
    keys = key_universe(rng, capacity + 64, by_id)
    live_rows = np.nonzero(rng.random(capacity) < live)[0]
    cols = table_of(rng, keys, capacity, live_rows, by_id)
    vacant = capacity - len(live_rows)
    pool = rng.permutation(live_rows)[:300]
    n_rst = min(int(len(pool) * resets + 0.5), vacant // 2)
    n_new = min(40, vacant - n_rst)
    rst_keys = pool[:n_rst]
    cand = np.concatenate([pool, capacity + np.arange(n_new), capacity + 40 + np.arange(8)]).astype(np.int64)
    pick = cand[rng.integers(0, len(cand), n)]
    is_rst = pick >= capacity + 40
    for k in rst_keys.tolist():
        at = np.nonzero(pick == k)[0]
        if len(at):
            j = int(rng.integers(0, len(at)))
            is_rst[at[j]] = True
            if j + 1 < len(at) and rng.random() < double:
                is_rst[at[j + 1]] = True
    return cols, packets(rng, keys, pick, is_rst, by_id, noise)


def run_chain(rc, cols, c, by_id, device, codec=None, hold=True):
    """resolve -> create (u_max = n) -> close -> create on a fresh table: -> dict(tab, res, cr1, cl, cr2, ref = the
    close's restatement)."""
    n = len(c["status"])
    tab = R.make_table(rc, cols, device, True, by_id, codec)
    res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
    R.compare(res, R.resolve_ref(cols, True, by_id, c))
    b = C.Batch(c, res["conv_row"], res["unknown"], device)
    cr1 = C.run_create(rc, tab, b, max(n, 1), codec)
    state1 = tab.column("state").copy()
    ref = close_ref(state1, hold, res["rst_first"], c["ctl_kind"], cr1["conv_row"], cr1["unknown"], cr1["n_unknown"])
    cl = run_close(rc, tab, device, codec, hold=hold, rst_first=res["rst_first"], ctl_kind=c["ctl_kind"],
                   conv_row=cr1["conv_row"], unknown=cr1["unknown"], n_unknown=cr1["n_unknown"])
    compare(cl, ref)
    assert np.array_equal(tab.column("state"), ref["state"])
    b = C.Batch(c, cl["conv_row"], cl["unknown"], device)
    cr2 = C.run_create(rc, tab, b, max(n, 1), codec)
    return {"tab": tab, "res": res, "cr1": cr1, "cl": cl, "cr2": cr2, "ref": ref}


def check_against_walk(cols, c, by_id, out, upto_first=False):
    """The chain's conv_row against walk_ref.  upto_first: only the packets up to their row's first reset (the
    specified deviations lie behind it) and the closes' rows."""
    cap = len(cols["state"])
    w = walk_ref(cols, True, by_id, c)
    row, leaf = out["cr2"]["conv_row"], w["leaf"]
    if upto_first:
        res_row = out["res"]["conv_row"]
        inside = res_row < cap
        at = np.where(inside, out["res"]["rst_first"][np.where(inside, res_row, 0).astype(np.int64)], NO_RST)
        sel = ~inside | (np.arange(len(row)) <= at)
        rstp = (c["ctl_kind"] == A.CTL_CONV_RST) & ~w["data"]
        sel &= ~(rstp & (leaf >= cap))  # a reset that hit a conv born in the batch: a deviation too
        row, leaf = row[sel], leaf[sel]
    else:
        assert w["exact"]
        assert out["cr2"]["n_unknown"] == 0 and out["cr2"]["n_full"] == 0
    assert np.array_equal(row == NONE, leaf < 0)
    on = leaf >= 0
    pairs = np.unique(np.stack([row[on].astype(np.int64), leaf[on]], axis=1), axis=0)
    assert len(pairs) == len(np.unique(pairs[:, 0])) == len(np.unique(pairs[:, 1]))  # conv_row <-> leaf is a bijection
    if upto_first:
        return w
    closes = sorted(w["closes"])
    cl = out["cl"]
    assert cl["n_closed"] == len(closes)
    assert cl["closed_rows_all"][:len(closes)].tolist() == [r for r, _ in closes]
    assert cl["closed_at_all"][:len(closes)].tolist() == [i for _, i in closes]
    assert cl["n_reopened"] == int(w["reopened"].sum())
    # cur_in of every row that was not closed: its start value (0 for a row born in the batch) + its leaf's DATA packets
    cur = out["tab"].column("cur_in")
    per_leaf = np.bincount(leaf[on & w["data"]], minlength=1)
    closed = set(r for r, _ in closes)
    seen = np.zeros(cap, bool)
    for r, lf in pairs.tolist():
        seen[r] = True
        if r in closed:
            continue
        start = int(cols["cur_in"][r]) if lf < cap else 0
        assert int(cur[r]) == (start + (int(per_leaf[lf]) if lf < len(per_leaf) else 0)) & 0xFFFFFFFF, (r, lf)
    quiet = ~seen
    quiet[list(closed)] = False
    born = np.zeros(cap, bool)
    for o in (out["cr1"], out["cr2"]):
        born[o["new_rows_all"][:o["n_new"]].astype(np.int64)] = True
    assert np.array_equal(cur[quiet & ~born], cols["cur_in"][quiet & ~born])
    return w


def scenario_walk(rc, n, capacity, by_id, device, codec=None, **kw):
    rng = np.random.default_rng(3000 * n + capacity + 13 * by_id)
    cols, c = recv_case(rng, n, capacity, by_id, **kw)
    out = run_chain(rc, cols, c, by_id, device, codec)
    w = check_against_walk(cols, c, by_id, out)
    # the key columns, alive and the counters of the closed rows: bytewise the resolve's
    rows = out["cl"]["closed_rows_all"][:out["cl"]["n_closed"]].astype(np.int64)
    for k in ("conv", "dst", "id", "alive", "cur_out", "prev_in", "prev_out"):
        if cols.get(k) is not None:
            w_ = 8 if k == "id" else 1
            assert np.array_equal(out["tab"].column(k).reshape(-1, w_)[rows], cols[k].reshape(-1, w_)[rows]), k
    return out, w


def scenario_walk_golden(rc, name, seed, device, codec=None):
    """The golden server inputs of demux.npz: the table starts with the convs of half of the batch's keys, and
    resets are injected on a third of those, one per key."""
    g, c, _cols, _k = C.golden_server(name)
    n = len(g["status"])
    rng = np.random.default_rng(seed)
    data = (g["status"] == VALID) & (g["cmd"] == A.CMD_DATA)
    first = R.first_arrivals(c, np.where(data, VALID, DROP))
    start = first[rng.random(len(first)) < 0.5]
    cap = len(first) + len(start) + 7  # under HOLD every reborn conv takes a row of its own
    cols = R.random_columns(rng, cap)
    rows = np.sort(rng.permutation(cap)[:len(start)])
    cols["conv"][rows], cols["dst"][rows] = g["conv"][start], g["dst"][start]
    cols["id"].reshape(-1, 8)[rows] = g["id"].reshape(n, 8)[start]
    cols["state"][rows] = LIVE
    c = dict(c, cmd=g["cmd"].copy(), conv=g["conv"].copy(), ctl_kind=np.full(n, A.CTL_NONE, np.uint8),
             ctl_arg=rng.integers(0, 2**63, n, dtype=np.uint64))
    _ex, _rst, keys = R.packet_keys(c, True, True)
    injected = 0
    for f in start[rng.random(len(start)) < 0.34].tolist():
        mine = [i for i in np.nonzero(data)[0].tolist() if keys[i] == keys[f]]
        i = mine[int(rng.integers(0, len(mine)))]
        c["cmd"][i], c["ctl_kind"][i], c["ctl_arg"][i] = A.CMD_CONV_RST, A.CTL_CONV_RST, int(g["conv"][i]) | (1 << 40)
        c["conv"][i] ^= np.uint32(0x5A5A5A5A)
        injected += 1
    out = run_chain(rc, cols, c, True, device, codec)
    check_against_walk(cols, c, True, out)
    assert out["cl"]["n_closed"] == injected
    return out


# ---- scenario 4: the deviations as specified -----------------------------------------------------------------
def scenario_deviations(rc, device, codec=None):
    rng = np.random.default_rng(401)
    cap, n = 40, 3000
    keys = key_universe(rng, cap + 8)
    cols = table_of(rng, keys, cap, np.arange(20))
    pick = rng.integers(0, 12, n)
    is_rst = np.zeros(n, bool)
    for k in range(10):  # rows 0..9: a second reset; even rows with DATA between the two, odd rows without
        at = np.nonzero(pick == k)[0]
        j = len(at) // 3
        is_rst[at[j]] = True
        is_rst[at[j + 1] if k % 2 else at[j + 5]] = True
    # a conv born in the batch (key cap + 1 is in no row) that a later reset names
    pick[100], pick[2000] = cap + 1, cap + 1
    is_rst[100], is_rst[2000] = False, True
    c = packets(rng, keys, pick, is_rst)
    out = run_chain(rc, cols, c, True, device, codec)
    w = check_against_walk(cols, c, True, out, upto_first=True)
    assert not w["exact"]
    cl, ref = out["cl"], out["ref"]
    assert cl["n_closed"] == 10 and cl["closed_rows_all"][:10].tolist() == list(range(10))
    assert cl["n_rst_again"] == ref["n_rst_again"] == 10 and cl["n_reopened"] == ref["n_reopened"] > 100
    # the reset on the conv born in the batch keeps NONE, and the conv stays
    assert out["cr2"]["conv_row"][2000] == NONE and out["cr2"]["conv_row"][100] != NONE
    assert out["cr2"]["conv_row"][100] == out["cr2"]["conv_row"][np.nonzero((pick == cap + 1) & ~is_rst)[0][-1]]


# ---- scenario 5: HOLD against not HOLD -----------------------------------------------------------------------
def scenario_hold(rc, device, codec=None):
    rng = np.random.default_rng(501)
    cap, n = 300, 4097
    keys = key_universe(rng, cap + 64)
    cols = table_of(rng, keys, cap, np.arange(cap))  # a full table: the closed rows are the only vacant ones
    pick = rng.integers(0, cap, n)
    is_rst = np.zeros(n, bool)
    rstk = rng.permutation(cap)[:25]
    for k in rstk.tolist():
        is_rst[np.nonzero(pick == k)[0][-1]] = True  # the key's last packet: nothing is reopened
    c = packets(rng, keys, pick, is_rst)
    newc = packets(rng, keys, cap + rng.integers(0, 60, 500), np.zeros(500, bool))
    outs = {}
    for hold in (False, True):
        tab = R.make_table(rc, cols, device, True, True, codec)
        res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
        cols1 = dict(cols, cur_in=tab.column("cur_in").copy())
        ref = close_ref(cols["state"], hold, res["rst_first"], c["ctl_kind"], res["conv_row"], res["unknown"], res["n_unknown"])
        got = run_close(rc, tab, device, codec, hold=hold, rst_first=res["rst_first"], ctl_kind=c["ctl_kind"],
                        conv_row=res["conv_row"], unknown=res["unknown"], n_unknown=res["n_unknown"])
        compare(got, ref)
        assert got["n_closed"] == 25 and got["n_reopened"] == 0
        check_table(rc, tab, cols1, ref, True, True, device, codec, hold=hold)
        state = tab.column("state").copy()
        res2 = R.run_resolve(rc, tab, newc, device, codec, msg_mode="none")
        assert res2["n_unknown"] == 500
        cr = C.run_create(rc, tab, C.Batch(newc, res2["conv_row"], res2["unknown"], device), 500, codec)
        outs[hold] = (got, state, cr)
    (g0, s0, c0), (g1, s1, c1) = outs[False], outs[True]
    closed = np.sort(rstk)
    assert np.array_equal(g0["closed_rows_all"], g1["closed_rows_all"]) and np.array_equal(g0["closed_rows_all"][:25], closed)
    assert np.array_equal(np.nonzero(s0 != s1)[0], closed) and bool(((s1[closed] & LIVE) != 0).all())
    assert np.array_equal(g0["conv_row"], g1["conv_row"])
    # the create behind the plain call reuses the closed rows; behind HOLD it finds no vacant row
    assert c0["n_new"] == 25 and np.array_equal(c0["new_rows_all"][:25], closed) and c0["n_full"] == 60 - 25
    assert c1["n_new"] == 0 and c1["n_full"] == 60 and c1["n_unknown"] == 500


# ---- scenario 6: nothing to close ------------------------------------------------------------------------------
def scenario_nothing(rc, device, codec=None):
    rng = np.random.default_rng(601)
    for by_dst, by_id, n, cap in ((True, True, 4097, 1025), (False, False, 2049, 300), (True, False, 65, 2)):
        cols, c = R.random_case(rng, n, cap, by_dst, by_id, known=0.7, pool=min(cap, 100))
        if by_dst:  # no reset hits: every CONV_RST names a conv that no row holds
            rstp = c["ctl_kind"] == A.CTL_CONV_RST
            c["dst"][rstp] = 0x01020304
        tab = R.make_table(rc, cols, device, by_dst, by_id, codec)
        res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
        assert bool((res["rst_first"] == NO_RST).all()) and (c["ctl_kind"] == A.CTL_CONV_RST).sum() > 2
        before, index = C.table_columns(tab), tab.index.clone()
        for hold in (False, True):
            got = run_close(rc, tab, device, codec, hold=hold, rst_first=res["rst_first"], ctl_kind=c["ctl_kind"],
                            conv_row=res["conv_row"], unknown=res["unknown"], n_unknown=res["n_unknown"])
            assert got["tail_ok"] and got["n_closed"] == got["n_reopened"] == got["n_rst_again"] == 0
            assert got["n_unknown"] == res["n_unknown"]
            assert np.array_equal(got["conv_row"], res["conv_row"]) and np.array_equal(got["unknown"], res["unknown"])
            assert bool((got["closed_rows_all"] == SENT32).all()) and bool((got["closed_at_all"] == SENT32).all())
        lst = rng.integers(0, cap, cap).astype(np.uint32)
        notlive = np.nonzero((cols["state"] & LIVE) == 0)[0].astype(np.uint32)
        for rows_, n_close in ((lst, 0), (notlive if len(notlive) else lst, len(notlive))):
            got = run_close(rc, tab, device, codec, close_rows=rows_, n_close=n_close)
            assert got["n_closed"] == 0 and bool((got["closed_rows_all"] == SENT32).all())
        C.compare_table(tab, before)
        assert bool((tab.index == index).all()), "the index was written"


# ---- scenario 7: skew ---------------------------------------------------------------------------------------------
def scenario_skew(rc, kind, device, codec=None):
    rng = np.random.default_rng(701)
    if kind == "one_conv":  # 4097 packets on one conv, its reset in the middle
        cap, n = 300, 4097
        keys = key_universe(rng, cap + 8)
        cols = table_of(rng, keys, cap, np.arange(0, cap, 2))
        pick, is_rst = np.full(n, 116), np.zeros(n, bool)
        is_rst[2048] = True
    elif kind == "every_row":  # every row of a 1025-row table reset once; nothing behind the resets
        cap = 1025
        keys = key_universe(rng, cap + 8)
        cols = table_of(rng, keys, cap, np.arange(cap))
        pick = np.concatenate([rng.integers(0, cap, 3000), rng.permutation(cap)])
        n = len(pick)
        is_rst = np.arange(n) >= 3000
    else:  # edges: a reset at packet 0 and one at packet n - 1
        cap, n = 64, 2049
        keys = key_universe(rng, cap + 8)
        cols = table_of(rng, keys, cap, np.arange(32))
        pick, is_rst = rng.integers(2, 32, n), np.zeros(n, bool)
        pick[0], pick[n - 1], pick[5], pick[700] = 0, 1, 0, 1
        is_rst[0] = is_rst[n - 1] = True
    c = packets(rng, keys, pick, is_rst)
    out = run_chain(rc, cols, c, True, device, codec)
    check_against_walk(cols, c, True, out)
    cl = out["cl"]
    if kind == "one_conv":
        assert cl["n_closed"] == 1 and cl["closed_at_all"][0] == 2048 and cl["n_reopened"] == 2048
        assert out["cr2"]["n_new"] == 1 and len(np.unique(out["cr2"]["conv_row"][2049:])) == 1
    elif kind == "every_row":
        assert cl["n_closed"] == cap and cl["n_reopened"] == 0
        check_lookups(rc, out["tab"], cols, out["ref"]["lookup_state"], True, True, device, codec)  # every key is gone
    else:
        assert cl["closed_rows_all"][:2].tolist() == [0, 1] and cl["closed_at_all"][:2].tolist() == [0, n - 1]
        assert cl["n_reopened"] == 1 and out["cr2"]["conv_row"][5] not in (0, NONE) and out["cr2"]["conv_row"][700] == 1


# ---- scenario 8: reads ----------------------------------------------------------------------------------------
def scenario_reads(rc, device, codec=None):
    rng = np.random.default_rng(801)
    cols, c = recv_case(rng, 4097, 1025, noise=0.1)
    tab = R.make_table(rc, cols, device, True, True, codec)
    res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
    ref = close_ref(cols["state"], False, res["rst_first"], c["ctl_kind"], res["conv_row"], res["unknown"], res["n_unknown"])
    assert ref["n_reopened"] > 100 and ref["n_rst_again"] > 2
    inside = res["conv_row"] < len(cols["state"])
    on_closed = inside & np.isin(res["conv_row"], ref["closed_rows"])
    for poison in (None, A.CTL_CONV_RST, 0, 0xFF):
        kind = c["ctl_kind"].copy()
        if poison is not None:
            kind[~on_closed] = poison
        tab = R.make_table(rc, cols, device, True, True, codec)
        tab.load(cur_in=cols["cur_in"])
        got = run_close(rc, tab, device, codec, rst_first=res["rst_first"], ctl_kind=kind, conv_row=res["conv_row"],
                        unknown=res["unknown"], n_unknown=res["n_unknown"])
        compare(got, ref)
        check_table(rc, tab, cols, ref, True, True, device, codec)
    # timer form: the entries of close_rows behind min(*n_close, m_max) name LIVE rows and close nothing
    live = np.nonzero(cols["state"] & LIVE)[0].astype(np.uint32)
    for n_close, m_max in ((7, len(live)), (len(live), 7)):
        tab = R.make_table(rc, cols, device, True, True, codec)
        got = run_close(rc, tab, device, codec, close_rows=live, n_close=n_close, m_max=m_max)
        ref = close_ref(cols["state"], close_rows=live[:7], n_close=7, m_max=7)
        compare(got, ref)
        assert got["n_closed"] == 7
        check_table(rc, tab, cols, ref, True, True, device, codec)


# ---- scenario 9: optional outputs ---------------------------------------------------------------------------------
def scenario_optional_outputs(rc, device, codec=None):
    rng = np.random.default_rng(901)
    cols, c = recv_case(rng, 2049, 300)
    tab = R.make_table(rc, cols, device, True, True, codec)
    res = R.run_resolve(rc, tab, c, device, codec, msg_mode="none")
    cols = dict(cols, cur_in=tab.column("cur_in").copy())
    ref = close_ref(cols["state"], False, res["rst_first"], c["ctl_kind"], res["conv_row"], res["unknown"], res["n_unknown"])
    assert ref["n_closed"] > 5 and ref["n_reopened"] > 50
    dead = np.nonzero(cols["state"] & LIVE)[0][::3].astype(np.uint32)
    tref = close_ref(cols["state"], close_rows=dead, n_close=len(dead), m_max=len(dead))
    for k in range(len(OPTIONAL) + 1):
        for want in itertools.combinations(OPTIONAL, k):
            if ("closed_rows" in want or "closed_at" in want) and "n_closed" not in want:
                continue  # RSK_EINVAL (check_einval)
            tab = R.make_table(rc, cols, device, True, True, codec)
            got = run_close(rc, tab, device, codec, rst_first=res["rst_first"], ctl_kind=c["ctl_kind"],
                            conv_row=res["conv_row"], unknown=res["unknown"] if "unknown" in want else None,
                            n_unknown=res["n_unknown"], want=want)
            compare(got, ref)
            check_table(rc, tab, cols, ref, True, True, device, codec)
            if "unknown" in want:
                continue  # the timer form has no packet columns
            tab = R.make_table(rc, cols, device, True, True, codec)
            got = run_close(rc, tab, device, codec, close_rows=dead, n_close=len(dead), want=want)
            compare(got, dict(tref, n_unknown=got.get("n_unknown")))
            C.compare_table(tab, dict(cols, state=tref["state"]))
    # a table without the counter columns
    tab = C.make_table(rc, cols, device, True, True, codec, absent=C.COUNTER_COLS)
    got = run_close(rc, tab, device, codec, rst_first=res["rst_first"], ctl_kind=c["ctl_kind"], conv_row=res["conv_row"],
                    unknown=res["unknown"], n_unknown=res["n_unknown"])
    compare(got, ref)
    # n == 0 in the receive form: the marked rows close, no packet column is looked at
    tab = R.make_table(rc, cols, device, True, True, codec)
    got = run_close(rc, tab, device, codec, rst_first=res["rst_first"], want=("closed_rows", "closed_at", "n_closed", "n_reopened"))
    assert got["n_closed"] == ref["n_closed"] and got["n_reopened"] == 0
    assert np.array_equal(got["closed_rows_all"][:ref["n_closed"]], ref["closed_rows"])
    check_table(rc, tab, cols, ref, True, True, device, codec)


# ---- scenario 10: arguments -----------------------------------------------------------------------------------------
def check_einval(rc, device, codec=None):
    """Every RSK_EINVAL of the close, with the outputs and the table untouched by a rejected call."""
    L = rc.lib()
    tabs, a, n = R.einval_fixture(rc, device, codec)
    server, client = tabs[(True, True)], tabs[(False, False)]
    ctx = () if codec is None else (codec._ctx,)
    tail = (1,) if codec is None else (None,)
    fn = L.rsk_conv_close_host if codec is None else L.rsk_conv_close_batch
    ref = lambda s: ctypes.byref(s) if s is not None else None  # noqa: E731
    p = lambda k: a[k].data_ptr()  # noqa: E731
    unk = R.tensor(np.full(n, DROP, np.int8), device)
    rst = R.tensor(np.full(4, NO_RST, np.uint32), device)
    lst = R.tensor(np.array([3, 0, 2, 2], np.uint32), device)  # rows that are not LIVE
    ncl = R.tensor(np.array([4], np.uint32), device)
    work = server.close_work()
    lists = R.filled(16, torch.int32, device)

    def cin(form, **kw):
        d = dict(close_rows=None, n_close=None, m_max=0, rst_first=None, ctl_kind=None, work=None, flags=0)
        if form == "timer":
            d.update(close_rows=lst.data_ptr(), n_close=ncl.data_ptr(), m_max=4, work=work.data_ptr())
        else:
            d.update(rst_first=rst.data_ptr(), ctl_kind=p("kind"))
        d.update(kw)
        return A.ConvCloseIn(*[d[f] for f, _ in A.ConvCloseIn._fields_])

    def cout(**kw):
        d = dict(conv_row=p("row"), unknown=unk.data_ptr(), n_unknown=None, closed_rows=lists.data_ptr(),
                 closed_at=lists.data_ptr() + 32, n_closed=p("cnt"), n_reopened=None, n_rst_again=None)
        d.update(kw)
        return A.ConvCloseOut(*[d[f] for f, _ in A.ConvCloseOut._fields_])

    S, SR, E = server.abi, server.abi_rows, A.EINVAL
    cases = [("null tab", None, SR(), n, cin("recv"), cout()), ("null rows", S(), None, n, cin("recv"), cout()),
             ("null in", S(), SR(), n, None, cout()), ("null out", S(), SR(), n, cin("recv"), None),
             ("both forms", S(), SR(), 0, cin("timer", rst_first=rst.data_ptr()), cout()),
             ("neither form", S(), SR(), n, cin("recv", rst_first=None), cout()),
             ("unknown flags", S(), SR(), n, cin("recv", flags=2), cout()),
             ("timer: no work", S(), SR(), 0, cin("timer", work=None), cout()),
             ("timer: no n_close", S(), SR(), 0, cin("timer", n_close=None), cout()),
             ("timer: n != 0", S(), SR(), n, cin("timer"), cout()),
             ("timer: HOLD", S(), SR(), 0, cin("timer", flags=A.CONV_CLOSE_HOLD), cout()),
             ("timer: ctl_kind", S(), SR(), 0, cin("timer", ctl_kind=p("kind")), cout()),
             ("timer: work misaligned", S(), SR(), 0, cin("timer", work=work.data_ptr() + 8), cout()),
             ("recv: n_close", S(), SR(), n, cin("recv", n_close=ncl.data_ptr()), cout()),
             ("recv: no ctl_kind", S(), SR(), n, cin("recv", ctl_kind=None), cout()),
             ("recv: no conv_row", S(), SR(), n, cin("recv"), cout(conv_row=None)),
             ("closed_rows without n_closed", S(), SR(), n, cin("recv"), cout(n_closed=None)),
             ("closed_at without n_closed", S(), SR(), n, cin("recv"), cout(n_closed=None, closed_rows=None)),
             ("n too large", S(), SR(), A.MAX_BATCH + 1, cin("recv"), cout())]
    for field, val in (("flags", 4), ("flags", 0x80000003), ("capacity", 0), ("capacity", A.CONN_MAX_ROWS + 1),
                       ("state", None), ("conv", None), ("index", None), ("dst", None), ("id", None)):
        t = S()
        setattr(t, field, val)
        cases.append((f"tab.{field}={val}", t, SR(), n, cin("recv"), cout()))
    for field in ("state", "conv", "dst", "id"):
        r = SR()
        setattr(r, field, getattr(client.abi(), "conv"))
        cases.append((f"rows.{field} not the table's", S(), r, n, cin("recv"), cout()))
        r = SR()
        setattr(r, field, None)
        cases.append((f"rows.{field} NULL", S(), r, n, cin("recv"), cout()))
    t = S()
    t.index += 4
    cases.append(("tab.index misaligned", t, SR(), n, cin("recv"), cout()))
    t, r = S(), SR()
    t.id += 4
    r.id += 4
    cases.append(("tab.id misaligned", t, r, n, cin("recv"), cout()))
    before, index = C.table_columns(server), server.index.clone()

    def untouched():
        if codec is not None:
            torch.cuda.synchronize()
        return (all(bool((x.cpu().view(torch.uint8) == SENT).all()) for x in (a["row"], a["cnt"], lists))
                and bool((unk.cpu() == DROP).all()))

    for label, t, r, nn, i, o in cases:
        if codec is None and "id misaligned" in label:  # the host twin reads ids bytewise
            continue
        assert fn(*ctx, ref(t), ref(r), nn, ref(i), ref(o), *tail) == E, label
        assert untouched(), label
    if codec is not None:
        assert L.rsk_conv_close_batch(None, ref(S()), ref(SR()), n, ref(cin("recv")), ref(cout()), None) == E
    C.compare_table(server, before)
    # the valid calls do run, and close nothing here: a client's rows need no dst / id
    crow = A.ConvRows(client.state.data_ptr(), client.conv.data_ptr(), None, None)
    assert fn(*ctx, ref(client.abi()), ref(crow), n, ref(cin("recv")), ref(cout()), *tail) == A.OK
    assert fn(*ctx, ref(S()), ref(SR()), n, ref(cin("recv", flags=A.CONV_CLOSE_HOLD)), ref(cout()), *tail) == A.OK
    assert fn(*ctx, ref(S()), ref(SR()), 0, ref(cin("recv", ctl_kind=None)), ref(cout(conv_row=None)), *tail) == A.OK
    assert fn(*ctx, ref(S()), ref(SR()), 0, ref(cin("timer")), ref(cout()), *tail) == A.OK
    assert fn(*ctx, ref(S()), ref(SR()), 0, ref(cin("timer", m_max=0)), ref(cout(closed_rows=None, closed_at=None, n_closed=None)),
              *tail) == A.OK
    if codec is not None:
        torch.cuda.synchronize()
    assert R.host(a["cnt"], np.uint32)[0] == 0 and bool((R.host(a["row"], np.uint8) == SENT).all())
    assert bool((lists.cpu().view(torch.uint8) == SENT).all())
    C.compare_table(server, before)
    assert bool((server.index == index).all())
    assert L.rsk_conv_close_bytes(0) == 0 and L.rsk_conv_close_bytes(A.CONN_MAX_ROWS + 1) == 0
    for cap in (1, 15, 16, 17, 1025, A.CONN_MAX_ROWS):  # one mark per row, rounded up to 16
        assert L.rsk_conv_close_bytes(cap) == (cap + 15) // 16 * 16


# ---- constructed clusters (tests/collide.py): index, resolve, create and close on one run ---------------------------
CLUSTER_LENGTHS = R.CR.CLUSTER_LENGTHS
INDEX_CLUSTERS = ([(n, shape, f, True) for n in CLUSTER_LENGTHS for shape in R.CR.CLUSTER_SHAPES for f in R.FLAG_COMBOS] +
                  [(65, "two_homes", (True, True), False), (257, "duplicates", (False, False), False),
                   (1025, "one_home", (False, True), False), (2049, "one_home", (True, True), True),
                   (2049, "duplicates", (True, False), True)])
LIFE_CLUSTERS = ([(n, f, True) for n in CLUSTER_LENGTHS for f in R.FLAG_COMBOS] +
                 [(65, (True, True), False), (257, (False, False), False), (1025, (True, False), False), (2049, (True, True), True)])


def cluster_keys(k, by_dst, by_id, home, slots, salt=0, base=0):
    """k distinct conv-table keys whose probes all start at `home`: the client's 32-bit convs by search, the others
    by running the hash backwards (BY_DST: the 64-bit key word is dst << 32 | conv; BY_ID alone: every conv under an
    IdBuf of its own; both: three IdBufs).  Another `salt`, other keys (the client's: the keys after the first `base`).  -> dict(conv, dst, id [k*8]) with None for
    the absent columns."""
    from tests import collide as X

    if not by_dst and not by_id:
        return {"conv": X.convs_at(home, base + k, slots)[base:], "dst": None, "id": None}
    if not by_dst:
        conv = ((np.arange(1, k + 1, dtype=np.uint64) + np.uint64(salt << 16)) * np.uint64(2654435761)).astype(np.uint32)
        return {"conv": conv, "dst": None, "id": X.ids_at(home, k, salt=salt, key=conv.astype(np.uint64)).view(np.uint8)}
    idw = np.array([0x1111, 0x0123456789ABCDEF, 2**64 - 1], np.uint64)[np.arange(k) % 3] if by_id else np.zeros(k, np.uint64)
    key = X.keys_at(home, k, idw, salt=salt)
    return {"conv": key.astype(np.uint32), "dst": (key >> np.uint64(32)).astype(np.uint32), "id": idw.view(np.uint8) if by_id else None}


def keys_take(keys, idx):
    """The keys `idx` of a cluster_keys dict."""
    k = len(keys["conv"])
    return {f: (None if v is None else v.reshape(k, -1)[idx].reshape(-1)) for f, v in keys.items()}


def keys_cat(parts):
    return {f: (None if parts[0][f] is None else np.concatenate([p[f] for p in parts])) for f in parts[0]}


def keys_batch(keys):
    """One VALID DATA packet per key."""
    n = len(keys["conv"])
    return {"status": np.ones(n, np.int8), "cmd": None, "hit": None, "conv": keys["conv"], "dst": keys["dst"], "id": keys["id"],
            "ctl_kind": None, "ctl_arg": None}


def scenario_cluster_index(rc, length, shape, by_dst, by_id, wrap, device, codec=None):
    """conn_ref.scenario_cluster for the conv table's key forms: every row LIVE, capacity = length, every key probing
    from one entry (two_homes: from H and H + 1 in turn; duplicates: a third of the rows repeat a key of the run).
    n_dup, the read-back proof that the index is one run from the predicted entry, rsk_conn.h's contract, and the
    resolve of every present key (the lowest row wins), of absent keys of the same home, of the neighbouring homes and
    of the entries at and behind the run's end."""
    from tests import collide as X

    home = R.CR.WRAP_HOME if wrap else R.CR.INNER_HOME
    cap, slots = length, X.conn_slots(length)
    rng = np.random.default_rng(length * 16 + by_dst * 8 + by_id * 4 + wrap * 2 + len(shape))
    if shape == "two_homes":
        a, b = cluster_keys((cap + 1) // 2, by_dst, by_id, home, slots), cluster_keys(cap // 2, by_dst, by_id, home + 1, slots, salt=1)
        order = np.argsort(np.concatenate([np.arange(0, cap, 2), np.arange(1, cap, 2)]), kind="stable")
        keys = keys_take(keys_cat([a, b]), order)
    else:
        keys = cluster_keys(cap, by_dst, by_id, home, slots)
        if shape == "duplicates":
            src = np.arange(cap)
            rep = rng.permutation(cap)[: cap // 3]
            src[rep] = rng.integers(0, cap, len(rep))
            keys = keys_take(keys, src)
    keys = keys_take(keys, rng.permutation(cap))
    cols = R.random_columns(rng, cap, by_dst, by_id)
    for f, v in keys.items():
        if v is not None:
            cols[f][:] = v
    cols["state"][:] = LIVE | (rng.integers(0, 2, cap) << 1).astype(np.uint8)
    tmap, dup = R.table_map(cols, by_dst, by_id)
    distinct = cap - dup
    absent = [cluster_keys(8, by_dst, by_id, home, slots, salt=3, base=cap)] + \
             [cluster_keys(3, by_dst, by_id, home + d, slots, salt=4 + j, base=cap) for j, d in enumerate((-1, 1, 2, cap - 1, cap))]
    probe = keys_batch(keys_cat([keys] + absent))
    got, want, tab = R.check_case(rc, cols, probe, by_dst, by_id, device, codec)
    nd = torch.full((1,), -1, dtype=torch.int32, device=device)
    tab.rebuild(codec, n_dup=nd)
    assert int(R.host(nd, np.uint32)[0]) == dup and (dup > 0) == (shape == "duplicates")
    X.one_run(tab.index.cpu().numpy(), home, distinct)
    assert R.check_index(tab, cols, by_dst, by_id) == distinct
    assert bool((got["conv_row"][:cap] != NONE).all()) and bool((got["conv_row"][cap:] == NONE).all())
    assert got["n_unknown"] == len(probe["status"]) - cap
    return distinct


def scenario_cluster(rc, capacity, by_dst, by_id, wrap, device, codec=None):
    """A conv table whose keys, and the keys born into it, all probe from one entry.  An eighth of the rows LIVE; a
    create from 3 x capacity packets fills the table, so the run is as long as the table has rows; the list form
    closes every second row; a second create fills the table again, in place, in the index AS THE CLOSE LEFT IT;
    (BY_DST) resets close a third of the rows under HOLD, which the index forgets while they stay LIVE; the list form
    closes the rest.  After every step the occupied entries are one run from the predicted entry, the index keeps
    rsk_conn.h's contract, and every lookup, list and column equals the restatements'."""
    from tests import collide as X

    home = R.CR.WRAP_HOME if wrap else R.CR.INNER_HOME
    rng = np.random.default_rng(capacity * 8 + by_dst * 4 + by_id * 2 + wrap)
    cap = capacity
    rows = np.sort(rng.permutation(cap)[: max(cap // 8, 1)])
    k1 = cap - len(rows)
    k2 = len(range(0, cap, 2))
    keys = cluster_keys(len(rows) + k1 + k2 + 8, by_dst, by_id, home, X.conn_slots(cap))
    part = lambda lo, hi: keys_take(keys, np.arange(lo, hi))  # noqa: E731
    cols = R.random_columns(rng, cap, by_dst, by_id)
    for f, v in part(0, len(rows)).items():
        if v is not None:
            cols[f].reshape(cap, -1)[rows] = v.reshape(len(rows), -1)
    cols["state"][rows] = LIVE | (rng.integers(0, 2, len(rows)) << 1).astype(np.uint8)

    def batch(lo, hi, n, known_from):
        """n packets: known keys of `known_from`'s LIVE rows and the keys lo..hi, each of those at least once."""
        new = part(lo, hi)
        live = np.nonzero(known_from["state"] & LIVE)[0]
        which = np.concatenate([np.arange(hi - lo), rng.integers(0, hi - lo, n // 2), -1 - rng.integers(0, len(live), n - n // 2 - (hi - lo))])
        which = rng.permutation(which)
        r = live[np.maximum(-1 - which, 0)]
        w = np.maximum(which, 0)
        pick = lambda f, width=1: np.where((which >= 0)[:, None], new[f].reshape(hi - lo, width)[w],  # noqa: E731
                                           known_from[f].reshape(cap, width)[r]).reshape(-1)
        return {"status": np.ones(n, np.int8), "cmd": None, "hit": None, "conv": pick("conv"), "dst": pick("dst") if by_dst else None,
                "id": pick("id", 8) if by_id else None, "ctl_kind": None, "ctl_arg": None}

    run = lambda tab, m: X.one_run(tab.index.cpu().numpy(), home, m)  # noqa: E731
    n = 3 * cap
    # the create fills the table: one run as long as the table has rows
    got, ref, tab, _b = C.resolve_create(rc, cols, batch(len(rows), len(rows) + k1, n, cols), by_dst, by_id, device, codec)
    assert got["n_new"] == k1 and got["n_unknown"] == 0
    run(tab, cap)
    # the list form closes every second row; no rebuild behind it
    now = ref["cols"]
    lst = rng.permutation(np.arange(0, cap, 2)).astype(np.uint32)
    cref = close_ref(now["state"], close_rows=lst, n_close=len(lst), m_max=len(lst))
    compare(run_close(rc, tab, device, codec, close_rows=lst, n_close=len(lst)), cref)
    C.compare_table(tab, dict(now, state=cref["state"]))
    check_lookups(rc, tab, now, cref["lookup_state"], by_dst, by_id, device, codec)
    now = dict(now, state=cref["state"])
    run(tab, cap - k2)
    # a second create, in place, into the run as the close left it
    c2 = batch(len(rows) + k1, len(rows) + k1 + k2, n, now)
    res_want = R.resolve_ref(now, by_dst, by_id, c2)
    res = R.run_resolve(rc, tab, c2, device, codec, msg_mode="none")
    R.compare(res, res_want)
    after = dict(now, cur_in=now["cur_in"] + res_want["add"])
    ref2 = C.create_ref(after, by_dst, by_id, c2, res["conv_row"], res["unknown"], n)
    C.compare(C.run_create(rc, tab, C.Batch(c2, res["conv_row"], res["unknown"], device), n, codec), ref2)
    now = ref2["cols"]
    C.compare_table(tab, now)
    C.check_lookups(rc, tab, now, by_dst, by_id, device, codec)
    assert ref2["n_new"] == k2 and ref2["n_unknown"] == 0
    run(tab, cap)
    left = cap
    if by_dst:  # one CONV_RST (its last word on its key) for every third row, closed under HOLD
        hit = np.arange(1, cap, 3)
        idb = None if not by_id else now["id"].reshape(cap, 8)[hit].reshape(-1)
        c3 = {"status": np.ones(len(hit), np.int8), "cmd": np.full(len(hit), A.CMD_CONV_RST, np.uint8), "hit": None,
              "conv": rng.integers(0, 2**32, len(hit), dtype=np.uint64).astype(np.uint32), "dst": now["dst"][hit], "id": idb,
              "ctl_kind": np.full(len(hit), A.CTL_CONV_RST, np.uint8), "ctl_arg": now["conv"][hit].astype(np.uint64)}
        res = R.run_resolve(rc, tab, c3, device, codec, msg_mode="none")
        assert np.array_equal(res["conv_row"], hit.astype(np.uint32))
        href = close_ref(now["state"], True, res["rst_first"], c3["ctl_kind"], res["conv_row"], res["unknown"], res["n_unknown"])
        compare(run_close(rc, tab, device, codec, hold=True, rst_first=res["rst_first"], ctl_kind=c3["ctl_kind"],
                          conv_row=res["conv_row"], unknown=res["unknown"], n_unknown=res["n_unknown"]), href)
        assert href["n_closed"] == len(hit) and np.array_equal(href["state"], now["state"])
        check_table(rc, tab, now, href, by_dst, by_id, device, codec, hold=True)  # the index forgets rows that stay LIVE
        left = cap - len(hit)
        run(tab, left)
    # then the rest
    lst = rng.permutation(cap).astype(np.uint32)
    cref = close_ref(now["state"], close_rows=lst, n_close=cap, m_max=cap)
    compare(run_close(rc, tab, device, codec, close_rows=lst, n_close=cap), cref)
    check_table(rc, tab, now, cref, by_dst, by_id, device, codec)
    assert not (cref["state"] & LIVE).any()
    run(tab, 0)
    return k1 + k2
