"""TEST INFRASTRUCTURE: the send pick (rsk_conn_pick_build / rsk_conn_pick_batch, include/rsk_codec.h)
restated twice, and the scenarios the CPU and GPU tests share (the device is a parameter: "cpu" drives the
host twins, a cuda device the batch calls of a Codec).

  rule_ref      the header's rule in numpy: groups, candidates in ascending row order, one draw per packet,
                the avoided candidate skipped by index arithmetic.
  dosend_walk   INetGroup::doSend (conn/INetGroup.cpp:111-135) step by step over an ordered conn list, fed
                from a draw iterator: it removes dead conns as it meets them and draws again; a step cap turns
                the reference's endless loop (the only alive conn is the one to avoid) into an exception."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import torch

from rsock_amd import _abi as A
from rsock_amd import workload
from tests import conn_ref as CR

NONE = A.CONN_NONE
UP = CR.UP
ERR_NO_CONN = CR.ERR_NO_CONN
SIZES = (1, 63, 64, 65, 2047, 2048, 2049, 4097)  # wave and tile edges of a 2048-packet block
CAPACITIES = (1, 2, 257, 65536)
BIG_GROUPS = (1024, 1025)  # a client table at, and just past, the 1024 rows whose candidates are staged in LDS


# ---- the two restatements -----------------------------------------------------------------------------------
def candidates(state, id, by_id):
    """-> {id word (0 without by_id): ascending array of the LIVE | ALIVE rows}."""
    up = np.nonzero((np.asarray(state) & UP) == UP)[0]
    if not by_id:
        return {0: up}
    w = CR.id_words(id, len(state))[up]
    return {int(k): up[w == k] for k in np.unique(w)}


def seed_draws(seed, n):
    """The draws of draw == NULL: the upper halves of the first n words of the splitmix64 stream."""
    return (workload.splitmix64_np(seed, 0, n) >> np.uint64(32)).astype(np.uint32)


def rule_ref(cols, by_id, n, len=None, id=None, avoid_key=None, draw=None, seed=0, derived=None):
    """-> (conn uint32 [n], n_none, used uint8 [capacity])."""
    cap = cols["state"].shape[0]
    groups, tmap = derived or (candidates(cols["state"], cols["id"], by_id),
                               CR.table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)[0])
    w = CR.id_words(id if by_id else None, n)
    d = np.asarray(draw, np.uint32) if draw is not None else seed_draws(seed, n)
    conn, used, n_none = np.full(n, NONE, np.uint32), np.zeros(cap, np.uint8), 0
    for i in range(n):
        if len is not None and int(len[i]) <= 0:
            continue
        g = groups.get(int(w[i]))
        m = 0 if g is None else g.shape[0]
        if m == 0:
            n_none += 1
            continue
        a = 0 if avoid_key is None else int(avoid_key[i])
        p = None
        if a != 0:
            r = tmap.get((int(w[i]), a))
            if r is not None:
                at = np.nonzero(g == r)[0]
                if at.size:
                    p = int(at[0])
        if p is None:
            k = int(d[i]) % m
        elif m == 1:
            n_none += 1
            continue
        else:
            k = int(d[i]) % (m - 1)
            k += k >= p
        conn[i] = g[k]
        used[g[k]] = 1
    return conn, n_none, used


class Spin(Exception):
    """dosend_walk gave up: the reference would loop for ever."""


def dosend_walk(conns, draws, nread=1, key_of_conn_to_reset=0, cap=10000):
    """conns: the group's mConns in order, a list of [row, intKey, alive]; dead ones are removed from it as
    the walk meets them.  draws: an iterator of rand() values.  -> the row that sends, ERR_NO_CONN, or nread
    when nread <= 0."""
    if nread > 0:
        steps = 0
        while conns:
            steps += 1
            if steps > cap:
                raise Spin()
            n = next(draws) % len(conns)
            row, key, alive = conns[n]
            if alive:
                if key_of_conn_to_reset != 0 and key == key_of_conn_to_reset:
                    continue
                return row
            del conns[n]
        return ERR_NO_CONN
    return nread


# ---- tables and the driver ------------------------------------------------------------------------------------
def tensor(a, device):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8 if a.dtype == np.uint8 else f"i{a.dtype.itemsize}").copy()).to(device)


def make_table(rc, cols, by_id, device, codec=None, build=True):
    """A ConnTable on `device` holding `cols`, its conn index and pick index built there."""
    tab = CR.make_table(rc, cols, cols["state"].shape[0], device, by_id=by_id)
    if build:
        tab.rebuild(codec)
        tab.rebuild_pick(codec)
    return tab


def run_pick(rc, tab, n, device, codec=None, len=None, id=None, avoid_key=None, draw=None, seed=0, nthreads=1,
             stream=None):
    """-> (conn uint32 [n], n_none, used uint8 [capacity]) of the host twin or the device call."""
    if device == "cpu":
        used = np.zeros(tab.capacity, np.uint8)
        conn, nn = rc.conn_pick_host(tab, n, len=len, id=id, avoid_key=avoid_key, draw=draw, seed=seed, used=used,
                                     nthreads=nthreads)
        return conn, nn, used
    conn = torch.full((max(n, 1),), 0x6E6E6E6E, dtype=torch.int32, device=device)
    nn = torch.full((1,), -1, dtype=torch.int32, device=device)
    used = torch.zeros(tab.capacity, dtype=torch.uint8, device=device)
    t = lambda a: tensor(a, device)  # noqa: E731
    codec.conn_pick_batch(tab, conn[:n], len=t(len), id=t(id), avoid_key=t(avoid_key), draw=t(draw), seed=seed,
                          n_none=nn, used=used, stream=stream)
    torch.cuda.synchronize()
    return conn[:n].cpu().numpy().view(np.uint32), int(nn.cpu().numpy().view(np.uint32)[0]), used.cpu().numpy()


def compare(got, want, what=""):
    assert np.array_equal(got[0], want[0]), (what, "conn", np.nonzero(got[0] != want[0])[0][:8])
    assert got[1] == want[1], (what, "n_none", got[1], want[1])
    assert np.array_equal(got[2], want[2]), (what, "used")


def check(rc, cols, by_id, n, device, codec=None, tab=None, derived=None, nthreads=1, **batch):
    tab = tab or make_table(rc, cols, by_id, device, codec)
    got = run_pick(rc, tab, n, device, codec, nthreads=nthreads, **batch)
    want = rule_ref(cols, by_id, n, derived=derived, **batch)
    compare(got, want)
    return got, want


def id_bytes(words):
    return np.ascontiguousarray(np.asarray(words, np.uint64)).view(np.uint8)


EDGE_DRAWS = np.array([0, 1, 0xFFFFFFFF, 0xFFFFFFFE, 0x80000000, 0x7FFFFFFF], np.uint32)


# ---- 1. sizes ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sized_table(capacity, by_id):
    """Random LIVE / ALIVE bits; with by_id the rows spread over a few IdBufs.  -> (cols, id pool, derived)."""
    rng = np.random.default_rng(1000 + capacity + by_id)
    cols = CR.random_columns(rng, capacity, by_id=by_id)
    cols["state"][:] = rng.integers(0, 8, capacity).astype(np.uint8)  # LIVE, ALIVE, NEW at random
    pool = np.concatenate([[0], rng.integers(1, 2**63, 6, dtype=np.uint64)]).astype(np.uint64)
    if by_id:
        cols["id"][:] = id_bytes(pool[rng.integers(0, 5, capacity)])  # pool[5], pool[6]: no group has them
    derived = (candidates(cols["state"], cols["id"], by_id),
               CR.table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)[0])
    return cols, pool, derived


def random_batch(rng, cols, pool, by_id, n):
    cap = cols["state"].shape[0]
    rows = rng.integers(0, cap, n)
    avoid = np.where(rng.random(n) < 0.5, cols["conn_key"][rows], 0).astype(np.uint64)
    avoid[rng.random(n) < 0.05] = rng.integers(1, 2**63, dtype=np.uint64)
    draw = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    draw[: min(n, EDGE_DRAWS.size)] = EDGE_DRAWS[: min(n, EDGE_DRAWS.size)]
    b = {"len": np.where(rng.random(n) < 0.85, rng.integers(1, 1500, n), rng.integers(-2, 1, n)).astype(np.int32),
         "avoid_key": avoid, "draw": draw}
    if by_id:
        # mostly the id of the avoided row (so the avoid key is found under it), some other ids of the pool
        w = CR.id_words(cols["id"], cap)[rows]
        other = rng.random(n) < 0.3
        w[other] = pool[rng.integers(0, pool.size, int(other.sum()))]
        b["id"] = id_bytes(w)
    return b


def scenario_sizes(rc, n, capacity, by_id, device, codec=None, tables=None):
    cols, pool, derived = sized_table(capacity, by_id)
    key = (capacity, by_id, str(device))
    if tables is not None and key not in tables:
        tables[key] = make_table(rc, cols, by_id, device, codec)
    tab = tables[key] if tables is not None else None
    rng = np.random.default_rng(n * 7 + capacity)
    return check(rc, cols, by_id, n, device, codec, tab=tab, derived=derived, **random_batch(rng, cols, pool, by_id, n))


# ---- 2. group shapes ----------------------------------------------------------------------------------------
GROUP_SIZES = (1, 2, 63, 64, 65)


def grouped_table(zero_real):
    """A BY_ID table: groups of 1, 2, 63, 64 and 65 candidates (each with some dead and some non-LIVE rows
    besides), a group whose rows are all dead, one whose rows are not LIVE, the rows of all of them
    interleaved; with zero_real the 64-candidate group's id is eight zero bytes.  -> (cols, ids by name)."""
    rng = np.random.default_rng(77)
    ids = {m: int(rng.integers(1, 2**63, dtype=np.uint64)) for m in GROUP_SIZES}
    if zero_real:
        ids[64] = 0
    ids["dead"], ids["unlive"], ids["absent"] = (int(rng.integers(1, 2**63, dtype=np.uint64)) for _ in range(3))
    if not zero_real:
        ids["zero"] = 0  # an absent group
    rows = []  # (id word, state)
    for m in GROUP_SIZES:
        rows += [(ids[m], UP)] * m + [(ids[m], A.CONN_LIVE)] * 3 + [(ids[m], A.CONN_ALIVE)] * 2 + [(ids[m], 0)]
    rows += [(ids["dead"], A.CONN_LIVE)] * 5 + [(ids["unlive"], A.CONN_ALIVE)] * 5
    order = rng.permutation(len(rows))
    cap = len(rows) + 9  # spare rows: state 0
    cols = CR.random_columns(rng, cap, by_id=True)
    at = np.sort(rng.permutation(cap)[: len(rows)])
    w = np.array([rows[j][0] for j in order], np.uint64)
    cols["id"].reshape(-1, 8)[at] = id_bytes(w).reshape(-1, 8)
    cols["state"][at] = np.array([rows[j][1] for j in order], np.uint8)
    return cols, ids


def scenario_groups(rc, zero_real, device, codec=None):
    cols, ids = grouped_table(zero_real)
    groups = candidates(cols["state"], cols["id"], True)
    assert sorted(len(g) for g in groups.values()) == sorted(GROUP_SIZES)
    for g in groups.values():  # interleaved: no group of several rows is contiguous
        assert len(g) < 3 or not np.array_equal(g, np.arange(g[0], g[0] + len(g)))
    rng = np.random.default_rng(5)
    names = list(ids)
    per = 200
    w = np.repeat(np.array([ids[k] for k in names], np.uint64), per)
    n = w.size
    draw = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    for j, k in enumerate(names):  # draws around the multiples of every group's m
        m = k if isinstance(k, int) else 7
        edge = np.concatenate([np.arange(2 * m + 2), [0xFFFFFFFF, 0xFFFFFFFF // m * m, 0xFFFFFFFF // m * m - 1]]
                              ).astype(np.uint64).astype(np.uint32)
        draw[j * per: j * per + edge.size] = edge
    got, want = check(rc, cols, True, n, device, codec, id=id_bytes(w), draw=draw)
    none = want[0] == NONE
    expect_none = np.repeat(np.array([not isinstance(k, int) for k in names]), per)
    assert np.array_equal(none, expect_none) and want[1] == int(expect_none.sum())
    for k in GROUP_SIZES:  # every candidate of every group is reached, nothing else
        assert set(want[0][w == np.uint64(ids[k])].tolist()) == set(groups[ids[k]].tolist())
    return got, want


def scenario_big_group(rc, m, device, codec=None):
    """A client table of m rows, every one a candidate of its one group; then the same with some rows dead."""
    rng = np.random.default_rng(m)
    cap = m
    cols = CR.random_columns(rng, cap)
    cols["state"][:] = UP
    n = 4097
    draw = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    draw[:6] = np.array([0, m - 1, m, m + 1, 2 * m - 1, 0xFFFFFFFF], np.uint64).astype(np.uint32)
    avoid = np.where(rng.random(n) < 0.3, cols["conn_key"][rng.integers(0, cap, n)], 0).astype(np.uint64)
    got, want = check(rc, cols, False, n, device, codec, draw=draw, avoid_key=avoid)
    assert want[1] == 0 and int(want[2].sum()) > m // 2
    cols["state"][rng.permutation(cap)[:70]] = A.CONN_LIVE
    check(rc, cols, False, n, device, codec, draw=draw, avoid_key=avoid)
    return got, want


# ---- 3. avoid keys --------------------------------------------------------------------------------------------
def scenario_avoid(rc, by_id, device, codec=None):
    rng = np.random.default_rng(31 + by_id)
    cap = 40
    cols = CR.random_columns(rng, cap, by_id=by_id)
    ida, idb, idc = 0x1111111111111111, 0x2222222222222222, 0x3333333333333333
    cand = np.array([3, 8, 9, 17, 30])  # the group under test: five candidates
    dead, unlive, other, lone = 12, 20, 25, 35
    cols["state"][cand] = UP
    cols["state"][dead] = A.CONN_LIVE | A.CONN_NEW
    cols["state"][unlive] = A.CONN_ALIVE
    cols["state"][other] = UP
    cols["state"][lone] = UP
    cols["conn_key"][: cap] = np.arange(1000, 1000 + cap, dtype=np.uint64)
    if by_id:
        w = np.full(cap, ida, np.uint64)
        w[other] = idb  # its key is alive only under another id
        w[lone] = idc   # a group of one candidate
        cols["id"][:] = id_bytes(w)
    key = cols["conn_key"]
    cases = [("first", key[3]), ("middle", key[9]), ("last", key[30]), ("dead", key[dead]), ("unlive", key[unlive]),
             ("absent", np.uint64(999999)), ("none", np.uint64(0))]
    if by_id:
        cases.append(("other_id", key[other]))
    per = 64
    avoid = np.repeat(np.array([k for _, k in cases], np.uint64), per)
    n = avoid.size
    m = 5 if by_id else 7
    draw = np.tile(np.concatenate([np.arange(0, 3 * m + 2), [0xFFFFFFFF, 0xFFFFFFFE, 0x80000000]]).astype(np.uint32),
                   per)[:per]
    draw = np.tile(draw, len(cases))
    idcol = id_bytes(np.full(n, ida, np.uint64)) if by_id else None
    got, want = check(rc, cols, by_id, n, device, codec, id=idcol, avoid_key=avoid, draw=draw)
    for j, (name, k) in enumerate(cases):
        picked = want[0][j * per: (j + 1) * per]
        row = int(np.nonzero(key == k)[0][0]) if name in ("first", "middle", "last") else None
        assert (row is None) or row not in picked.tolist(), name
        skipped = name in ("first", "middle", "last")
        assert len(set(picked.tolist())) == m - skipped, name
    assert want[1] == 0
    # the avoided row as the only candidate: NONE, counted
    if by_id:
        tab = make_table(rc, cols, True, device, codec)
        one = {"id": id_bytes(np.full(8, idc, np.uint64)), "draw": np.arange(8, dtype=np.uint32),
               "avoid_key": np.array([key[lone]] * 4 + [0] * 4, np.uint64)}
        g1, w1 = check(rc, cols, True, 8, device, codec, tab=tab, **one)
    else:
        solo = {k: (v.copy() if v is not None else None) for k, v in cols.items()}
        solo["state"][:] = A.CONN_LIVE
        solo["state"][lone] = UP
        one = {"draw": np.arange(8, dtype=np.uint32), "avoid_key": np.array([key[lone]] * 4 + [0] * 4, np.uint64)}
        g1, w1 = check(rc, solo, False, 8, device, codec, **one)
    assert w1[1] == 4 and np.array_equal(w1[0], np.array([NONE] * 4 + [lone] * 4, np.uint32))
    # an avoid column of zeros equals no column
    tab = make_table(rc, cols, by_id, device, codec)
    z = run_pick(rc, tab, n, device, codec, id=idcol, avoid_key=np.zeros(n, np.uint64), draw=draw)
    compare(z, run_pick(rc, tab, n, device, codec, id=idcol, draw=draw))
    compare(z, rule_ref(cols, by_id, n, id=idcol, draw=draw))


# ---- 4. draws -------------------------------------------------------------------------------------------------
def ten_conns(rng, by_id=False):
    cap = 16
    cols = CR.random_columns(rng, cap, by_id=by_id)
    cols["state"][:] = A.CONN_LIVE
    cols["state"][np.sort(rng.permutation(cap)[:10])] = UP
    return cols


def scenario_seed(rc, device, codec=None, seed=0x5EED_0123_4567_89AB, n=4096):
    """draw == NULL with a seed: the same as the column of the stream's upper halves; and with 10 candidates
    every one of them is picked in 4096 packets."""
    cols = ten_conns(np.random.default_rng(3))
    tab = make_table(rc, cols, False, device, codec)
    want = rule_ref(cols, False, n, seed=seed)
    assert set(want[0].tolist()) == set(candidates(cols["state"], None, False)[0].tolist())  # the inputs carry it
    if device == "cpu":
        column = seed_draws(seed, n)
    else:
        words = torch.empty(n, dtype=torch.int64, device=device)
        rc.fill_splitmix(words, seed)
        torch.cuda.synchronize()
        column = (words.cpu().numpy().view(np.uint64) >> np.uint64(32)).astype(np.uint32)
        assert np.array_equal(column, seed_draws(seed, n))
    got = run_pick(rc, tab, n, device, codec, seed=seed)
    compare(got, want)
    compare(run_pick(rc, tab, n, device, codec, draw=column), got)
    assert set(got[0].tolist()) == set(want[0].tolist()) and len(set(got[0].tolist())) == 10


# ---- 5. the len gate and what is read -------------------------------------------------------------------------
def scenario_reads(rc, device, codec=None):
    """len <= 0 gives NONE, uncounted; the other fields of such a packet carry poison, and without BY_ID the
    id column is a NULL pointer: no output depends on either."""
    for by_id in (False, True):
        cols, pool, derived = sized_table(257, by_id)
        tab = make_table(rc, cols, by_id, device, codec)
        rng = np.random.default_rng(8)
        n = 3000
        b = random_batch(rng, cols, pool, by_id, n)
        b["len"][::3] = np.array([0, -1, -(2**31)], np.int32)[np.arange(0, n, 3) // 3 % 3]
        skip = b["len"] <= 0
        want = rule_ref(cols, by_id, n, derived=derived, **b)
        assert bool((want[0][skip] == NONE).all()) and want[1] == int((want[0][~skip] == NONE).sum())
        for poison in (0x00, 0xFF, 0x5A):
            p = dict(b)
            for k in ("avoid_key", "draw", "id"):
                if k in p:
                    a = p[k].copy()
                    if k == "id":
                        a.reshape(-1, 8)[skip] = poison
                    else:
                        a[skip] = a.dtype.type(int.from_bytes(bytes([poison] * a.dtype.itemsize), "little"))
                    p[k] = a
            compare(run_pick(rc, tab, n, device, codec, **p), want, f"poison {poison:#x}")
        if not by_id:  # an id column given to a client table is ignored
            p = dict(b)
            p["id"] = np.full(8 * n, 0xA5, np.uint8)
            compare(run_pick(rc, tab, n, device, codec, **p), want, "id without BY_ID")
    # nothing taken: only len is read
    got = run_pick(rc, tab, 100, device, codec, len=np.zeros(100, np.int32), id=np.zeros(800, np.uint8))
    assert bool((got[0] == NONE).all()) and got[1] == 0 and not got[2].any()


# ---- 6. a stale index -----------------------------------------------------------------------------------------
def scenario_stale_state(rc, by_id, device, codec=None):
    """state changed after the build: every conn is NONE or a row of the table (which one is unspecified)."""
    cols, pool, _ = sized_table(257, by_id)
    tab = make_table(rc, cols, by_id, device, codec)
    rng = np.random.default_rng(12)
    new = rng.integers(0, 4, 257).astype(np.uint8)
    tab.load(state=new)
    b = random_batch(rng, cols, pool, by_id, 4097)
    conn, nn, used = run_pick(rc, tab, 4097, device, codec, **b)
    ok = (conn == NONE) | (conn < 257)
    assert bool(ok.all()) and nn <= 4097
    tab.rebuild(codec)
    tab.rebuild_pick(codec)  # and after the rebuild the rule holds again
    stale_cols = dict(cols)
    stale_cols["state"] = new
    compare(run_pick(rc, tab, 4097, device, codec, **b), rule_ref(stale_cols, by_id, 4097, **b))


def scenario_garbage_index(rc, by_id, capacity, seed):
    """HOST ONLY.  A pick index that was never built: words drawn from rows and offsets inside and outside
    their ranges.  Every conn is NONE or a row of the table."""
    cols, pool, _ = sized_table(capacity, by_id)
    tab = CR.make_table(rc, cols, capacity, "cpu", by_id=by_id)
    tab.rebuild(None)
    rng = np.random.default_rng(seed)
    words = tab.pick.numel()
    menu = np.array([0, 1, 2, capacity - 1, capacity, capacity + 1, 2 * capacity, words, 0x7FFFFFFF, 0x80000000,
                     0xFFFFFFFE, 0xFFFFFFFF], np.uint64)
    g = np.where(rng.random(words) < 0.5, menu[rng.integers(0, menu.size, words)],
                 rng.integers(0, 2 * capacity + 2, words, dtype=np.uint64)).astype(np.uint32)
    if by_id and seed % 2:  # group entries under the ids the packets carry, so the probe finds them
        slots = (words - 4 - 2 * ((capacity + 3) & ~3)) // 5
        ent = g[words - 4 * slots:].reshape(slots, 4)
        ent[:, :2] = np.ascontiguousarray(pool[rng.integers(0, pool.size, slots)]).view(np.uint32).reshape(slots, 2)
    tab.pick.copy_(torch.from_numpy(g.view(np.int32)))
    n = 4097
    b = random_batch(rng, cols, pool, by_id, n)
    for nthreads in (1, 4):
        conn, nn, used = run_pick(rc, tab, n, "cpu", **b, nthreads=nthreads)
        assert bool(((conn == NONE) | (conn < capacity)).all())
        assert nn == int(((conn == NONE) & (b["len"] > 0)).sum())


# ---- 8. argument errors and the empty batch -------------------------------------------------------------------
def check_einval(rc, device, codec=None):
    lib = rc.lib()
    cpu = device == "cpu"
    cols, pool, _ = sized_table(257, True)
    srv = make_table(rc, cols, True, device, codec)
    ccols, _, _ = sized_table(257, False)
    cli = make_table(rc, ccols, False, device, codec)
    n = 10
    conn = tensor(np.zeros(n, np.uint32), device)
    idc = tensor(np.zeros(8 * n + 8, np.uint8), device)
    avoid = tensor(np.zeros(n, np.uint64), device)
    nn = tensor(np.full(1, 7, np.uint32), device)
    cnt = tensor(np.zeros(2, np.uint32), device)

    def batch(t, pick, n_, pin, pout, ctx=True):
        ta = ctypes.byref(t) if t is not None else None
        pi = ctypes.byref(pin) if pin is not None else None
        po = ctypes.byref(pout) if pout is not None else None
        if cpu:
            return lib.rsk_conn_pick_host(ta, pick, n_, pi, po, 1)
        return lib.rsk_conn_pick_batch(codec._ctx if ctx else None, ta, pick, n_, pi, po, None)

    def build(t, pick, ctx=True):
        ta = ctypes.byref(t) if t is not None else None
        if cpu:
            return lib.rsk_conn_pick_build_host(ta, pick, cnt.data_ptr(), 1)
        return lib.rsk_conn_pick_build(codec._ctx if ctx else None, ta, pick, cnt.data_ptr(), None)

    sp, cp = srv.pick.data_ptr(), cli.pick.data_ptr()
    pin = A.ConnPickIn(None, idc.data_ptr(), None, None, 1)
    pout = A.ConnPickOut(conn.data_ptr(), nn.data_ptr(), None)
    assert batch(srv.abi(), sp, n, pin, pout) == A.OK
    assert build(srv.abi(), sp) == A.OK
    bad = []
    if not cpu:
        bad += [batch(srv.abi(), sp, n, pin, pout, ctx=False), build(srv.abi(), sp, ctx=False)]
        bad.append(batch(srv.abi(), sp, A.MAX_BATCH + 1, pin, pout))
        # an id column that is not 8-B aligned: the batch's, then the table's
        bad.append(batch(srv.abi(), sp, n, A.ConnPickIn(None, idc.data_ptr() + 4, None, None, 1), pout))
        t = srv.abi()
        t.id += 4
        bad += [batch(t, sp, n, pin, pout), build(t, sp)]
    bad += [batch(None, sp, n, pin, pout), batch(srv.abi(), None, n, pin, pout), batch(srv.abi(), sp, n, None, pout),
            batch(srv.abi(), sp, n, pin, None), build(None, sp), build(srv.abi(), None)]
    bad.append(batch(srv.abi(), sp, n, pin, A.ConnPickOut(None, nn.data_ptr(), None)))  # a NULL conn with n > 0
    bad.append(batch(srv.abi(), sp, n, A.ConnPickIn(None, None, None, None, 1), pout))  # id missing with BY_ID
    t = srv.abi()
    t.id = None
    bad += [batch(t, sp, n, pin, pout), build(t, sp)]
    for field in ("conn_key", "index"):  # avoid_key on a table that cannot look a key up
        t = cli.abi()
        setattr(t, field, None)
        bad.append(batch(t, cp, n, A.ConnPickIn(None, None, avoid.data_ptr(), None, 1), pout))
        assert batch(t, cp, n, A.ConnPickIn(None, None, None, None, 1), pout) == A.OK  # fine without the column
    t = cli.abi()
    t.state = None
    bad.append(build(t, cp))
    assert batch(t, cp, n, A.ConnPickIn(None, None, None, None, 1), pout) == A.OK  # the batch does not read state
    for flags, capacity in ((2, 257), (0, 0), (0, A.CONN_MAX_ROWS + 1)):
        t = cli.abi()
        t.flags, t.capacity = flags, capacity
        bad += [batch(t, cp, n, A.ConnPickIn(None, None, None, None, 1), pout), build(t, cp)]
        assert lib.rsk_conn_pick_bytes(capacity, flags) == 0
    bad += [batch(cli.abi(), cp + 4, n, A.ConnPickIn(None, None, None, None, 1), pout), build(cli.abi(), cp + 4)]
    assert bad and all(r == A.EINVAL for r in bad), bad
    # n == 0 zeroes a given n_none, NULL columns and all
    assert batch(srv.abi(), sp, 0, A.ConnPickIn(None, None, None, None, 0), A.ConnPickOut(None, nn.data_ptr(), None)) == A.OK
    if not cpu:
        torch.cuda.synchronize()
    assert int(nn.cpu().numpy().view(np.uint32)[0]) == 0
    assert lib.rsk_conn_pick_bytes(1, 0) % 16 == 0 and lib.rsk_conn_pick_bytes(A.CONN_MAX_ROWS, 1) % 16 == 0


def group_taken(tab):
    """Which entries of the pick index's group table are taken (rsk_pick.h: [4 + 2 C4 + S, + 4 S), 16 B per entry
    {IdBuf word, offset, count}, count 0 = free), read back from a BY_ID table's pick index."""
    from tests import collide as X

    cap = tab.capacity
    c4, slots = (cap + 3) & ~3, X.conn_slots(cap)
    pick = tab.pick.cpu().numpy().view(np.uint32)
    assert len(pick) == 4 + 2 * c4 + 5 * slots, "tests/pick_ref.py: rsk_pick.h's layout has changed"
    return pick[4 + 2 * c4 + slots:].reshape(slots, 4)[:, 3] != 0


def check_group_run(tab, cols, home):
    """The proof that ids built to share a pick home do: on a freshly built pick index the taken group entries are
    one run from the predicted entry, as many as there are groups with a candidate."""
    from tests import collide as X

    groups = sum(1 for g in candidates(cols["state"], cols["id"], True).values() if len(g))
    X.run_of(group_taken(tab), home, groups, "the constructed IdBufs' group entries")
    return groups


# ---- constructed clusters (tests/collide.py) -------------------------------------------------------------------
def scenario_colliding_groups(rc, groups, device, codec=None, wrap=True):
    """`groups` IdBufs whose group entries in the pick index all probe from one entry (a run of `groups` entries,
    across the index's end when `wrap`), one to four candidates each and some rows that are no candidates; the conn
    keys probe from one entry of the conn index too, so the avoid keys walk its run.  Draws over every group, avoid
    keys of the group, of another group and of nobody, and ids of the same home that no row has."""
    from tests import collide as X

    home = CR.WRAP_HOME if wrap else CR.INNER_HOME
    rng = np.random.default_rng(groups + wrap)
    cap = 3 * groups
    gids = X.ids_at(home, groups + 3)
    assert {X.group_home(int(g), cap) for g in gids} == {home % X.conn_slots(cap)}
    w = gids[np.concatenate([np.arange(groups), rng.integers(0, groups, cap - groups)])][rng.permutation(cap)]
    cols = CR.random_columns(rng, cap, by_id=True)
    CR.place(cols, np.arange(cap), X.keys_at(home, cap, w), id=id_bytes(w))
    cols["state"][rng.random(cap) < 0.15] = A.CONN_LIVE  # LIVE, not ALIVE: in the conn index, no candidate
    per = 4
    wi = np.repeat(np.concatenate([gids, gids[:2]]), per)  # the last ids: no row has them
    n = len(wi)
    rows = rng.integers(0, cap, n)
    own = np.array([rng.choice(np.nonzero(w == i)[0]) if (w == i).any() else 0 for i in wi])
    kind = np.arange(n) % per
    avoid = np.where(kind == 0, 0, np.where(kind == 1, cols["conn_key"][own], cols["conn_key"][rows])).astype(np.uint64)
    avoid[kind == 3] = X.keys_at(home, int((kind == 3).sum()), wi[kind == 3], salt=5)  # absent, walks the whole run
    draw = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    draw[: EDGE_DRAWS.size] = EDGE_DRAWS
    tab = make_table(rc, cols, True, device, codec)
    if codec is not None:
        torch.cuda.synchronize()
    CR.check_index(tab, cols, True)
    assert check_group_run(tab, cols, home) > groups // 2  # some one-row groups lost their only candidate
    got, want = check(rc, cols, True, n, device, codec, tab=tab, id=id_bytes(wi), avoid_key=avoid, draw=draw)
    assert want[1] >= 2 * per and int((want[0] != NONE).sum()) > n // 2
    return n
