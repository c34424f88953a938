"""TEST INFRASTRUCTURE: the connection table (rsk_conn_table, include/rsk_codec.h) restated with a dict
and numpy, and the tables / batches the CPU and GPU tests share.

The reference keeps the level per packet: INetGroup::Input looks the packet's connKey up in mConnMap
(conn/INetGroup.cpp:57-83; one INetGroup per IdBuf on a server, server/ServerGroup.cpp:44-60), only for
DATA packets (conn/IAppGroup.cpp:80-95), and a packet to send takes its connection's TcpInfo
(conn/INetConn.cpp:30-39, conn/FakeTcp.cpp:14-50)."""
from __future__ import annotations

import os

import numpy as np

from rsock_amd import _abi as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "demux.npz")
ERR_NO_CONN = -20  # INetGroup::ERR_NO_CONN, the reference's return for a DATA packet of an unknown connKey
NONE = A.CONN_NONE
UP = A.CONN_LIVE | A.CONN_ALIVE
EXPAND_COLUMNS = ("src", "dst", "sp", "dp", "ack", "flag", "conn_key")


def id_words(id, n):
    """The [n*8] IdBuf bytes as one uint64 per packet / row (zeros without an id column)."""
    if id is None:
        return np.zeros(n, np.uint64)
    return np.ascontiguousarray(id, np.uint8).reshape(n, 8).view(np.uint64).ravel()


def table_map(state, conn_key, id=None):
    """-> ({(id word, connKey): lowest LIVE row}, number of LIVE rows that lost their key)."""
    w = id_words(id, len(state))
    m, dup = {}, 0
    for r in np.nonzero(np.asarray(state) & A.CONN_LIVE)[0].tolist():
        k = (int(w[r]), int(conn_key[r]))
        if k in m:
            dup += 1
        else:
            m[k] = r
    return m, dup


def resolve_ref(tmap, status, conn_key, cmd=None, id=None):
    """rsk_conn_resolve_batch: -> (conn uint32, hit uint8, miss int8, n_miss)."""
    n = len(status)
    w = id_words(id, n)
    look = np.asarray(status) == A.RECV_VALID
    if cmd is not None:
        look &= np.asarray(cmd) == A.CMD_DATA
    conn = np.full(n, NONE, np.uint32)
    for i in np.nonzero(look)[0].tolist():
        conn[i] = tmap.get((int(w[i]), int(conn_key[i])), NONE)
    hit = (conn != NONE).astype(np.uint8)
    miss = np.where(look & (conn == NONE), A.RECV_VALID, A.RECV_DROP).astype(np.int8)
    return conn, hit, miss, int((miss == A.RECV_VALID).sum())


def expand_ref(cols, capacity, conn):
    """rsk_conn_expand_batch over the table columns `cols` (numpy, unsigned): -> (dict of the output
    columns incl. ok and, when cols has it, id [n*8]; n_bad)."""
    conn = np.asarray(conn, np.uint32)
    inside = conn < capacity
    r = np.where(inside, conn, 0).astype(np.int64)
    ok = inside & ((cols["state"][r] & UP) == UP)
    out = {k: np.where(ok, cols[k][r], 0).astype(cols[k].dtype) for k in EXPAND_COLUMNS}
    if cols.get("id") is not None:
        out["id"] = np.where(ok, id_words(cols["id"], capacity)[r], 0).astype(np.uint64).view(np.uint8)
    out["ok"] = ok.astype(np.uint8)
    return out, int((~ok).sum())


def first_missing(miss, conn_key, id=None):
    """Packet indices of the first packet of every distinct missing key, in arrival order: what
    rsk_demux_batch on the miss column lists in seg_first."""
    idx = np.nonzero(np.asarray(miss) == A.RECV_VALID)[0]
    w = id_words(id, len(miss))
    seen, out = set(), []
    for i in idx.tolist():
        k = (int(w[i]), int(conn_key[i]))
        if k not in seen:
            seen.add(k)
            out.append(i)
    return np.array(out, np.uint32)


def random_columns(rng, capacity, by_id=False):
    """Table columns with random TcpInfo and no LIVE row (numpy, unsigned dtypes)."""
    r32 = lambda: rng.integers(0, 2**32, capacity, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    r16 = lambda: rng.integers(0, 2**16, capacity, dtype=np.uint64).astype(np.uint16)  # noqa: E731
    cols = {"state": np.zeros(capacity, np.uint8), "conn_key": rng.integers(0, 2**63, capacity, dtype=np.uint64),
            "src": r32(), "dst": r32(), "sp": r16(), "dp": r16(), "seq": r32(), "ack": r32(),
            "flag": rng.integers(0, 256, capacity, dtype=np.uint64).astype(np.uint8)}
    cols["id"] = rng.integers(0, 256, capacity * 8, dtype=np.uint64).astype(np.uint8) if by_id else None
    return cols


def place(cols, rows, conn_key, id=None, state=UP):
    """Put the keys (and IdBufs) at `rows` and mark them `state`."""
    rows = np.asarray(rows, np.int64)
    cols["conn_key"][rows] = conn_key
    cols["state"][rows] = state
    if id is not None:
        cols["id"].reshape(-1, 8)[rows] = np.asarray(id, np.uint8).reshape(-1, 8)
    return cols


def make_table(rc, cols, capacity, device, by_id=False):
    """A rsock_amd.codec.ConnTable on `device` holding `cols` (index not built)."""
    tab = rc.ConnTable.alloc(capacity, device, by_id=by_id)
    return tab.load(**{k: v for k, v in cols.items() if v is not None})


def golden_case(name):
    z = np.load(GOLDEN)
    ci = z["names"].tolist().index(name)
    p = f"c{ci}_"
    return {k[len(p):]: z[k] for k in z.files if k.startswith(p)}


# the reference's own count of ERR_NO_CONN returns per client case of tests/golden/demux.npz
GOLDEN_CLIENT = {"client_large": (50000, 7983), "client_tile_edges": (9000, 4486), "client_small": (3000, 0)}


def golden_client_table(name, capacity=257, seed=5):
    """The client case `name` and a table of its known_keys at shuffled rows of a larger capacity:
    -> (case dict, table columns, {key: row})."""
    c = golden_case(name)
    rng = np.random.default_rng(seed)
    cols = random_columns(rng, capacity)
    keys = c["known_keys"]
    rows = rng.permutation(capacity)[:len(keys)]
    # the unused rows hold keys of the batch too, but are not LIVE: they must not be found
    spare = np.setdiff1d(np.arange(capacity), rows)
    cols["conn_key"][spare] = rng.choice(np.unique(c["conn_key"]), len(spare))
    place(cols, rows, keys)
    return c, cols, {int(k): int(r) for k, r in zip(keys, rows)}


def check_golden_client(name, c, key_row, conn, miss):
    """The reference pin: miss <=> the reference returned ERR_NO_CONN; a looked-up packet it delivered
    resolves to its key's row; control packets of unknown keys are NONE and no misses."""
    n, n_err = GOLDEN_CLIENT[name]
    ret, st, cmd, ck = c["ret"], c["status"], c["cmd"], c["conn_key"]
    assert len(ret) == n and int((ret == ERR_NO_CONN).sum()) == n_err
    assert np.array_equal(miss == A.RECV_VALID, ret == ERR_NO_CONN)
    look = (st == A.RECV_VALID) & (cmd == A.CMD_DATA)
    found = look & (ret != ERR_NO_CONN)
    assert found.sum() > 0
    assert np.array_equal(conn[found], np.array([key_row[int(k)] for k in ck[found]], np.uint32))
    assert bool((conn[~found] == NONE).all())
    known = np.isin(ck, np.array(list(key_row), np.uint64))
    ctrl_unknown = (st == A.RECV_VALID) & (cmd != A.CMD_DATA) & ~known
    assert bool((conn[ctrl_unknown] == NONE).all()) and bool((miss[ctrl_unknown] == A.RECV_DROP).all())
    return int(ctrl_unknown.sum())


def server_case(seed=3, frac=0.7):
    """tests/golden/demux.npz's server_many_groups inputs and a BY_ID table holding a random `frac` of
    its distinct (IdBuf, connKey) pairs: -> (case, columns, capacity)."""
    c = golden_case("server_many_groups")
    rng = np.random.default_rng(seed)
    n = len(c["status"])
    pairs = np.stack([id_words(c["id"], n), c["conn_key"]], axis=1)
    uniq = np.unique(pairs, axis=0)
    keep = uniq[rng.random(len(uniq)) < frac]
    capacity = 2 * len(uniq) + 3
    cols = random_columns(rng, capacity, by_id=True)
    # every row starts with a pair of the batch that is not LIVE
    fill = uniq[rng.integers(0, len(uniq), capacity)]
    cols["id"][:] = np.ascontiguousarray(fill[:, 0]).view(np.uint8)
    cols["conn_key"][:] = fill[:, 1]
    rows = rng.permutation(capacity)[:len(keep)]
    place(cols, rows, keep[:, 1], id=np.ascontiguousarray(keep[:, 0]).view(np.uint8))
    return c, cols, capacity


def edge_table(by_id):
    """Keys 0 and 2^64 - 1, pairs that differ only in the high word, and (BY_ID) rows that differ only in
    one IdBuf byte; one LIVE row each, every one of them LIVE: -> (columns, capacity, probes) where
    probes = (conn_key [m], id [m*8] or None) holds every row's key and near misses of each."""
    base = np.array([0, 2**64 - 1, 0x10002711_9C40, 0x10002711_9C40 ^ (1 << 63), 0x10002711_9C40 ^ (1 << 32),
                     1, 1 << 32, 2**63, 2**64 - 2, 0xFFFFFFFF, 0xFFFFFFFF00000000], np.uint64)
    rng = np.random.default_rng(17)
    if by_id:
        ids = [bytes(8), bytes([255] * 8)] + [bytes([0] * b + [1] + [0] * (7 - b)) for b in range(8)]
        keys = np.repeat(base[:4], len(ids))
        idb = np.frombuffer(b"".join(ids) * 4, np.uint8).copy()
    else:
        keys, idb = base, None
    cap = len(keys)
    cols = random_columns(rng, cap, by_id=by_id)
    rows = rng.permutation(cap)
    place(cols, rows, keys, id=idb)
    # probes: every key, and each with one bit flipped (absent unless it is another row's key)
    pk = np.concatenate([keys] + [keys ^ np.uint64(1 << b) for b in (0, 31, 32, 63)])
    pid = None
    if by_id:
        flip = idb.reshape(-1, 8).copy()
        flip[:, 3] ^= 0x80
        pid = np.concatenate([idb] * 5 + [flip.ravel()])
        pk = np.concatenate([pk, keys])
    return cols, cap, (pk, pid)


# ---- constructed clusters (tests/collide.py) -------------------------------------------------------------------
# one run of the index as long as the table has rows, at the wave's edges, past one block of the build and the
# resolve; 2049 once per table kind
CLUSTER_LENGTHS = (63, 64, 65, 257, 1025)
CLUSTER_SHAPES = ("one_home", "two_homes", "duplicates")
CLUSTER_SHAPES_BY_ID = CLUSTER_SHAPES + ("one_key_many_ids",)
WRAP_HOME, INNER_HOME = -3, 5  # entry slots - 3 (the run crosses the table's end) and entry 5 (it does not)


def cluster_table(length, shape, by_id, wrap):
    """Every row UP, capacity = length, every key's probe starting at one entry H (two_homes: at H and H + 1 in
    turn), the rows in random order.  -> (cols, H, distinct keys, probes (conn_key, id words)): every present key,
    absent keys of the same home (their probe walks the whole run to the free entry behind it), of the
    neighbouring homes, and of an entry inside the run."""
    from tests import collide as X

    cap, home = length, (WRAP_HOME if wrap else INNER_HOME)
    rng = np.random.default_rng(length * 8 + by_id * 4 + wrap * 2 + CLUSTER_SHAPES_BY_ID.index(shape))
    cols = random_columns(rng, cap, by_id=by_id)
    id0 = 0x0123456789ABCDEF if by_id else 0
    ids = np.full(cap, id0, np.uint64)
    if shape == "one_key_many_ids":
        keys = np.full(cap, 0x10002711_9C40, np.uint64)
        ids = X.ids_at(home, cap, key=int(keys[0]))
    elif shape == "two_homes":
        keys = np.empty(cap, np.uint64)
        keys[0::2] = X.keys_at(home, (cap + 1) // 2, id0)
        keys[1::2] = X.keys_at(home + 1, cap // 2, id0, salt=1)
    else:
        keys = X.keys_at(home, cap, id0)
        if shape == "duplicates":  # a third of the rows repeat a key of the cluster
            rep = rng.permutation(cap)[: cap // 3]
            keys[rep] = keys[rng.integers(0, cap, len(rep))]
    order = rng.permutation(cap)
    keys, ids = keys[order], ids[order]
    place(cols, np.arange(cap), keys, id=ids.view(np.uint8) if by_id else None)
    distinct = len({(int(i), int(k)) for i, k in zip(ids, keys)})
    pk = [keys, X.keys_at(home, 8, id0, salt=7), X.keys_at(home - 1, 3, id0, salt=8), X.keys_at(home + 1, 3, id0, salt=9),
          X.keys_at(home + 2, 3, id0, salt=10), X.keys_at(home + cap - 1, 3, id0, salt=11), X.keys_at(home + cap, 3, id0, salt=12)]
    pi = [ids] + [np.full(len(k), id0, np.uint64) for k in pk[1:]]
    if by_id:  # a present key under an absent id of the same home, and under the neighbour's
        pk += [keys[:4], keys[:4]]
        pi += [X.ids_at(home, 4, salt=13, key=int(keys[0])), X.ids_at(home + 1, 4, salt=14, key=int(keys[0]))]
    return cols, home, distinct, (np.concatenate(pk), np.concatenate(pi))


def built_table(rc, cols, by_id, device, codec=None):
    """-> (ConnTable on `device` with its index built there, n_dup)."""
    import torch

    tab = make_table(rc, cols, len(cols["state"]), device, by_id=by_id)
    nd = torch.full((1,), -1, dtype=torch.int32, device=device)
    tab.rebuild(codec, n_dup=nd)
    if codec is not None:
        torch.cuda.synchronize()
    return tab, int(nd.cpu().numpy().view(np.uint32)[0])


def resolve_on(rc, tab, key, idb, device, codec=None):
    """The conn column of a resolve of all-VALID DATA packets, on the host twin or the device."""
    import torch

    status = np.ones(len(key), np.int8)
    if codec is None:
        return rc.conn_resolve_host(tab, status, key, id=idb)[0]
    t = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(dt)).to(device)  # noqa: E731
    conn = torch.zeros(len(key), dtype=torch.int32, device=device)
    codec.conn_resolve_batch(tab, t(status, np.int8), t(key, np.int64), conn, id=t(idb, np.uint8))
    torch.cuda.synchronize()
    return conn.cpu().numpy().view(np.uint32)


def check_index(tab, cols, by_id, what=""):
    """collide.index_invariant on the table's index as it stands."""
    from tests import collide as X

    cap = len(cols["state"])
    return X.index_invariant(tab.index.cpu().numpy(), cap, cols["state"], cols["conn_key"],
                             id_words(cols["id"], cap) if by_id else None, by_id, what=what)


def scenario_cluster(rc, length, shape, by_id, wrap, device, codec=None):
    """Build and resolve on a table that is one cluster: n_dup, the proof that the keys are one run from the
    predicted home, the index's contract, and every lookup against resolve_ref."""
    from tests import collide as X

    cols, home, distinct, (pk, pi) = cluster_table(length, shape, by_id, wrap)
    tab, ndup = built_table(rc, cols, by_id, device, codec)
    assert ndup == length - distinct, (ndup, length, distinct)
    X.one_run(tab.index.cpu().numpy(), home, distinct)
    assert check_index(tab, cols, by_id) == distinct
    tmap, _ = table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)
    idb = pi.view(np.uint8) if by_id else None
    want = resolve_ref(tmap, np.ones(len(pk), np.int8), pk, id=idb)[0]
    got = resolve_on(rc, tab, pk, idb, device, codec)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]
    assert bool((want[:length] != NONE).all()) and bool((want[length:] == NONE).all())
    return distinct
