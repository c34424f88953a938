"""CPU: the host twins of the connection table (rsk_conn_index_build_host, rsk_conn_resolve_host,
rsk_conn_expand_host; include/rsk_codec.h) against tests/conn_ref, pinned to the reference's own
per-packet returns (tests/golden/demux.npz: INetGroup::ERR_NO_CONN), and every RSK_EINVAL case of the
three entry points.  The device kernels share the hash and the probe rule with these
(rsock_amd/csrc/rsk_conn.h); tests/test_gpu_conn.py checks them."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_ref as R


def host_table(cols, capacity, by_id=False):
    tab = R.make_table(rc, cols, capacity, "cpu", by_id=by_id)
    nd = np.full(1, 0xFFFFFFFF, np.uint32)
    rcode = rc.lib().rsk_conn_index_build_host(ctypes.byref(tab.abi()), nd.ctypes.data, 1)
    assert rcode == A.OK
    return tab, int(nd[0])


def check_resolve(tab, cols, status, conn_key, cmd=None, id=None, nthreads=1):
    tmap, _ = R.table_map(cols["state"], cols["conn_key"], cols["id"])
    want = R.resolve_ref(tmap, status, conn_key, cmd, id)
    got = rc.conn_resolve_host(tab, status, conn_key, cmd=cmd, id=id, nthreads=nthreads)
    for name, g, w in zip(("conn", "hit", "miss"), got, want):
        assert np.array_equal(g, w), name
    assert got[3] == want[3]
    return got


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CLIENT))
def test_host_reference_pin(name):
    c, cols, key_row = R.golden_client_table(name)
    tab, ndup = host_table(cols, 257)
    assert ndup == 0
    conn, _hit, miss, n_miss = check_resolve(tab, cols, c["status"], c["conn_key"], c["cmd"], nthreads=4)
    n_ctrl = R.check_golden_client(name, c, key_row, conn, miss)
    assert n_miss == R.GOLDEN_CLIENT[name][1]
    if name == "client_large":
        assert n_ctrl >= 6 and len(np.setdiff1d(np.unique(c["conn_key"]), c["known_keys"])) == 2


def test_host_server_shape():
    c, cols, cap = R.server_case()
    tab, ndup = host_table(cols, cap, by_id=True)
    assert ndup == 0
    conn, hit, miss, n_miss = check_resolve(tab, cols, c["status"], c["conn_key"], c["cmd"], c["id"])
    assert 0 < n_miss < int(hit.sum())
    assert 0 < len(R.first_missing(miss, c["conn_key"], c["id"])) < n_miss


@pytest.mark.parametrize("capacity", [1, 64, 2048, 65536])
def test_host_full_table_present_and_absent(capacity):
    """Every row LIVE: lookups of all present keys and as many absent ones end and are right."""
    rng = np.random.default_rng(capacity)
    cols = R.random_columns(rng, capacity)
    keys = rng.permutation(np.arange(capacity, dtype=np.uint64) * np.uint64(0x10001) + np.uint64(0x10000000))
    R.place(cols, np.arange(capacity), keys)
    tab, ndup = host_table(cols, capacity)
    assert ndup == 0
    probe = np.concatenate([keys, keys + np.uint64(1 << 40)])
    conn, hit, _miss, n_miss = check_resolve(tab, cols, np.ones(len(probe), np.int8), probe, nthreads=4)
    assert np.array_equal(conn[:capacity], np.arange(capacity, dtype=np.uint32)) and n_miss == capacity


@pytest.mark.parametrize("by_id", [False, True])
def test_host_key_edges(by_id):
    cols, cap, (pk, pid) = R.edge_table(by_id)
    tab, ndup = host_table(cols, cap, by_id=by_id)
    assert ndup == 0
    conn, hit, _miss, _n = check_resolve(tab, cols, np.ones(len(pk), np.int8), pk, id=pid)
    assert bool((hit[:cap] == 1).all()) and 0 < int(hit[cap:].sum()) < len(pk) - cap
    assert np.array_equal(cols["conn_key"][conn[:cap]], pk[:cap])


def test_host_duplicates_lowest_row_wins():
    rng = np.random.default_rng(9)
    cap = 300
    cols = R.random_columns(rng, cap)
    keys = rng.integers(0, 40, cap).astype(np.uint64)  # 40 distinct keys over 300 rows
    R.place(cols, np.arange(cap), keys)
    cols["state"][rng.random(cap) < 0.2] = A.CONN_ALIVE  # not LIVE: not in the index, not a duplicate
    tab, ndup = host_table(cols, cap)
    live = (cols["state"] & A.CONN_LIVE) != 0
    assert ndup == int(live.sum()) - len(np.unique(keys[live])) > 0
    conn, _h, _m, _n = check_resolve(tab, cols, np.ones(40, np.int8), np.arange(40, dtype=np.uint64))
    for k in range(40):
        assert conn[k] == np.nonzero(live & (keys == k))[0][0]


CLUSTERS = ([(n, shape, by_id, True) for n in R.CLUSTER_LENGTHS for by_id in (False, True)
             for shape in (R.CLUSTER_SHAPES_BY_ID if by_id else R.CLUSTER_SHAPES)] +
            [(65, "one_home", False, False), (257, "two_homes", True, False), (1025, "duplicates", False, False),
             (2049, "one_home", False, True), (2049, "one_key_many_ids", True, True)])


@pytest.mark.parametrize("length,shape,by_id,wrap", CLUSTERS)
def test_host_constructed_cluster(length, shape, by_id, wrap):
    """A table whose keys all probe from one entry (tests/collide.py): a run as long as the table has rows, across
    the index's end and inside it; n_dup, rsk_conn.h's contract on the index, and every lookup."""
    assert R.scenario_cluster(rc, length, shape, by_id, wrap, "cpu") > length // 2


def test_host_state_changes_with_rebuild():
    rng = np.random.default_rng(4)
    cols = R.random_columns(rng, 16)
    R.place(cols, [3, 7], np.array([111, 222], np.uint64), state=A.CONN_LIVE)  # LIVE matches without ALIVE
    tab, _ = host_table(cols, 16)
    probe, st = np.array([111, 222], np.uint64), np.ones(2, np.int8)
    assert rc.conn_resolve_host(tab, st, probe)[0].tolist() == [3, 7]
    tab.state[3] = 0
    tab.rebuild()
    assert rc.conn_resolve_host(tab, st, probe)[0].tolist() == [A.CONN_NONE, 7]
    tab.state[7], tab.state[12], tab.conn_key[12] = 0, A.CONN_LIVE, 222  # the key moves to another row
    tab.rebuild()
    assert rc.conn_resolve_host(tab, st, probe)[0].tolist() == [A.CONN_NONE, 12]


def test_host_not_looked_up_packets_never_read_their_keys():
    """A packet that is not VALID DATA gets NONE / 0 / DROP whatever its key fields hold."""
    rng = np.random.default_rng(6)
    cols = R.random_columns(rng, 8)
    R.place(cols, [2], np.array([5], np.uint64))
    tab, _ = host_table(cols, 8)
    st = np.array([1, 1, 0, -1, 1], np.int8)
    cmd = np.array([0, 3, 0, 0, 255], np.uint8)
    conn, hit, miss, n_miss = rc.conn_resolve_host(tab, st, np.full(5, 5, np.uint64), cmd=cmd)
    assert conn.tolist() == [2] + [A.CONN_NONE] * 4 and hit.tolist() == [1, 0, 0, 0, 0]
    assert miss.tolist() == [A.RECV_DROP] * 5 and n_miss == 0


@pytest.mark.parametrize("by_id", [False, True])
def test_host_expand(by_id):
    rng = np.random.default_rng(12)
    cap = 100
    cols = R.random_columns(rng, cap, by_id=by_id)
    cols["state"][:] = rng.choice([0, A.CONN_LIVE, A.CONN_ALIVE, R.UP, R.UP | 0x80], cap)
    tab = R.make_table(rc, cols, cap, "cpu", by_id=by_id)
    conn = rng.integers(0, cap, 5000).astype(np.uint32)
    odd = rng.random(5000) < 0.1
    conn[odd] = rng.choice(np.array([A.CONN_NONE, cap, cap + 1, 2**31], np.uint32), int(odd.sum()))
    want, want_bad = R.expand_ref(cols, cap, conn)
    got, n_bad = rc.conn_expand_host(tab, conn, nthreads=4)
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k]), k
    assert n_bad == want_bad and 0 < n_bad < 5000
    dead = (conn < cap) & ((cols["state"][np.minimum(conn, cap - 1)] & R.UP) != R.UP)
    assert dead.any() and bool((got["ok"][dead] == 0).all()) and bool((got["src"][dead] == 0).all())


def test_host_argument_errors_and_empty_batch():
    L = rc.lib()
    rng = np.random.default_rng(2)
    cols = R.random_columns(rng, 4, by_id=True)
    R.place(cols, [1], np.array([9], np.uint64), id=np.arange(8, dtype=np.uint8))
    client = R.make_table(rc, {k: v for k, v in cols.items() if k != "id"}, 4, "cpu")
    server = R.make_table(rc, cols, 4, "cpu", by_id=True)
    st, key, idb = np.ones(3, np.int8), np.full(3, 9, np.uint64), np.zeros(24, np.uint8)
    conn, nm = np.zeros(3, np.uint32), np.full(1, 7, np.uint32)
    ok = np.zeros(3, np.uint8)

    def build(t):
        return L.rsk_conn_index_build_host(ctypes.byref(t) if t else None, None, 1)

    def resolve(t, rin, rout, n=3):
        return L.rsk_conn_resolve_host(ctypes.byref(t) if t else None, n, ctypes.byref(rin) if rin else None,
                                       ctypes.byref(rout) if rout else None, 1)

    def expand(t, eout, n=3, c=conn):
        return L.rsk_conn_expand_host(ctypes.byref(t) if t else None, n, c.ctypes.data if c is not None else None,
                                      ctypes.byref(eout) if eout else None, 1)

    rin = lambda: A.ConnResolveIn(st.ctypes.data, None, idb.ctypes.data, key.ctypes.data)  # noqa: E731
    rout = lambda: A.ConnResolveOut(conn.ctypes.data, None, None, nm.ctypes.data)  # noqa: E731
    eout = lambda: A.ConnExpandOut(None, None, None, None, None, None, None, None, ok.ctypes.data, nm.ctypes.data)  # noqa: E731
    for tab in (client, server):
        assert build(tab.abi()) == A.OK and resolve(tab.abi(), rin(), rout()) == A.OK and expand(tab.abi(), eout()) == A.OK
        # unknown flags, capacity out of range
        for field, val in (("flags", tab.flags | 2), ("flags", 0x80000000), ("capacity", 0),
                           ("capacity", A.CONN_MAX_ROWS + 1)):
            t = tab.abi()
            setattr(t, field, val)
            assert build(t) == A.EINVAL and resolve(t, rin(), rout()) == A.EINVAL and expand(t, eout()) == A.EINVAL, field
        # a NULL in a required table column
        for field in ("state", "conn_key", "index"):
            t = tab.abi()
            setattr(t, field, None)
            assert build(t) == A.EINVAL, field
            assert resolve(t, rin(), rout()) == (A.OK if field == "state" else A.EINVAL), field
        t = tab.abi()
        t.state = None
        assert expand(t, eout()) == A.EINVAL
        # NULL structs, NULL required batch columns
        assert build(None) == A.EINVAL and resolve(None, rin(), rout()) == A.EINVAL and expand(None, eout()) == A.EINVAL
        assert resolve(tab.abi(), None, rout()) == A.EINVAL and resolve(tab.abi(), rin(), None) == A.EINVAL
        assert expand(tab.abi(), None) == A.EINVAL and expand(tab.abi(), eout(), c=None) == A.EINVAL
        for field in ("status", "conn_key"):
            r = rin()
            setattr(r, field, None)
            assert resolve(tab.abi(), r, rout()) == A.EINVAL, field
        o = rout()
        o.conn = None
        assert resolve(tab.abi(), rin(), o) == A.EINVAL
        e = eout()
        e.ok = None
        assert expand(tab.abi(), e) == A.EINVAL
        # an index that is not 16-B aligned
        t = tab.abi()
        t.index += 4
        assert build(t) == A.EINVAL
    # id missing with BY_ID: in the table, in the batch
    t = server.abi()
    t.id = None
    assert build(t) == A.EINVAL and resolve(t, rin(), rout()) == A.EINVAL
    r = rin()
    r.id = None
    assert resolve(server.abi(), r, rout()) == A.EINVAL and resolve(client.abi(), r, rout()) == A.OK
    # an output column the table does not have
    e = eout()
    e.id = idb.ctypes.data
    assert expand(client.abi(), e) == A.EINVAL and expand(server.abi(), e) == A.OK
    # the empty batch zeroes the counts and may pass null arrays
    nm[0] = 7
    assert resolve(client.abi(), A.ConnResolveIn(None, None, None, None), A.ConnResolveOut(None, None, None, nm.ctypes.data),
                   n=0) == A.OK and nm[0] == 0
    nm[0] = 7
    assert expand(client.abi(), A.ConnExpandOut(*([None] * 9), nm.ctypes.data), n=0, c=None) == A.OK and nm[0] == 0
    assert L.rsk_conn_index_bytes(0, 0) == 0 and L.rsk_conn_index_bytes(A.CONN_MAX_ROWS + 1, 0) == 0
    assert L.rsk_conn_index_bytes(4, 2) == 0 and L.rsk_conn_index_bytes(1, 0) == 16
    assert L.rsk_conn_index_bytes(A.CONN_MAX_ROWS, A.CONN_BY_ID) == 8 * A.CONN_MAX_ROWS
    assert L.rsk_conn_index_bytes(1000, 0) == 4 * 2048 and L.rsk_conn_index_bytes(1024, 0) == 4 * 2048


def test_struct_layouts_match_header(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = {"rsk_conn_table": A.ConnTable, "rsk_conn_resolve_in": A.ConnResolveIn,
         "rsk_conn_resolve_out": A.ConnResolveOut, "rsk_conn_expand_out": A.ConnExpandOut}
    body = "".join(f'printf("{t} %zu\\n", sizeof({t}));' +
                   "".join(f'printf("{t}.{f} %zu\\n", offsetof({t}, {f}));' for f, _ in c._fields_) for t, c in m.items())
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsk_codec.h"\nint main(void){' + body + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if not ln.strip():
            continue
        k, v = ln.split()
        if "." in k:
            t, f = k.split(".")
            assert getattr(m[t], f).offset == int(v), k
        else:
            assert ctypes.sizeof(m[k]) == int(v), k
