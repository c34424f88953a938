"""GPU: the connection table on the device (rsk_conn_index_build, rsk_conn_resolve_batch,
rsk_conn_expand_batch; include/rsk_codec.h) against tests/conn_ref: the reference's own per-packet
returns (tests/golden/demux.npz), the server shape with the missing pairs listed by rsk_demux_batch,
the index (a full table, key edge values, duplicates, rebuilds, host-built and device-built indices on
either side), the resolve mechanics over batch sizes and capacities, the expand, a send -> receive
round trip through the wire build and the parse, the device entry points' argument checks, and a
captured graph."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from rsock_amd import workload
from tests import conn_ref as R

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


def dev(a, gpu, dt=None):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dt) if dt is not None else a).to(gpu)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_table(cx, gpu, cols, capacity, by_id=False):
    """-> (ConnTable on the device with its index built there, n_dup)."""
    import torch

    tab = R.make_table(rc, cols, capacity, gpu, by_id=by_id)
    nd = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    tab.rebuild(cx, n_dup=nd)
    return tab, int(u32(nd)[0])


def resolve(cx, gpu, tab, status, conn_key, cmd=None, id=None, opt=(True, True, True), slack=3):
    """-> (conn, hit, miss, n_miss) on the host (None for an output not asked for); the outputs are
    `slack` entries longer than n and pre-filled, and nothing past n may be written."""
    import torch

    n = len(status)
    conn = torch.full((n + slack,), 0x6EEEEEEE, dtype=torch.int32, device=gpu)
    hit = torch.full((n + slack,), 0xEE, dtype=torch.uint8, device=gpu) if opt[0] else None
    miss = torch.full((n + slack,), 0x55, dtype=torch.int8, device=gpu) if opt[1] else None
    nm = torch.full((1,), -1, dtype=torch.int32, device=gpu) if opt[2] else None
    cx.conn_resolve_batch(tab, dev(status, gpu), dev(conn_key, gpu, np.int64), conn[:n], cmd=dev(cmd, gpu),
                          id=dev(id, gpu), hit=None if hit is None else hit[:n], miss=None if miss is None else miss[:n],
                          n_miss=nm)
    torch.cuda.synchronize()
    assert bool((conn[n:] == 0x6EEEEEEE).all())
    assert hit is None or bool((hit[n:] == 0xEE).all())
    assert miss is None or bool((miss[n:] == 0x55).all())
    h = lambda t: None if t is None else t[:n].cpu().numpy()  # noqa: E731
    return u32(conn[:n]), h(hit), h(miss), None if nm is None else int(u32(nm)[0])


def check_resolve(cx, gpu, tab, cols, status, conn_key, cmd=None, id=None, opt=(True, True, True)):
    tmap, _ = R.table_map(cols["state"], cols["conn_key"], cols["id"])
    want = R.resolve_ref(tmap, status, conn_key, cmd, id)
    got = resolve(cx, gpu, tab, status, conn_key, cmd, id, opt)
    for name, g, w in zip(("conn", "hit", "miss", "n_miss"), got, want):
        assert g is None or np.array_equal(g, w), name
    return got


# ---- 1. the reference pin ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.GOLDEN_CLIENT))
def test_reference_pin(cx, gpu, name):
    c, cols, key_row = R.golden_client_table(name)
    tab, ndup = dev_table(cx, gpu, cols, 257)
    assert ndup == 0
    conn, _hit, miss, n_miss = check_resolve(cx, gpu, tab, cols, c["status"], c["conn_key"], c["cmd"])
    R.check_golden_client(name, c, key_row, conn, miss)
    assert n_miss == R.GOLDEN_CLIENT[name][1]


# ---- 1b. constructed clusters ------------------------------------------------------------------------
def _clusters():
    from tests.test_conn_host import CLUSTERS

    return CLUSTERS


@pytest.mark.parametrize("length,shape,by_id,wrap", _clusters())
def test_constructed_cluster(cx, gpu, length, shape, by_id, wrap):
    """tests/test_conn_host.py's clusters on the device: up to 2049 lanes of one launch insert into one run of the
    index with compare-and-swap, across its end; n_dup, rsk_conn.h's contract on the index as the build left it
    (the occupied entries are a sequential insert's, so also the host twin's), and every lookup."""
    assert R.scenario_cluster(rc, length, shape, by_id, wrap, gpu, cx) > length // 2


# ---- 2. the server shape; the missing pairs through the demux ----------------------------------------
def test_server_shape_missing_pairs_by_demux(cx, gpu):
    import torch

    c, cols, cap = R.server_case()
    tab, ndup = dev_table(cx, gpu, cols, cap, by_id=True)
    assert ndup == 0
    n = len(c["status"])
    st, cmd, idb, key = dev(c["status"], gpu), dev(c["cmd"], gpu), dev(c["id"], gpu), dev(c["conn_key"], gpu, np.int64)
    conn = torch.empty(n, dtype=torch.int32, device=gpu)
    miss = torch.empty(n, dtype=torch.int8, device=gpu)
    cx.conn_resolve_batch(tab, st, key, conn, cmd=cmd, id=idb, miss=miss)
    dmx = rc.DemuxBuffers.alloc(n, gpu)
    cx.demux_batch(miss, cmd, A.DEMUX_ID | A.DEMUX_CONN_KEY, dmx, id=idb, conn_key=key)
    torch.cuda.synchronize()
    tmap, _ = R.table_map(cols["state"], cols["conn_key"], cols["id"])
    wconn, _whit, wmiss, wn = R.resolve_ref(tmap, c["status"], c["conn_key"], c["cmd"], c["id"])
    assert np.array_equal(u32(conn), wconn) and np.array_equal(miss.cpu().numpy(), wmiss)
    want = R.first_missing(wmiss, c["conn_key"], c["id"])
    ns = int(dmx.n_seg.item())
    assert 0 < len(want) < wn and ns == len(want) and int(dmx.n_valid.item()) == wn
    assert np.array_equal(u32(dmx.seg_first[:ns]), want)


# ---- 3. the index -------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [1, 64, 2048, 65536])
def test_full_table_present_and_absent(cx, gpu, capacity):
    rng = np.random.default_rng(capacity)
    cols = R.random_columns(rng, capacity)
    keys = rng.permutation(np.arange(capacity, dtype=np.uint64) * np.uint64(0x10001) + np.uint64(0x10000000))
    R.place(cols, np.arange(capacity), keys)
    tab, ndup = dev_table(cx, gpu, cols, capacity)
    assert ndup == 0
    probe = np.concatenate([keys, keys + np.uint64(1 << 40)])
    conn, _hit, _miss, n_miss = check_resolve(cx, gpu, tab, cols, np.ones(len(probe), np.int8), probe)
    assert np.array_equal(conn[:capacity], np.arange(capacity, dtype=np.uint32)) and n_miss == capacity


@pytest.mark.parametrize("by_id", [False, True])
def test_key_edges(cx, gpu, by_id):
    cols, cap, (pk, pid) = R.edge_table(by_id)
    tab, ndup = dev_table(cx, gpu, cols, cap, by_id=by_id)
    assert ndup == 0
    conn, hit, _miss, _n = check_resolve(cx, gpu, tab, cols, np.ones(len(pk), np.int8), pk, id=pid)
    assert bool((hit[:cap] == 1).all()) and 0 < int(hit[cap:].sum()) < len(pk) - cap


@pytest.mark.parametrize("capacity,n_keys", [(300, 40), (70000, 3), (4096, 1)])
def test_duplicates_lowest_row_wins(cx, gpu, capacity, n_keys):
    """Many rows per key, inserted by lanes of many waves and blocks at once: the lowest row wins and
    n_dup is exact (twice, so that a different arrival order shows)."""
    rng = np.random.default_rng(capacity)
    cols = R.random_columns(rng, capacity)
    keys = rng.integers(0, n_keys, capacity).astype(np.uint64)
    R.place(cols, np.arange(capacity), keys)
    cols["state"][rng.random(capacity) < 0.2] = A.CONN_ALIVE  # not LIVE
    cols["state"][:3] = 0  # the lowest rows of all are vacant
    live = (cols["state"] & A.CONN_LIVE) != 0
    for _ in range(2):
        tab, ndup = dev_table(cx, gpu, cols, capacity)
        assert ndup == int(live.sum()) - len(np.unique(keys[live])) > 0
        conn, _h, _m, _n = check_resolve(cx, gpu, tab, cols, np.ones(n_keys, np.int8), np.arange(n_keys, dtype=np.uint64))
        assert conn.tolist() == [int(np.nonzero(live & (keys == k))[0][0]) for k in range(n_keys)]


def test_state_changes_with_rebuild(cx, gpu):
    import torch

    rng = np.random.default_rng(4)
    cols = R.random_columns(rng, 16)
    R.place(cols, [3, 7], np.array([111, 222], np.uint64), state=A.CONN_LIVE)  # LIVE matches without ALIVE
    tab, _ = dev_table(cx, gpu, cols, 16)
    probe, st = np.array([111, 222], np.uint64), np.ones(2, np.int8)
    assert resolve(cx, gpu, tab, st, probe)[0].tolist() == [3, 7]
    tab.state[3] = 0
    tab.rebuild(cx)
    assert resolve(cx, gpu, tab, st, probe)[0].tolist() == [A.CONN_NONE, 7]
    tab.state[7], tab.state[12] = 0, A.CONN_LIVE
    tab.conn_key[12] = 222
    nd = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    tab.rebuild(cx, n_dup=nd)
    assert resolve(cx, gpu, tab, st, probe)[0].tolist() == [A.CONN_NONE, 12] and int(nd.item()) == 0


@pytest.mark.parametrize("by_id", [False, True])
def test_index_built_on_either_side_is_valid_on_the_other(cx, gpu, by_id):
    rng = np.random.default_rng(21)
    cap = 3000
    cols = R.random_columns(rng, cap, by_id=by_id)
    rows = rng.permutation(cap)[:2000]
    keys = rng.integers(0, 900, 2000).astype(np.uint64)  # duplicates too
    ids = np.repeat(rng.integers(0, 256, (4, 8), dtype=np.uint64).astype(np.uint8), 500, axis=0) if by_id else None
    R.place(cols, rows, keys, id=ids)
    probe = np.arange(1200, dtype=np.uint64)
    pid = np.tile(ids[::500], (300, 1)).ravel() if by_id else None
    st = np.ones(1200, np.int8)
    tmap, _ = R.table_map(cols["state"], cols["conn_key"], cols["id"])
    want = R.resolve_ref(tmap, st, probe, None, pid)[0]
    assert 0 < int((want != R.NONE).sum()) < 1200
    # built on the host, used on the device
    htab = R.make_table(rc, cols, cap, "cpu", by_id=by_id)
    htab.rebuild()
    up = htab.to(gpu)
    assert np.array_equal(resolve(cx, gpu, up, st, probe, id=pid)[0], want)
    # built on the device, used on the host
    dtab, _ = dev_table(cx, gpu, cols, cap, by_id=by_id)
    down = dtab.to("cpu")
    assert np.array_equal(rc.conn_resolve_host(down, st, probe, id=pid)[0], want)


# ---- 4. resolve mechanics -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mech_tables(cx, gpu):
    """One half-LIVE table per capacity, with the keys a batch draws from (present and absent ones)."""
    out = {}
    for cap in (1, 64, 2048, 65536):
        rng = np.random.default_rng(cap + 1)
        cols = R.random_columns(rng, cap)
        rows = rng.permutation(cap)[:max(1, cap // 2)]
        R.place(cols, rows, rng.integers(0, 2**62, len(rows), dtype=np.uint64), state=A.CONN_LIVE)
        pool = np.concatenate([cols["conn_key"][rows], rng.integers(0, 2**62, len(rows), dtype=np.uint64)])
        tab, _ = dev_table(cx, gpu, cols, cap)
        out[cap] = (tab, cols, pool)
    return out


@pytest.mark.parametrize("capacity", [1, 64, 2048, 65536])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 70000])
def test_resolve_sizes(cx, gpu, mech_tables, n, capacity):
    tab, cols, pool = mech_tables[capacity]
    rng = np.random.default_rng(n)
    st = rng.choice(np.array([1, 1, 1, 1, 0, -1], np.int8), n)
    cmd = np.where(rng.random(n) < 0.9, 0, rng.integers(1, 256, n)).astype(np.uint8)
    _c, _h, _m, n_miss = check_resolve(cx, gpu, tab, cols, st, pool[rng.integers(0, len(pool), n)], cmd)
    assert n < 64 or n_miss > 0


def test_resolve_optional_outputs_counts_and_empty_batch(cx, gpu, mech_tables):
    import torch

    tab, cols, pool = mech_tables[2048]
    rng = np.random.default_rng(8)
    n = 1000
    st, key = np.ones(n, np.int8), pool[rng.integers(0, len(pool), n)]
    for k in range(8):  # hit, miss, n_miss given or NULL in every combination; cmd NULL = all DATA
        check_resolve(cx, gpu, tab, cols, st, key, opt=(bool(k & 1), bool(k & 2), bool(k & 4)))
    # n_miss is written, not accumulated; n == 0 zeroes it
    nm = torch.full((1,), 1234, dtype=torch.int32, device=gpu)
    conn = torch.empty(n, dtype=torch.int32, device=gpu)
    dst, dkey = dev(st, gpu), dev(key, gpu, np.int64)
    want = R.resolve_ref(R.table_map(cols["state"], cols["conn_key"])[0], st, key)[3]
    for _ in range(2):
        cx.conn_resolve_batch(tab, dst, dkey, conn, n_miss=nm)
        assert int(nm.item()) == want > 0
    cx.conn_resolve_batch(tab, dst[:0], dkey[:0], conn[:0], n_miss=nm)
    assert int(nm.item()) == 0
    # the key fields of a packet that is not looked up do not matter
    st2 = st.copy()
    st2[::3] = -1
    a = resolve(cx, gpu, tab, st2, key)
    key2 = key.copy()
    key2[::3] = cols["conn_key"][np.nonzero(cols["state"])[0][0]]
    b = resolve(cx, gpu, tab, st2, key2)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]
    assert bool((a[0][::3] == A.CONN_NONE).all()) and bool((a[2][::3] == A.RECV_DROP).all())


# ---- 5. expand ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("n", [1, 64, 257, 5000])
def test_expand(cx, gpu, by_id, n):
    import torch

    rng = np.random.default_rng(12 + n)
    cap = 100
    cols = R.random_columns(rng, cap, by_id=by_id)
    cols["state"][:] = rng.choice([0, A.CONN_LIVE, A.CONN_ALIVE, R.UP, R.UP | 0x80], cap)
    tab = R.make_table(rc, cols, cap, gpu, by_id=by_id)  # the expand needs no index
    conn = rng.integers(0, cap, n).astype(np.uint32)
    odd = rng.random(n) < 0.15
    conn[odd] = rng.choice(np.array([A.CONN_NONE, cap, cap + 1, 2**31], np.uint32), int(odd.sum()))
    want, want_bad = R.expand_ref(cols, cap, conn)
    slack = 2
    fill = lambda dt, k=1: torch.full(((n + slack) * k,), 0x6E, dtype=dt, device=gpu)  # noqa: E731
    o = {"src": fill(torch.int32), "dst": fill(torch.int32), "sp": fill(torch.int16), "dp": fill(torch.int16),
         "ack": fill(torch.int32), "flag": fill(torch.uint8), "conn_key": fill(torch.int64),
         "id": fill(torch.uint8, 8) if by_id else None, "ok": fill(torch.uint8)}
    nb = torch.full((1,), 77, dtype=torch.int32, device=gpu)
    cut = lambda k: None if o[k] is None else o[k][:n * (8 if k == "id" else 1)]  # noqa: E731
    for _ in range(2):  # n_bad is written, not accumulated
        cx.conn_expand_batch(tab, dev(conn, gpu, np.int32), cut("ok"), n_bad=nb,
                             **{k: cut(k) for k in o if k != "ok"})
        torch.cuda.synchronize()
        assert int(nb.item()) == want_bad
    for k, w in want.items():
        got = o[k].cpu().numpy()
        m = n * (8 if k == "id" else 1)
        assert np.array_equal(got[:m].view(w.dtype), w), k
        assert bool((got[m:] == 0x6E).all()), k
    # ok alone; the empty batch zeroes n_bad
    ok = torch.full((n,), 0x6E, dtype=torch.uint8, device=gpu)
    cx.conn_expand_batch(tab, dev(conn, gpu, np.int32), ok)
    assert np.array_equal(ok.cpu().numpy(), want["ok"])
    cx.conn_expand_batch(tab, ok[:0].to(torch.int32), ok[:0], n_bad=nb)
    assert int(nb.item()) == 0


# ---- 6. send -> wire -> parse -> resolve: the round trip on the device -------------------------------
def test_round_trip_on_the_device(cx, gpu):
    import torch

    n, cap, nconn = 3000, 11, 8
    rng = np.random.default_rng(30)
    d = workload.describe("c4", 0, n, n=n)
    w = workload.DeviceWorkload(d, gpu)
    plen = d.pay_len.astype(np.int64)
    rows = np.sort(rng.permutation(cap)[:nconn])
    sp, dp = 40000 + np.arange(nconn), 10001 + np.arange(nconn) % 10
    keys = (0x10000000 | (dp << 16) | sp).astype(np.uint64)
    a_ip, b_ip = rc.ip_u32("10.0.0.1"), rc.ip_u32("10.0.0.2")
    send_cols = R.random_columns(rng, cap)
    R.place(send_cols, rows, keys)
    send_cols["src"][rows], send_cols["dst"][rows] = a_ip, b_ip
    send_cols["sp"][rows], send_cols["dp"][rows] = sp, dp
    send_cols["seq"][rows] = rng.integers(0, 2**30, nconn)
    send_cols["flag"][rows] = 0x18
    recv_cols = {k: (None if v is None else v.copy()) for k, v in send_cols.items()}
    recv_cols["src"][rows], recv_cols["dst"][rows] = b_ip, a_ip  # the peer's view of the same conns
    recv_cols["sp"][rows], recv_cols["dp"][rows] = dp, sp
    recv_cols["ack"][:] = 0
    snd, _ = dev_table(cx, gpu, send_cols, cap)
    rcv, _ = dev_table(cx, gpu, recv_cols, cap)
    conn_h = rows[rng.integers(0, nconn, n)].astype(np.uint32)
    conn = dev(conn_h, gpu, np.int32)
    e = lambda dt: torch.empty(n, dtype=dt, device=gpu)  # noqa: E731
    # 1. expand
    x = {"src": e(torch.int32), "dst": e(torch.int32), "sp": e(torch.int16), "dp": e(torch.int16),
         "ack": e(torch.int32), "flag": e(torch.uint8), "conn_key": e(torch.int64)}
    ok, nb = e(torch.uint8), torch.empty(1, dtype=torch.int32, device=gpu)
    cx.conn_expand_batch(snd, conn, ok, n_bad=nb, **x)
    # 2. seq and IP id from the table's seq column
    fst = dev(31 + plen, gpu).to(torch.int32)
    ipn = torch.zeros(1, dtype=torch.int16, device=gpu)
    seq, ipid = e(torch.int32), e(torch.int16)
    cx.tcp_send_seq_batch(conn, fst, snd.seq, ipn, seq, ipid)
    # 3. Ethernet packets, back to back
    wl = 54 + 31 + plen
    woff = dev(np.concatenate([[0], np.cumsum(wl)[:-1]]), gpu)
    wire = torch.zeros(int(wl.sum()) + 64, dtype=torch.uint8, device=gpu)
    wst = e(torch.int32)
    eth = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
    cmd0 = torch.zeros(n, dtype=torch.uint8, device=gpu)
    cx.output_wire_batch(w.payload, w.pay_off, w.pay_len, cmd0, w.conv, x["conn_key"], x["src"], x["dst"], x["sp"],
                         x["dp"], seq, x["ack"], x["flag"], ipid, wire, woff, wst, eth=eth, id_uniform=workload.ID_UNIFORM)
    # 4. filter + parse + decode, 5. checksums, 6. resolve at the peer, 7. its ack
    tcp, dec = rc.TcpInfoBuffers.alloc(n, gpu), rc.DecodeBuffers.alloc(n, gpu)
    match = e(torch.uint8)
    cx.filter_rawinput_batch(wire, woff, wst, wst, A.DLT_EN10MB, 0, rc.make_filter(dst_ip="10.0.0.2"), match, tcp, dec)
    csum, nbad = e(torch.uint8), torch.empty(1, dtype=torch.int32, device=gpu)
    cx.verify_wire_batch(wire, woff, wst, A.DLT_EN10MB, csum, status=dec.status, status_out=dec.status, n_bad=nbad)
    rconn, hit, nm = e(torch.int32), e(torch.uint8), torch.empty(1, dtype=torch.int32, device=gpu)
    cx.conn_resolve_batch(rcv, dec.status, dec.conn_key, rconn, cmd=dec.cmd, hit=hit, n_miss=nm)
    cx.tcp_recv_ack_batch(rconn, hit, tcp.seq, rcv.ack)
    torch.cuda.synchronize()
    assert int(nb.item()) == 0 and bool((ok == 1).all()) and bool((match == 1).all())
    assert np.array_equal(wst.cpu().numpy(), wl) and int(nbad.item()) == 0 and bool((dec.status == 1).all())
    assert bool((hit == 1).all()) and int(nm.item()) == 0 and np.array_equal(u32(rconn), conn_h)
    # the parsed addresses are the peer row's own (self view: src = ip_dst)
    assert np.array_equal(u32(tcp.src), recv_cols["src"][conn_h]) and np.array_equal(u32(tcp.dst), recv_cols["dst"][conn_h])
    assert np.array_equal(tcp.sp.cpu().numpy().view(np.uint16), recv_cols["sp"][conn_h])
    adv = np.bincount(conn_h, weights=31 + plen, minlength=cap).astype(np.uint64)
    assert np.array_equal(u32(snd.seq), ((send_cols["seq"] + adv) & 0xFFFFFFFF).astype(np.uint32))
    pseq = u32(tcp.seq)
    want_ack = np.zeros(cap, np.uint32)
    np.maximum.at(want_ack, conn_h, pseq)
    assert np.array_equal(u32(rcv.ack), want_ack) and bool((want_ack[rows] > 0).all())


# ---- 7. the device entry points' own argument checks ---------------------------------------------------
def test_device_argument_errors(cx, gpu):
    """The checks the host twins do not have (alignment of the index and of the IdBuf columns, the batch
    limit, the NULL ctx) and a sample of the shared ones; no kernel runs for a refused call."""
    import ctypes

    import torch

    L = rc.lib()
    rng = np.random.default_rng(2)
    cols = R.random_columns(rng, 4, by_id=True)
    R.place(cols, [1], np.array([9], np.uint64), id=np.arange(8, dtype=np.uint8))
    tab, _ = dev_table(cx, gpu, cols, 4, by_id=True)
    st, key = torch.ones(3, dtype=torch.int8, device=gpu), torch.full((3,), 9, dtype=torch.int64, device=gpu)
    idb = torch.zeros(40, dtype=torch.uint8, device=gpu)
    conn, ok = torch.full((3,), 7, dtype=torch.int32, device=gpu), torch.full((3,), 7, dtype=torch.uint8, device=gpu)
    s = torch.cuda.current_stream().cuda_stream
    rin = lambda off=0: A.ConnResolveIn(st.data_ptr(), None, idb.data_ptr() + off, key.data_ptr())  # noqa: E731
    rout = A.ConnResolveOut(conn.data_ptr(), None, None, None)
    eout = lambda off=0: A.ConnExpandOut(*([None] * 7), idb.data_ptr() + off, ok.data_ptr(), None)  # noqa: E731
    build = lambda c, t: L.rsk_conn_index_build(c, ctypes.byref(t), None, s)  # noqa: E731
    resolve = lambda c, t, r, n=3: L.rsk_conn_resolve_batch(c, ctypes.byref(t), n, ctypes.byref(r), ctypes.byref(rout), s)  # noqa: E731
    expand = lambda c, t, e, n=3: L.rsk_conn_expand_batch(c, ctypes.byref(t), n, conn.data_ptr(), ctypes.byref(e), s)  # noqa: E731
    ctx = cx._ctx
    assert build(ctx, tab.abi()) == A.OK and resolve(ctx, tab.abi(), rin()) == A.OK
    conn.fill_(0)
    assert expand(ctx, tab.abi(), eout()) == A.OK
    conn.fill_(7)
    ok.fill_(7)
    assert build(None, tab.abi()) == A.EINVAL and resolve(None, tab.abi(), rin()) == A.EINVAL
    assert expand(None, tab.abi(), eout()) == A.EINVAL
    t = tab.abi()
    t.index += 4
    assert build(ctx, t) == A.EINVAL
    t = tab.abi()
    t.id += 4
    assert build(ctx, t) == A.EINVAL and resolve(ctx, t, rin()) == A.EINVAL and expand(ctx, t, eout()) == A.EINVAL
    assert resolve(ctx, tab.abi(), rin(4)) == A.EINVAL and expand(ctx, tab.abi(), eout(4)) == A.EINVAL
    assert resolve(ctx, tab.abi(), rin(), n=A.MAX_BATCH + 1) == A.EINVAL
    assert expand(ctx, tab.abi(), eout(), n=A.MAX_BATCH + 1) == A.EINVAL
    for field, val in (("flags", 3), ("capacity", 0), ("capacity", A.CONN_MAX_ROWS + 1), ("conn_key", None)):
        t = tab.abi()
        setattr(t, field, val)
        assert build(ctx, t) == A.EINVAL and resolve(ctx, t, rin()) == A.EINVAL, field
    torch.cuda.synchronize()
    assert bool((conn == 7).all()) and bool((ok == 7).all())  # nothing ran


# ---- 8. captured graph --------------------------------------------------------------------------------
def test_resolve_in_captured_graph(cx, gpu):
    """A resolve captured on a side stream of a fresh context, with no reserve: replayed, then replayed
    again after a row was edited and the index rebuilt -- the second replay reflects the edit.  (The
    eager calls on the module's context first only make sure the kernels' code object is loaded.)"""
    import torch

    rng = np.random.default_rng(40)
    cols = R.random_columns(rng, 64)
    R.place(cols, np.arange(0, 64, 2), np.arange(100, 132, dtype=np.uint64))
    tab, _ = dev_table(cx, gpu, cols, 64)
    n = 500
    key_h = rng.integers(95, 140, n).astype(np.uint64)
    st_h = np.ones(n, np.int8)
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        st, key = dev(st_h, gpu), dev(key_h, gpu, np.int64)
        conn = torch.empty(n, dtype=torch.int32, device=gpu)
        hit = torch.empty(n, dtype=torch.uint8, device=gpu)
        miss = torch.empty(n, dtype=torch.int8, device=gpu)
        nm = torch.empty(1, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cxg.conn_resolve_batch(tab, st, key, conn, hit=hit, miss=miss, n_miss=nm, stream=torch.cuda.current_stream())
        for r in range(2):
            if r:  # key 100 leaves row 0; key 139 arrives at the vacant row 1
                tab.state[0] = 0
                tab.conn_key[1], tab.state[1] = 139, R.UP
                tab.rebuild(cx)
                cols["state"][0], cols["conn_key"][1], cols["state"][1] = 0, 139, R.UP
            conn.fill_(0x6EEEEEEE)
            nm.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = R.resolve_ref(R.table_map(cols["state"], cols["conn_key"])[0], st_h, key_h)
            assert np.array_equal(u32(conn), want[0]) and np.array_equal(hit.cpu().numpy(), want[1]), r
            assert np.array_equal(miss.cpu().numpy(), want[2]) and int(nm.item()) == want[3], r
        assert bool((want[0][key_h == 100] == R.NONE).all()) and bool((want[0][key_h == 139] == 1).all())
        assert (key_h == 100).any() and (key_h == 139).any()
        del g
    finally:
        cxg.close()
