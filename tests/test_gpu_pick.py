"""GPU: the send pick on the device (rsk_conn_pick_build, rsk_conn_pick_batch; include/rsk_codec.h) against
tests/pick_ref's rule_ref: the scenarios of tests/test_pick_host.py on the device (batch sizes and capacities,
group shapes, avoid keys, draws, the len gate, a pick index gone stale), the index built on either side, the
argument checks, the whole send chain down to verified wire packets, the control messages' resets, and a
captured graph.  The never-built (garbage) index runs on the host twins only."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from rsock_amd import workload
from tests import conn_ref as CR
from tests import conv_ref as VR
from tests import pick_ref as R

pytestmark = pytest.mark.gpu

KEY = b"hello135"
TABLES: dict = {}


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    TABLES.clear()
    c.close()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", R.CAPACITIES)
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes(cx, gpu, n, capacity, by_id):
    R.scenario_sizes(rc, n, capacity, by_id, gpu, cx, tables=TABLES)


@pytest.mark.parametrize("zero_real", [False, True])
def test_group_shapes(cx, gpu, zero_real):
    R.scenario_groups(rc, zero_real, gpu, cx)


@pytest.mark.parametrize("m", R.BIG_GROUPS)
def test_big_group(cx, gpu, m):
    R.scenario_big_group(rc, m, gpu, cx)


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("groups", [65, 1025])
def test_colliding_groups(cx, gpu, groups, wrap):
    """65 and 1025 groups whose entries in the pick index all probe from one entry (ids built by running the hash
    backwards, tests/collide.py): the build's lanes claim one run of entries, across the index's end, and every
    pick walks it; the avoid keys walk a run of the conn index as long as the table has rows."""
    assert R.scenario_colliding_groups(rc, groups, gpu, cx, wrap=wrap) > 4 * groups


@pytest.mark.parametrize("by_id", [False, True])
def test_avoid_keys(cx, gpu, by_id):
    R.scenario_avoid(rc, by_id, gpu, cx)


def test_seed_stream_and_coverage(cx, gpu):
    R.scenario_seed(rc, gpu, cx)


def test_len_gate_and_reads(cx, gpu):
    R.scenario_reads(rc, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
def test_stale_state(cx, gpu, by_id):
    """state changed without a rebuild: every value in the index is still a valid row, the picks stay inside
    the table; after the rebuild the rule holds."""
    R.scenario_stale_state(rc, by_id, gpu, cx)


def test_counts(cx, gpu):
    import torch

    cols, ids = R.grouped_table(True)
    tab = R.make_table(rc, cols, True, gpu, cx)
    counts = torch.full((2,), -1, dtype=torch.int32, device=gpu)
    tab.rebuild_pick(cx, counts=counts)
    torch.cuda.synchronize()
    assert u32(counts).tolist() == [len(R.GROUP_SIZES), sum(R.GROUP_SIZES)]
    ccols, _, derived = R.sized_table(65536, False)
    ctab = R.make_table(rc, ccols, False, gpu, cx)
    ctab.rebuild_pick(cx, counts=counts)
    torch.cuda.synchronize()
    assert u32(counts).tolist() == [1, len(derived[0][0])]


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [257, 65536])
def test_index_built_on_either_side(cx, gpu, capacity, by_id):
    """One layout: the host-built index copied to the device, and the device-built one copied to the host,
    give the picks of the index built in place."""
    import torch

    cols, pool, derived = R.sized_table(capacity, by_id)
    n = 4097
    b = R.random_batch(np.random.default_rng(21), cols, pool, by_id, n)
    want = R.rule_ref(cols, by_id, n, derived=derived, **b)
    host_tab = R.make_table(rc, cols, by_id, "cpu")
    dev_tab = R.make_table(rc, cols, by_id, gpu, cx)
    torch.cuda.synchronize()
    R.compare(R.run_pick(rc, host_tab.to(gpu), n, gpu, cx, **b), want, "host-built on the device")
    R.compare(R.run_pick(rc, dev_tab.to("cpu"), n, "cpu", **b), want, "device-built on the host")
    # cand and pos do not depend on which side built them (the groups' hash entries may)
    words = 4 + 2 * ((capacity + 3) & ~3)
    assert bool((dev_tab.pick[:words].cpu() == host_tab.pick[:words]).all())


def test_device_argument_errors_and_empty_batch(cx, gpu):
    R.check_einval(rc, gpu, cx)


# ---- the send chain ---------------------------------------------------------------------------------------
ETH = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])


def _server(rng, gpu, cx, groups=3, per=7):
    """A BY_ID conn table of `groups` IdBufs with `per` alive conns each (and a dead and a non-LIVE row each),
    rows interleaved; a conv table of four convs per IdBuf.  -> (conn cols, conn table, conv cols, conv table,
    id words)."""
    idw = rng.integers(1, 2**63, groups, dtype=np.uint64)
    cap = groups * (per + 2) + 3
    cols = CR.random_columns(rng, cap, by_id=True)
    rows = rng.permutation(cap)[: groups * (per + 2)].reshape(groups, per + 2)
    for g in range(groups):
        r = rows[g]
        sp = 40000 + np.arange(per + 2) + 100 * g
        cols["conn_key"][r] = (0x10000000 | (10001 << 16) | sp).astype(np.uint64)
        cols["sp"][r] = sp
        cols["id"].reshape(-1, 8)[r] = R.id_bytes(idw[g: g + 1])
        cols["state"][r] = R.UP
        cols["state"][r[per]] = A.CONN_LIVE
        cols["state"][r[per + 1]] = A.CONN_ALIVE
    cols["flag"][:] = 0x18
    tab = R.make_table(rc, cols, True, gpu, cx)
    vcap = 4 * groups
    vcols = VR.random_columns(rng, vcap, by_dst=True, by_id=True)
    vcols["state"][:] = A.CONN_LIVE
    vcols["id"][:] = R.id_bytes(np.repeat(idw, 4))
    vtab = VR.make_table(rc, vcols, gpu, True, True, cx)
    return cols, tab, vcols, vtab, idw


def _wire(cx, gpu, tab, conn, n, payload, pay_off, pay_len, cmd, conv, idcol, ipn):
    """expand -> send_seq -> encode_wire on the picked conns: -> (expand columns, ok, wire, woff, wst)."""
    import torch

    e = lambda dt, k=1: torch.empty(n * k, dtype=dt, device=gpu)  # noqa: E731
    x = {"src": e(torch.int32), "dst": e(torch.int32), "sp": e(torch.int16), "dp": e(torch.int16),
         "ack": e(torch.int32), "flag": e(torch.uint8), "conn_key": e(torch.int64), "id": e(torch.uint8, 8)}
    ok = e(torch.uint8)
    cx.conn_expand_batch(tab, conn, ok, **x)
    fst = 31 + pay_len.to(torch.int32)
    seq, ipid = e(torch.int32), e(torch.int16)
    cx.tcp_send_seq_batch(conn, fst, tab.seq, ipn, seq, ipid)
    wl = 54 + 31 + pay_len.cpu().numpy().astype(np.int64)
    woff = torch.from_numpy(np.concatenate([[0], np.cumsum(wl)[:-1]])).to(gpu)
    wire = torch.zeros(int(wl.sum()) + 64, dtype=torch.uint8, device=gpu)
    wst = e(torch.int32)
    cx.output_wire_batch(payload, pay_off, pay_len, cmd, conv, x["conn_key"], x["src"], x["dst"], x["sp"], x["dp"], seq,
                         x["ack"], x["flag"], ipid, wire, woff, wst, eth=ETH, id=idcol)
    torch.cuda.synchronize()
    assert np.array_equal(wst.cpu().numpy(), wl)
    return x, ok, wire, woff, wst


def test_send_chain_to_verified_wire(cx, gpu):
    """conv_send -> pick -> expand -> send_seq -> encode_wire on 2049 packets over a 3-group server table:
    every packet carries the TcpInfo and connKey of a candidate of its own IdBuf's group, and the checksum
    verification accepts every one of them."""
    import torch

    rng = np.random.default_rng(50)
    n = 2049
    cols, tab, vcols, vtab, idw = _server(rng, gpu, cx)
    d = workload.describe("c4", 0, n, n=n)
    w = workload.DeviceWorkload(d, gpu)
    conv_row = R.tensor(rng.integers(0, vtab.capacity, n).astype(np.uint32), gpu)
    conv, idcol = torch.empty(n, dtype=torch.int32, device=gpu), torch.empty(8 * n, dtype=torch.uint8, device=gpu)
    vok = torch.empty(n, dtype=torch.uint8, device=gpu)
    cx.conv_send_batch(vtab, conv_row, conv=conv, id=idcol, ok=vok)
    conn = torch.empty(n, dtype=torch.int32, device=gpu)
    nn = torch.empty(1, dtype=torch.int32, device=gpu)
    used = torch.zeros(tab.capacity, dtype=torch.uint8, device=gpu)
    cx.conn_pick_batch(tab, conn, len=w.pay_len.to(torch.int32) + 31, id=idcol, seed=77, n_none=nn, used=used)
    ipn = torch.zeros(1, dtype=torch.int16, device=gpu)
    x, ok, wire, woff, wst = _wire(cx, gpu, tab, conn, n, w.payload, w.pay_off, w.pay_len, w.cmd, conv, idcol, ipn)
    assert bool((vok == 1).all()) and bool((ok == 1).all()) and int(u32(nn)[0]) == 0
    groups = R.candidates(cols["state"], cols["id"], True)
    got, pid = u32(conn), CR.id_words(idcol.cpu().numpy(), n)
    assert np.array_equal(got, R.rule_ref(cols, True, n, id=idcol.cpu().numpy(), seed=77)[0])
    for g in idw.tolist():
        mine = got[pid == np.uint64(g)]
        assert mine.size > 0 and set(mine.tolist()) == set(groups[g].tolist())
    assert np.array_equal(np.nonzero(used.cpu().numpy())[0], np.unique(got))
    # what went onto the wire is the picked row's TcpInfo, connKey and IdBuf
    tcp, dec = rc.TcpInfoBuffers.alloc(n, gpu), rc.DecodeBuffers.alloc(n, gpu)
    cx.rawinput_batch(wire, woff, wst, wst, A.DLT_EN10MB, 0, tcp, dec)
    csum, nbad = torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(1, dtype=torch.int32, device=gpu)
    cx.verify_wire_batch(wire, woff, wst, A.DLT_EN10MB, csum, status=dec.status, status_out=dec.status, n_bad=nbad)
    torch.cuda.synchronize()
    assert int(nbad.item()) == 0 and bool((dec.status == 1).all())
    assert np.array_equal(dec.conn_key.cpu().numpy().view(np.uint64), cols["conn_key"][got])
    assert np.array_equal(CR.id_words(dec.id.cpu().numpy(), n), pid)
    # the parse gives the receiver's view: the sender's addresses and ports reversed
    for k, mine in (("src", "dst"), ("dst", "src")):
        assert np.array_equal(u32(getattr(tcp, k)), cols[mine][got]), k
    for k, mine in (("sp", "dp"), ("dp", "sp")):
        assert np.array_equal(getattr(tcp, k).cpu().numpy().view(np.uint16), cols[mine][got]), k


def test_control_resets_avoid_their_conn(cx, gpu):
    """KEEP_ALIVE_REQs for conns the table no longer has come out of rsk_control_batch as NETCONN_RSTs with
    their avoid_key; through the pick with the message columns as they stand, no reset travels on the conn
    it names, and every other message takes a candidate."""
    import torch

    rng = np.random.default_rng(51)
    cap, nconn = 12, 9
    rows = np.sort(rng.permutation(cap)[:nconn])
    sp = 40000 + np.arange(nconn)
    keys = (0x10000000 | (10001 << 16) | sp).astype(np.uint64)
    cols = CR.random_columns(rng, cap)
    CR.place(cols, rows, keys)
    lost = rows[[2, 6]]
    cols["state"][lost] = A.CONN_ALIVE  # no longer LIVE: a request naming them is a miss ...
    peer = {k: (None if v is None else v.copy()) for k, v in cols.items()}
    peer["state"][lost] = R.UP  # ... while the table that picks still has them, alive
    tab = CR.make_table(rc, cols, cap, gpu)
    tab.rebuild(cx)
    ptab = R.make_table(rc, peer, False, gpu, cx)
    n = 600  # requests: body = a conn key
    body = keys[rng.integers(0, nconn, n)]
    out = rc.ControlBuffers.alloc(n, gpu, capacity=cap)
    t = lambda a: R.tensor(a, gpu)  # noqa: E731
    cx.control_batch(tab, t(np.ones(n, np.int8)), t(np.full(n, A.CMD_KEEP_ALIVE_REQ, np.uint8)),
                     t(np.zeros(n, np.uint16)), t(np.full(n, 8, np.uint16)), t(body.view(np.uint8)),
                     t(8 * np.arange(n, dtype=np.uint64)), out)
    msgs = out.messages()
    k = len(msgs["cmd"])
    is_rst = msgs["cmd"] == A.CMD_NETCONN_RST
    assert k == n and 0 < int(is_rst.sum()) < n and np.array_equal(msgs["avoid_key"], np.where(is_rst, body, 0))
    conn = torch.empty(k, dtype=torch.int32, device=gpu)
    nn = torch.empty(1, dtype=torch.int32, device=gpu)
    cx.conn_pick_batch(ptab, conn, len=out.msg_pay_len[:k].to(torch.int32), id=out.msg_id[:8 * k],
                       avoid_key=out.msg_avoid_key[:k], seed=5, n_none=nn)
    torch.cuda.synchronize()
    got = u32(conn)
    want = R.rule_ref(peer, False, k, len=msgs["pay_len"].astype(np.int32), avoid_key=msgs["avoid_key"], seed=5)
    assert np.array_equal(got, want[0]) and int(u32(nn)[0]) == 0
    assert bool((peer["conn_key"][got][is_rst] != msgs["avoid_key"][is_rst]).all())
    assert set(got[is_rst].tolist()) == set(rows.tolist())  # the two named conns carry each other's resets
    assert set(got.tolist()) == set(rows.tolist())


def test_pick_expand_in_captured_graph(cx, gpu):
    """pick -> expand captured on a side stream (no reserve: neither call has scratch); replayed, then
    replayed after ALIVE was cleared on one row and the pick index rebuilt eagerly: the row is gone."""
    import torch

    rng = np.random.default_rng(52)
    n = 2049
    cols, tab, _vc, _vt, idw = _server(rng, gpu, cx)
    idcol = R.tensor(R.id_bytes(idw[rng.integers(0, idw.size, n)]), gpu)
    conn = torch.empty(n, dtype=torch.int32, device=gpu)
    nn = torch.empty(1, dtype=torch.int32, device=gpu)
    ok, nbad = torch.empty(n, dtype=torch.uint8, device=gpu), torch.empty(1, dtype=torch.int32, device=gpu)
    ckey = torch.empty(n, dtype=torch.int64, device=gpu)
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        cx.conn_pick_batch(tab, conn, id=idcol, seed=9, n_none=nn)  # loads the kernels ahead of the capture
        cx.conn_expand_batch(tab, conn, ok, conn_key=ckey, n_bad=nbad)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cxg.conn_pick_batch(tab, conn, id=idcol, seed=9, n_none=nn, stream=torch.cuda.current_stream())
            cxg.conn_expand_batch(tab, conn, ok, conn_key=ckey, n_bad=nbad, stream=torch.cuda.current_stream())
        gone = None
        for r in range(2):
            if r:
                gone = int(u32(conn)[0])
                tab.state[gone] = A.CONN_LIVE
                cols["state"][gone] = A.CONN_LIVE
                tab.rebuild_pick(cx)
            conn.fill_(0x5A5A5A5A)
            ok.fill_(0x5A)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = R.rule_ref(cols, True, n, id=idcol.cpu().numpy(), seed=9)
            assert np.array_equal(u32(conn), want[0]) and int(u32(nn)[0]) == 0, r
            assert bool((ok == 1).all()) and int(u32(nbad)[0]) == 0, r
            assert np.array_equal(ckey.cpu().numpy().view(np.uint64), cols["conn_key"][want[0]]), r
        assert gone is not None and not (u32(conn) == gone).any()
        del g
    finally:
        cxg.close()
