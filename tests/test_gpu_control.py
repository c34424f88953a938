"""GPU: rsk_control_batch and rsk_keepalive_flush on the device (include/rsk_codec.h) against
tests/control_ref: the scenarios of tests/test_control_host.py on the device (golden batches with
synthetic frames, snapshot against the per-packet walk, batch sizes and capacities, optional outputs,
the miss option, TCP_CLOSE, the timer), a keepalive round trip between two peers' tables through the
wire build and the parse, a captured graph, and the device entry points' argument checks."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from rsock_amd import workload
from tests import conn_ref as R
from tests import control_ref as C

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", C.GOLDEN_NAMES)
def test_golden_classification(cx, gpu, name):
    C.scenario_golden(rc, name, gpu, cx)


def test_snapshot_against_sequential(cx, gpu):
    C.scenario_sequential(rc, gpu, cx)


@pytest.mark.parametrize("capacity", C.CAPACITIES)
@pytest.mark.parametrize("n", C.SIZES)
def test_sizes(cx, gpu, n, capacity):
    C.scenario_sizes(rc, n, capacity, gpu, cx)


@pytest.mark.parametrize("n", [257, 4097])
def test_sizes_by_id(cx, gpu, n):
    got, _ = C.scenario_sizes(rc, n, 257, gpu, cx, by_id=True)
    assert (got["conn"] != C.NONE).any()


def test_extremes(cx, gpu):
    C.scenario_extremes(rc, gpu, cx)


def test_optional_outputs(cx, gpu):
    C.scenario_optional_outputs(rc, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
def test_miss_option(cx, gpu, by_id):
    C.scenario_miss(rc, gpu, cx, by_id=by_id)


def test_tcp_close(cx, gpu):
    C.scenario_tcp_close(rc, gpu, cx)


@pytest.mark.parametrize("max_retry", [1, 3])
@pytest.mark.parametrize("capacity", [1, 1000, 65536])
def test_flush_steps(cx, gpu, capacity, max_retry):
    C.scenario_flush_steps(rc, capacity, max_retry, gpu, cx, by_id=capacity == 1000)


def test_flush_edges(cx, gpu):
    C.scenario_flush_edges(rc, gpu, cx)


def test_counts_are_written_not_accumulated(cx, gpu):
    import torch

    rng = np.random.default_rng(9)
    c, cols, cap = C.random_batch(rng, 3000, ctrl=0.3)
    tab = C.table_on(rc, cols, cap, False, gpu, cx)
    want = C.snapshot_ref(c, R.table_map(cols["state"], cols["conn_key"])[0], cap, False)
    t = lambda a, dt=None: C.tensor(a, gpu, dt)  # noqa: E731
    out = rc.ControlBuffers.alloc(3000, gpu, capacity=cap)
    args = (tab, t(c["status"]), t(c["cmd"]), t(c["pay_off"], np.int16), t(c["pay_len"], np.int16), t(c["arena"]),
            t(c["base_off"], np.int64), out)
    for _ in range(2):
        cx.control_batch(*args, inner_off=t(c["inner_off"], np.int16))
        torch.cuda.synchronize()
        assert int(u32(out.n_msg)[0]) == want["n_msg"] > 0 and int(u32(out.n_ctl)[0]) == want["n_ctl"] > 0
    # the empty batch zeroes the counts and fills rst_first
    out.rst_first.fill_(5)
    e = t(c["status"])[:0]
    cx.control_batch(tab, e, e.view(torch.uint8), None, None, None, None, out)
    torch.cuda.synchronize()
    assert int(u32(out.n_msg)[0]) == 0 and int(u32(out.n_ctl)[0]) == 0 and bool((u32(out.rst_first) == C.NO_RST).all())


# ---- the round trip: timer -> wire -> the peer's control pass -> wire -> this side's control pass ---------
def _send(cx, gpu, tab, conn, payload, pay_off, pay_len, cmd, ipn):
    """expand -> send_seq -> Ethernet packets back to back: -> (wire, wire_off, wire_len)."""
    import torch

    n = conn.numel()
    e = lambda dt: torch.empty(n, dtype=dt, device=gpu)  # noqa: E731
    x = {"src": e(torch.int32), "dst": e(torch.int32), "sp": e(torch.int16), "dp": e(torch.int16),
         "ack": e(torch.int32), "flag": e(torch.uint8), "conn_key": e(torch.int64)}
    ok = e(torch.uint8)
    cx.conn_expand_batch(tab, conn, ok, **x)
    fst = (31 + pay_len.to(torch.int32))
    seq, ipid = e(torch.int32), e(torch.int16)
    cx.tcp_send_seq_batch(conn, fst, tab.seq, ipn, seq, ipid)
    wl = 54 + 31 + pay_len.cpu().numpy().astype(np.int64)
    woff = torch.from_numpy(np.concatenate([[0], np.cumsum(wl)[:-1]])).to(gpu)
    wire = torch.zeros(int(wl.sum()) + 64, dtype=torch.uint8, device=gpu)
    wst = e(torch.int32)
    eth = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
    conv = torch.zeros(n, dtype=torch.int32, device=gpu)
    cx.output_wire_batch(payload, pay_off, pay_len, cmd, conv, x["conn_key"], x["src"], x["dst"], x["sp"], x["dp"], seq,
                         x["ack"], x["flag"], ipid, wire, woff, wst, eth=eth, id_uniform=workload.ID_UNIFORM)
    torch.cuda.synchronize()
    assert bool((ok == 1).all()) and np.array_equal(wst.cpu().numpy(), wl)
    return wire, woff, wst


def _receive(cx, gpu, tab, wire, woff, wst, dst_ip, tries):
    """filter + parse -> verify -> resolve -> control: -> (ControlBuffers, decode buffers)."""
    import torch

    n = wst.numel()
    e = lambda dt: torch.empty(n, dtype=dt, device=gpu)  # noqa: E731
    tcp, dec = rc.TcpInfoBuffers.alloc(n, gpu), rc.DecodeBuffers.alloc(n, gpu)
    match, csum, nbad = e(torch.uint8), e(torch.uint8), torch.empty(1, dtype=torch.int32, device=gpu)
    cx.filter_rawinput_batch(wire, woff, wst, wst, A.DLT_EN10MB, 0, rc.make_filter(dst_ip=dst_ip), match, tcp, dec)
    cx.verify_wire_batch(wire, woff, wst, A.DLT_EN10MB, csum, status=dec.status, status_out=dec.status, n_bad=nbad)
    conn, miss = e(torch.int32), e(torch.int8)
    cx.conn_resolve_batch(tab, dec.status, dec.conn_key, conn, cmd=dec.cmd, miss=miss)
    out = rc.ControlBuffers.alloc(n, gpu, capacity=tab.capacity)
    cx.control_batch(tab, dec.status, dec.cmd, dec.pay_off, dec.pay_len, wire, woff, out, id=dec.id,
                     conn_key=dec.conn_key, inner_off=tcp.cap_pay_off, tcp_sp=tcp.sp, tcp_dp=tcp.dp, miss=miss,
                     ka_tries=tries)
    torch.cuda.synchronize()
    assert bool((match == 1).all()) and int(nbad.item()) == 0 and bool((dec.status == 1).all())
    return out, dec, miss


def test_keepalive_round_trip(cx, gpu):
    import torch

    n, cap, nconn = 3000, 11, 8
    rng = np.random.default_rng(30)
    rows = np.sort(rng.permutation(cap)[:nconn])
    sp, dp = 40000 + np.arange(nconn), 10001 + np.arange(nconn) % 10
    keys = (0x10000000 | (dp << 16) | sp).astype(np.uint64)
    a_ip, b_ip = rc.ip_u32("10.0.0.1"), rc.ip_u32("10.0.0.2")
    a_cols = R.random_columns(rng, cap)
    R.place(a_cols, rows, keys)
    a_cols["src"][rows], a_cols["dst"][rows], a_cols["sp"][rows], a_cols["dp"][rows] = a_ip, b_ip, sp, dp
    a_cols["flag"][rows] = 0x18
    b_cols = {k: (None if v is None else v.copy()) for k, v in a_cols.items()}
    b_cols["src"][rows], b_cols["dst"][rows], b_cols["sp"][rows], b_cols["dp"][rows] = b_ip, a_ip, dp, sp
    lost = int(rows[5])
    b_cols["state"][lost] = 0  # the peer no longer has this conn
    ta, tb = (C.table_on(rc, cols, cap, False, gpu, cx) for cols in (a_cols, b_cols))
    tries_a = torch.full((cap,), A.KA_NONE, dtype=torch.uint8, device=gpu)
    tries_b = torch.full((cap,), A.KA_NONE, dtype=torch.uint8, device=gpu)
    est = torch.zeros(cap, dtype=torch.int64, device=gpu)
    now = 10**9
    ipn = torch.zeros(1, dtype=torch.int16, device=gpu)
    # 1. the timer at A: one request per conn
    fl = rc.ControlBuffers.alloc(0, gpu, capacity=cap, m=cap)
    cx.keepalive_flush(ta, tries_a, est, now, fl, max_retry=1)
    req = fl.messages()
    m = len(req["cmd"])
    assert m == nconn and np.array_equal(req["src"], rows.astype(np.uint32)) and np.array_equal(req["body"], keys)
    assert int(fl.n_dead.item()) == 0 and tries_a.cpu().numpy()[rows].tolist() == [0] * nconn
    # 2. A sends them among DATA packets: the message columns are the encode's inputs as they stand
    d = workload.describe("c4", 0, n - m, n=n - m)
    w = workload.DeviceWorkload(d, gpu)
    conn_h = np.concatenate([req["src"], rows[rng.integers(0, nconn, n - m)].astype(np.uint32)])
    payload = torch.cat([fl.msg_body[:m].view(torch.uint8), w.payload])
    pay_off = torch.cat([fl.msg_pay_off[:m], w.pay_off + 8 * m])
    pay_len = torch.cat([fl.msg_pay_len[:m], w.pay_len])
    cmd = torch.cat([fl.msg_cmd[:m], torch.zeros(n - m, dtype=torch.uint8, device=gpu)])
    wire, woff, wst = _send(cx, gpu, ta, C.tensor(conn_h, gpu, np.int32), payload, pay_off, pay_len, cmd, ipn)
    # 3. B: the requests come back as responses; the conn B lacks is answered with a reset naming it
    out_b, dec_b, miss_b = _receive(cx, gpu, tb, wire, woff, wst, "10.0.0.2", tries_b)
    kind = out_b.kind.cpu().numpy()
    assert kind[:m].tolist() == [A.CTL_KA_REQ] * m and not kind[m:].any()
    ans = out_b.messages()
    n_lost_data = int((conn_h[m:] == lost).sum())
    assert len(ans["cmd"]) == m + n_lost_data and int(miss_b.eq(1).sum()) == n_lost_data > 0
    is_req = ans["src"] < m
    assert np.array_equal(ans["body"][is_req], keys)
    want_cmd = np.where(rows == lost, A.CMD_NETCONN_RST, A.CMD_KEEP_ALIVE_RESP)
    assert np.array_equal(ans["cmd"][is_req], want_cmd)
    assert np.array_equal(ans["avoid_key"][is_req], np.where(rows == lost, keys, 0))
    lost_key = keys[5]
    assert bool((ans["cmd"][~is_req] == A.CMD_NETCONN_RST).all()) and bool((ans["avoid_key"][~is_req] == lost_key).all())
    assert np.array_equal(ans["id"], np.tile(np.frombuffer(workload.ID_UNIFORM, np.uint8), (len(ans["cmd"]), 1)))
    # 4. B sends the answers: a response on its own conn, a reset on a conn that is not the one it names
    k = m  # the per-packet resets of the DATA packets add nothing here
    pick = np.where(rows == lost, rows[0], rows).astype(np.uint32)
    wire2, woff2, wst2 = _send(cx, gpu, tb, C.tensor(pick, gpu, np.int32), out_b.msg_body[:k].view(torch.uint8),
                               out_b.msg_pay_off[:k], out_b.msg_pay_len[:k], out_b.msg_cmd[:k], ipn)
    # 5. A: the responses clear the pending requests; the reset finds the conn it names
    out_a, _dec, _miss = _receive(cx, gpu, ta, wire2, woff2, wst2, "10.0.0.1", tries_a)
    kind = out_a.kind.cpu().numpy()
    assert kind.tolist() == [A.CTL_NETCONN_RST if r == lost else A.CTL_KA_RESP for r in rows]
    assert np.array_equal(u32(out_a.conn), rows.astype(np.uint32)) and int(out_a.n_msg.item()) == 0
    rst = u32(out_a.rst_first)
    assert rst[lost] == 5 and int((rst != C.NO_RST).sum()) == 1
    t = tries_a.cpu().numpy()
    assert t[lost] == 0 and bool((t[rows[rows != lost]] == A.KA_NONE).all())
    # 6. the next tick: no timeout for the answered conns, one for the conn nobody answered for
    cx.keepalive_flush(ta, tries_a, est, now + 1000, fl, max_retry=1)
    torch.cuda.synchronize()
    assert u32(fl.dead_rows)[:int(fl.n_dead.item())].tolist() == [lost]
    assert np.array_equal(fl.messages()["src"], rows[rows != lost].astype(np.uint32))


def test_control_in_captured_graph(cx, gpu):
    """A control pass captured on a side stream of a fresh context after a reserve; replayed, then
    replayed after a row edit and a rebuild: the second replay sees the edit."""
    import torch

    rng = np.random.default_rng(40)
    n = 5000
    c, cols, cap = C.random_batch(rng, n, ctrl=0.3)
    tab = C.table_on(rc, cols, cap, False, gpu, cx)
    t = lambda a, dt=None: C.tensor(a, gpu, dt)  # noqa: E731
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        cxg.reserve(n, stream=s)
        out = rc.ControlBuffers.alloc(n, gpu, capacity=cap)
        tries = torch.zeros(cap, dtype=torch.uint8, device=gpu)
        args = (tab, t(c["status"]), t(c["cmd"]), t(c["pay_off"], np.int16), t(c["pay_len"], np.int16), t(c["arena"]),
                t(c["base_off"], np.int64), out)
        kw = dict(inner_off=t(c["inner_off"], np.int16), ka_tries=tries)
        cx.control_batch(*args, **kw)  # on the module's context: only loads the kernels ahead of the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cxg.control_batch(*args, stream=torch.cuda.current_stream(), **kw)
        hit_row = None
        for r in range(2):
            if r:  # the conn of the first request that hit leaves the table
                got_conn = u32(out.conn)
                i = int(np.nonzero((out.kind.cpu().numpy() == A.CTL_KA_REQ) & (got_conn != C.NONE))[0][0])
                hit_row = int(got_conn[i])
                tab.state[hit_row] = 0
                tab.rebuild(cx)
                cols["state"][hit_row] = 0
            for f in ("kind", "arg", "conn", "n_ctl", "n_msg", "rst_first", "msg_cmd"):
                getattr(out, f).view(torch.uint8).fill_(C.SENT)
            tries.zero_()
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want = C.snapshot_ref(c, R.table_map(cols["state"], cols["conn_key"])[0], cap, False, np.zeros(cap, np.uint8))
            assert np.array_equal(out.kind.cpu().numpy(), want["kind"]) and np.array_equal(u32(out.conn), want["conn"]), r
            assert int(u32(out.n_msg)[0]) == want["n_msg"] and int(u32(out.n_ctl)[0]) == want["n_ctl"], r
            assert np.array_equal(u32(out.rst_first), want["rst_first"]) and np.array_equal(tries.cpu().numpy(), want["ka_tries"]), r
            for name, a in out.messages().items():
                assert np.array_equal(a, want["msgs"][name]), (r, name)
        assert hit_row is not None and not (want["conn"] == hit_row).any()
        del g
    finally:
        cxg.close()


def test_device_argument_errors(cx, gpu):
    """Every RSK_EINVAL of the two device entry points, the alignment checks the host twins do not have
    included; no kernel runs for a refused call."""
    import torch

    L = rc.lib()
    client, server, keep, a = C.einval_fixture(rc, gpu)
    for t in (client, server):
        t.rebuild(cx)
    s = torch.cuda.current_stream().cuda_stream
    ctx = cx._ctx
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    ok, bad = C.control_einval_cases(client, server, a)
    for label, t, n, i, o in ok:
        assert L.rsk_control_batch(ctx, ref(t), n, ref(i), ref(o), s) == A.OK, label
    torch.cuda.synchronize()
    assert keep["kind"].tolist() == [0, 0, 0]
    keep["kind"].fill_(7)
    _, t, n, i, o = ok[0]
    assert L.rsk_control_batch(None, ref(t), n, ref(i), ref(o), s) == A.EINVAL
    for label, t, n, i, o in bad:
        assert L.rsk_control_batch(ctx, ref(t), n, ref(i), ref(o), s) == A.EINVAL, label
    # unaligned IdBuf columns: the batch's, the table's (BY_ID), the messages'
    _, t, n, i, o = ok[1]
    i.id += 4
    assert L.rsk_control_batch(ctx, ref(t), n, ref(i), ref(o), s) == A.EINVAL
    i.id -= 4
    t.id += 4
    assert L.rsk_control_batch(ctx, ref(t), n, ref(i), ref(o), s) == A.EINVAL
    t.id -= 4
    o.msgs.id, o.msgs.n_msg = a["id"] + 4, a["word"]
    assert L.rsk_control_batch(ctx, ref(t), n, ref(i), ref(o), s) == A.EINVAL
    fok, fbad = C.flush_einval_cases(client, a)
    for label, t, k, o in fok:
        assert L.rsk_keepalive_flush(ctx, ref(t), ref(k), ref(o), s) == A.OK, label
    _, t, k, o = fok[0]
    assert L.rsk_keepalive_flush(None, ref(t), ref(k), ref(o), s) == A.EINVAL
    for label, t, k, o in fbad:
        assert L.rsk_keepalive_flush(ctx, ref(t), ref(k), ref(o), s) == A.EINVAL, label
    _, t, k, o = C.flush_einval_cases(server, a)[0][0]
    o.msgs.id, o.msgs.n_msg = a["id"] + 4, a["word"]
    assert L.rsk_keepalive_flush(ctx, ref(t), ref(k), ref(o), s) == A.EINVAL
    torch.cuda.synchronize()
    assert keep["kind"].tolist() == [7, 7, 7] and int(keep["word"][0]) == 7 and keep["dead"].tolist() == [7] * 4
