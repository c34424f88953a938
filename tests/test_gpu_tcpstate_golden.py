"""GPU: rsk_tcp_send_seq_batch, rsk_tcp_recv_ack_batch and the send chain on an rsk_conn_table (recv_ack ->
rsk_conn_expand_batch -> rsk_tcp_send_seq_batch(tab.seq) -> rsk_encode_wire_batch) against what the REFERENCE's
own FakeTcp / INetConn / RConn / RawTcp did with the same scripts: tests/golden/tcpstate.npz, read through
tests/tcpstate_golden.py, whose scripts tests/test_tcpstate_golden.py runs on the oracle.  Only the fixture is
read here.  Every comparison is integer- or byte-exact."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_ref as CR
from tests import tcpstate_golden as G
from tests.test_gpu_verify import WIRE_PATHS

pytestmark = pytest.mark.gpu

ETH = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
PITCH, FIRST = 176, 3  # wire slots: 14 + 40 + 31 + 64 bytes fit; packets start at odd addresses
CHAIN_SCRIPTS = G.names("mixed") + ["send_k7_rr_frames", "send_k64_random_frames"]


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(G.KEY, 0)
    yield c
    c.close()


def dev(a, gpu, dt=None):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dt) if dt is not None else a).to(gpu)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def u16(t):
    return t.cpu().numpy().view(np.uint16)


# ---- 1. rsk_tcp_send_seq_batch ------------------------------------------------------------------------
@pytest.mark.parametrize("groupby", [0, 1, 2])
@pytest.mark.parametrize("name", G.names("send"))
def test_send_seq_equals_the_reference(cx, gpu, name, groupby):
    """Every send script, batch after batch on device state: seq / ip_id of the framed packets equal the
    recorded libnet_build_tcp seq / libnet_build_ipv4 id, conn_seq equals mInfo.seq and ip_id_next mIpId after
    every batch; a rejected frame gets 0 / 0 and moves neither (include/rsk_codec.h)."""
    import torch

    s = G.script(name)
    seq0, _ = G.init_rows(s)
    d_cs = dev(seq0, gpu, np.int32)
    d_ipn = dev(np.array([s["ip_id0"]], np.uint16), gpu, np.int16)
    try:
        cx.set_send_seq_groupby(groupby)
        for lo, hi, kind in G.batches(s):
            assert kind == G.SEND
            n = hi - lo
            status = G.status_of(s, lo, hi)
            seq = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
            ipid = torch.full((n,), 0x5A5A, dtype=torch.int16, device=gpu)
            cx.tcp_send_seq_batch(dev(s["conn"][lo:hi], gpu, np.int32), dev(status, gpu), d_cs, d_ipn, seq, ipid)
            torch.cuda.synchronize()
            sent = status > 0
            assert np.array_equal(u32(seq)[sent], s["t_seq"][lo:hi][sent]), (lo, hi)
            assert np.array_equal(u16(ipid)[sent], s["i_id"][lo:hi][sent]), (lo, hi)
            assert bool((u32(seq)[~sent] == 0).all()) and bool((u16(ipid)[~sent] == 0).all()), (lo, hi)
            assert np.array_equal(u32(d_cs), G.state_after(s, hi, "conn_seq", seq0)), (lo, hi)
            assert int(u16(d_ipn)[0]) == int(s["ip_id_next"][hi - 1]), (lo, hi)
    finally:
        cx.set_send_seq_groupby(0)


# ---- 2. rsk_tcp_recv_ack_batch ------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.names("recv"))
def test_recv_ack_equals_the_reference(cx, gpu, name):
    """Every receive script with delivered = (recorded return >= 0): conn_ack equals the recorded mInfo.ack after
    every batch.  Packets of conn ids >= K are mixed in on the device side only (the reference has no such
    packet): they change nothing."""
    import torch

    s = G.script(name)
    k = len(s["key"])
    _, ack0 = G.init_rows(s)
    d_ack = dev(ack0, gpu, np.int32)
    rng = np.random.default_rng(k)
    for lo, hi, kind in G.batches(s):
        assert kind == G.RECV
        n = hi - lo
        m = n + max(n // 10, 3)
        at = np.sort(rng.permutation(m)[:n])  # where the script's packets sit among the strangers
        conn = rng.choice(np.array([k, k + 1, 2 * k + 7, 0xFFFFFFFF], np.uint32), m)
        dl = np.ones(m, np.uint8)
        seq = np.full(m, 0xFFFFFFFF, np.uint32)
        conn[at], dl[at], seq[at] = s["conn"][lo:hi], s["ret"][lo:hi] >= 0, s["a"][lo:hi]
        cx.tcp_recv_ack_batch(dev(conn, gpu, np.int32), dev(dl, gpu), dev(seq, gpu, np.int32), d_ack)
        torch.cuda.synchronize()
        assert np.array_equal(u32(d_ack), G.state_after(s, hi, "conn_ack", ack0)), (lo, hi)


# ---- 3. the send chain on a connection table ----------------------------------------------------------
def make_table(cx, gpu, s, seed):
    """The script's conns at scattered rows of a larger table, every row initialised by INTEGRATION.md's rule
    (tests/tcpstate_golden.init_rows); the other rows hold random values and are not LIVE."""
    k = len(s["key"])
    cap = k + 5
    rng = np.random.default_rng(seed)
    rows = rng.permutation(cap)[:k]
    cols = CR.random_columns(rng, cap)
    CR.place(cols, rows, s["key"])
    info = s["info"]
    for col, name in enumerate(("src", "dst", "sp", "dp")):
        cols[name][rows] = info[:, col]
    cols["flag"][rows] = info[:, 6]
    cols["seq"][rows], cols["ack"][rows] = G.init_rows(s)
    tab = CR.make_table(rc, cols, cap, gpu)
    tab.rebuild(cx)
    return tab, rows.astype(np.uint32)


class Recv:
    """Device columns of one receive batch of at most n packets; unused slots are not delivered."""

    def __init__(self, gpu, n):
        import torch

        self.n = n
        self.conn = torch.zeros(n, dtype=torch.int32, device=gpu)
        self.dl = torch.zeros(n, dtype=torch.uint8, device=gpu)
        self.seq = torch.zeros(n, dtype=torch.int32, device=gpu)

    def fill(self, s, lo, hi, rows):
        pad = self.n - (hi - lo)
        z = lambda a, dt: np.concatenate([a, np.zeros(pad, a.dtype)]).view(dt)  # noqa: E731
        gpu = self.conn.device
        self.conn.copy_(dev(z(rows[s["conn"][lo:hi]], np.int32), gpu))
        self.dl.copy_(dev(z((s["ret"][lo:hi] >= 0).astype(np.uint8), np.uint8), gpu))
        self.seq.copy_(dev(z(s["a"][lo:hi], np.int32), gpu))

    def run(self, cx, tab, stream=None):
        cx.tcp_recv_ack_batch(self.conn, self.dl, self.seq, tab.ack, stream=stream)


class Send:
    """Device columns of one send batch of at most n packets and its wire ring; unused slots have no payload
    (status RSK_SEND_RESET: nothing is sent)."""

    def __init__(self, gpu, n, s):
        import torch

        e = lambda dt, k=1: torch.zeros(n * k, dtype=dt, device=gpu)  # noqa: E731
        self.n, self.gpu = n, gpu
        self.payload = dev(np.concatenate([s["arena"], np.zeros(64, np.uint8)]), gpu)
        self.conn, self.status, self.conv = e(torch.int32), e(torch.int32), e(torch.int32)
        self.pay_off, self.pay_len, self.cmd = e(torch.int64), e(torch.int16), e(torch.uint8)
        self.x = {"src": e(torch.int32), "dst": e(torch.int32), "sp": e(torch.int16), "dp": e(torch.int16),
                  "ack": e(torch.int32), "flag": e(torch.uint8), "conn_key": e(torch.int64)}
        self.ok, self.seq, self.ipid, self.wst = e(torch.uint8), e(torch.int32), e(torch.int16), e(torch.int32)
        self.woff = torch.arange(n, device=gpu, dtype=torch.int64) * PITCH + FIRST
        self.wire = torch.zeros(n * PITCH + 64, dtype=torch.uint8, device=gpu)
        self.id8 = s["id8"].tobytes()

    def fill(self, s, lo, hi, rows):
        pad = self.n - (hi - lo)
        z = lambda a, dt: np.concatenate([a, np.zeros(pad, a.dtype)]).view(dt)  # noqa: E731
        nread = s["a"][lo:hi]
        self.conn.copy_(dev(z(rows[s["conn"][lo:hi]], np.int32), self.gpu))
        self.status.copy_(dev(z(G.status_of(s, lo, hi), np.int32), self.gpu))
        self.conv.copy_(dev(z(s["conv"][lo:hi], np.int32), self.gpu))
        self.pay_off.copy_(dev(z(s["pay_off"][lo:hi], np.int64), self.gpu))
        self.pay_len.copy_(dev(z(nread.astype(np.uint16), np.int16), self.gpu))
        self.wire.fill_(0xA5)
        self.wst.fill_(0x5A5A5A5A)

    def run(self, cx, tab, ipn, eth, stream=None):
        x = self.x
        cx.conn_expand_batch(tab, self.conn, self.ok, stream=stream, **x)
        cx.tcp_send_seq_batch(self.conn, self.status, tab.seq, ipn, self.seq, self.ipid, stream=stream)
        cx.output_wire_batch(self.payload, self.pay_off, self.pay_len, self.cmd, self.conv, x["conn_key"], x["src"],
                             x["dst"], x["sp"], x["dp"], self.seq, x["ack"], x["flag"], self.ipid, self.wire, self.woff,
                             self.wst, eth=ETH if eth else None, id_uniform=self.id8, stream=stream)

    def check(self, s, lo, hi, eth):
        """Every packet's IPv4 / TCP header fields against the recorded libnet arguments, the bytes behind the
        headers against the recorded frame, both checksums; rejected and unused slots wrote nothing."""
        n = hi - lo
        L = 14 if eth else 0
        assert bool((self.ok[:n] == 1).all())
        status = G.status_of(s, lo, hi)
        sent = status > 0
        wst = self.wst.cpu().numpy()
        assert np.array_equal(wst[:n], np.where(sent, L + 40 + status, A.SEND_OVERSIZE))
        assert bool((wst[n:] == A.SEND_RESET).all())
        ring = self.wire.cpu().numpy()
        slots = ring[FIRST:FIRST + self.n * PITCH].reshape(self.n, PITCH)
        assert bool((ring[:FIRST] == 0xA5).all()) and bool((ring[FIRST + self.n * PITCH:] == 0xA5).all())
        used = np.zeros(self.n, np.int64)
        used[:n] = np.where(sent, wst[:n], 0)
        assert bool((slots[np.arange(PITCH)[None, :] >= used[:, None]] == 0xA5).all())
        idx = lo + np.nonzero(sent)[0]
        mine = slots[:n][sent]
        if eth:
            assert np.array_equal(mine[:, :14], np.broadcast_to(np.frombuffer(ETH, np.uint8), (len(mine), 14)))
        G.check_packets(s, idx, mine[:, L:], wst[:n][sent].astype(np.int64) - L)
        return len(idx)


def check_state(s, hi, tab, rows, ipn):
    seq0, ack0 = G.init_rows(s)
    assert np.array_equal(u32(tab.seq)[rows], G.state_after(s, hi, "conn_seq", seq0)), hi
    assert np.array_equal(u32(tab.ack)[rows], G.state_after(s, hi, "conn_ack", ack0)), hi
    assert int(u16(ipn)[0]) == int(s["ip_id_next"][hi - 1]), hi


@pytest.mark.parametrize("eth", [False, True], ids=["raw4", "eth"])
@pytest.mark.parametrize("wpath", WIRE_PATHS, ids=["perset", "two_pass_k1", "two_pass_k2", "two_pass_k4"])
@pytest.mark.parametrize("name", CHAIN_SCRIPTS)
def test_send_chain_equals_the_reference(cx, gpu, name, wpath, eth):
    """The script's batches in order on one table, the wire build held to one path: what goes onto the wire
    carries the reference's seq, ack (as the preceding receive batch left it), IP id, addresses, ports, flags
    and constants, and behind the headers the reference's frame (connKey stamped, tag, payload)."""
    import torch

    s = G.script(name)
    tab, rows = make_table(cx, gpu, s, seed=len(name))
    ipn = dev(np.array([s["ip_id0"]], np.uint16), gpu, np.int16)
    n_checked = 0
    try:
        cx.set_encode_path(wpath[0])
        cx.set_copy_k(wpath[1])
        for lo, hi, kind in G.batches(s):
            if kind == G.RECV:
                b = Recv(gpu, hi - lo)
                b.fill(s, lo, hi, rows)
                b.run(cx, tab)
            else:
                b = Send(gpu, hi - lo, s)
                b.fill(s, lo, hi, rows)
                b.run(cx, tab, ipn, eth)
                took = (cx.last_encode_path, cx.last_copy_k if wpath[0] == 2 else 0)
                assert took == wpath, f"wire build held to {wpath} ran {took}"
                torch.cuda.synchronize()
                n_checked += b.check(s, lo, hi, eth)
            torch.cuda.synchronize()
            check_state(s, hi, tab, rows, ipn)
    finally:
        cx.set_encode_path(0)
        cx.set_copy_k(0)
    assert n_checked > 150


# ---- 4. the chain replayed from a captured graph ------------------------------------------------------
def test_send_chain_in_captured_graph(gpu):
    """mixed_k64_frames: recv_ack -> expand -> send_seq (the per-tile table path: 69 rows) -> encode_wire captured
    once on a reserved side stream, a linear chain, and replayed for each of the script's three receive / send
    batch pairs with the inputs rewritten in place; the table and the IP id counter advance on the device from
    replay to replay."""
    import torch

    s = G.script("mixed_k64_frames")
    pairs = G.batches(s)
    n_recv = max(hi - lo for lo, hi, k in pairs if k == G.RECV)
    n_send = max(hi - lo for lo, hi, k in pairs if k == G.SEND) + 2  # two unused slots in every replay
    cx = rc.Codec(G.KEY, 0)
    try:
        tab, rows = make_table(cx, gpu, s, seed=1)
        ipn = dev(np.array([s["ip_id0"]], np.uint16), gpu, np.int16)
        keep = (tab.seq.clone(), tab.ack.clone(), ipn.clone())
        st = torch.cuda.Stream(gpu)
        cx.reserve(max(n_recv, n_send), stream=st)
        r, w = Recv(gpu, n_recv), Send(gpu, n_send, s)
        r.fill(s, *pairs[0][:2], rows)
        w.fill(s, *pairs[1][:2], rows)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):  # eager once: the kernels are loaded and the stream's scratch exists
            r.run(cx, tab, stream=st)
            w.run(cx, tab, ipn, True, stream=st)
        torch.cuda.synchronize()
        w.check(s, *pairs[1][:2], True)
        tab.seq.copy_(keep[0])
        tab.ack.copy_(keep[1])
        ipn.copy_(keep[2])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            r.run(cx, tab, stream=torch.cuda.current_stream())
            w.run(cx, tab, ipn, True, stream=torch.cuda.current_stream())
        n_checked = 0
        for (rlo, rhi, _), (slo, shi, _) in zip(pairs[0::2], pairs[1::2]):
            r.fill(s, rlo, rhi, rows)
            w.fill(s, slo, shi, rows)
            torch.cuda.synchronize()
            with torch.cuda.stream(st):
                g.replay()
            torch.cuda.synchronize()
            n_checked += w.check(s, slo, shi, True)
            check_state(s, shi, tab, rows, ipn)
        assert n_checked > 150 and cx.check_device_errors() == 0
        del g
    finally:
        cx.close()
