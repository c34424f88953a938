"""CPU: the fake-TCP connection state (orc_tcp_send_seq_batch / orc_tcp_recv_ack_batch, the Python walk of
tests/test_tcpstate_oracle.py) and the wire build's field values (orc_build_wire) against what the REFERENCE's
own FakeTcp / INetConn / RConn / RawTcp did: tests/golden/tcpstate.npz, read through tests/tcpstate_golden.py.
Everything is integer- and byte-exact."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from tests import tcpstate_golden as G
from tests.oracle_lib import ref_available, ref_tcpstate_available
from tests.test_tcpstate_oracle import py_send

ETH = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])


def test_fixture_covers_the_shapes():
    """The scripts hold the sizes at which the kernels change path, three batches of sends each, rejected
    frames, ISNs at both ends of the range and an IP id that wraps."""
    ks, ns = set(), set()
    for name in G.names("send"):
        s = G.script(name)
        b = G.batches(s)
        assert len(b) == 3 and all(kind == G.SEND for _, _, kind in b)
        ks.add(len(s["key"]))
        ns.update(hi - lo for lo, hi, _ in b)
        nread = s["a"]
        assert int(nread.min()) >= 1 and int(nread.max()) == 1470
    assert ks == {1, 7, 64, 2047, 2048, 2049} and ns >= {1, 63, 64, 65, 2047, 2048, 2049, 4097}
    every = np.concatenate([G.script(n)["a"][G.script(n)["kind"] == G.SEND] for n in G.names()])
    assert {1, 1468, 1469, 1470} <= set(every.tolist()) and len(set(every.tolist())) > 1000
    assert {len(G.script(n)["key"]) for n in G.names("recv")} == {3, 5000, 8192, 8193}
    isn = np.concatenate([G.script(n)["info"][:3, 5] for n in G.names("send")])
    assert {0, 0xFFFFFFFF} <= set(isn.tolist()) and any(0xFFFF0000 < v < 0xFFFFFFFF for v in isn.tolist())
    starts = {int(G.script(n)["ip_id0"]) for n in G.names("send")}
    assert {0, 65000} <= starts
    assert any(bool((np.diff(G.script(n)["ip_id_next"].astype(np.int64)) < 0).any()) for n in G.names("send"))
    for name in G.names("mixed"):
        assert [k for _, _, k in G.batches(G.script(name))] == [G.RECV, G.SEND] * 3
    for name in G.names():
        assert int(G.script(name)["head_size"]) == G.HEAD == A.HEAD_SIZE  # the reference's RConn::HEAD_SIZE


@pytest.mark.parametrize("name", G.names())
def test_libnet_calls(name):
    """A framed send is one libnet_build_tcp, one libnet_build_ipv4 and one libnet_write with the constants of
    RawTcp::SendRawTcp; a rejected one (nread 1470) makes no libnet call, returns < 0 and moves neither
    mInfo.seq nor mIpId; a receive makes none."""
    s = G.script(name)
    send = s["kind"] == G.SEND
    sent = send & (s["a"] <= G.MAX_PAYLOAD)
    for k in ("n_tcp", "n_ip", "n_write"):
        assert np.array_equal(s[k], sent.astype(np.uint8)), k
    rej = send & ~sent
    assert bool((s["ret"][rej] < 0).all()) and np.array_equal(s["ret"][sent], G.HEAD + s["a"][sent].astype(np.int32))
    if rej.any():
        at = np.nonzero(rej)[0]
        seq0, _ = G.init_rows(s)
        before_ip = np.where(at > 0, s["ip_id_next"][at - 1], s["ip_id0"])
        assert np.array_equal(s["ip_id_next"][at], before_ip)
        for i in at[:200].tolist():
            assert s["conn_seq"][i] == G.state_after(s, i, "conn_seq", seq0)[s["conn"][i]]
    if sent.any():
        one = lambda k, v: bool((s[k][sent] == v).all())  # noqa: E731
        assert one("t_win", 65535) and one("t_sum", 0) and one("t_urg", 0) and one("t_payload_set", 1)
        assert one("i_tos", 0) and one("i_frag", 0x4000) and one("i_ttl", 64) and one("i_prot", 6) and one("i_sum", 0)
        assert one("i_payload_set", 0) and one("i_payload_s", 0)
        plen = s["t_payload_s"][sent].astype(np.int64)
        assert np.array_equal(plen, G.HEAD + s["a"][sent].astype(np.int64))
        assert np.array_equal(s["t_len"][sent], plen + 20) and np.array_equal(s["i_len"][sent], plen + 40)
        first = np.nonzero(sent)[0][0]  # the ptags: 0 builds, then the tags the recorders returned
        assert s["t_ptag"][first] == 0 and s["i_ptag"][first] == 0
        rest = np.nonzero(sent)[0][1:]
        assert bool((s["t_ptag"][rest] == 1).all()) and bool((s["i_ptag"][rest] == 2).all())
        info = s["info"][s["conn"][sent]]
        for k, col in (("i_src", 0), ("i_dst", 1), ("t_sp", 2), ("t_dp", 3), ("t_control", 6)):
            assert np.array_equal(s[k][sent], info[:, col]), k
    if int(s["frame_cap"]):  # INetConn::Output stamped the conn's key into the head: frame bytes 22..29
        fr = s["frames"][sent]
        key = fr[:, 22:30].astype(np.uint64)
        got = sum(key[:, j] << np.uint64(8 * j) for j in range(8))
        assert np.array_equal(got, s["key"][s["conn"][sent]])
        assert bool((fr[:, 8] == 23).all()) and bool((fr[:, 9] == 0).all())
        assert np.array_equal(fr[:, 10:18], np.broadcast_to(s["id8"], (len(fr), 8)))


@pytest.mark.parametrize("name", G.names())
def test_row_initialisation(name):
    """Rows filled by INTEGRATION.md's rule equal the reference's state after FakeTcp::Init."""
    s = G.script(name)
    seq, ack = G.init_rows(s)
    assert np.array_equal(s["state0"][:, 0], seq) and np.array_equal(s["state0"][:, 1], ack)


@pytest.mark.parametrize("name", G.names())
def test_oracle_and_walk_equal_the_reference(oracle, name):
    """orc_tcp_send_seq_batch / orc_tcp_recv_ack_batch and the Python walk, batch by batch with the state
    carried over, against the recorded libnet_build_tcp seq, libnet_build_ipv4 id, mInfo.seq, mInfo.ack and
    mIpId."""
    s = G.script(name)
    seq, ack = G.init_rows(s)
    ipn = int(s["ip_id0"])
    for lo, hi, kind in G.batches(s):
        conn = s["conn"][lo:hi]
        if kind == G.SEND:
            status = G.status_of(s, lo, hi)
            es, ei, ecs, eipn = py_send(conn.tolist(), status.tolist(), seq.tolist(), ipn)
            got_seq, got_id, seq, ipn = oracle.tcp_send_seq_batch(conn, status, seq, ipn)
            assert got_seq.tolist() == es and got_id.tolist() == ei and seq.tolist() == ecs and ipn == eipn
            sent = status > 0
            assert np.array_equal(got_seq[sent], s["t_seq"][lo:hi][sent])
            assert np.array_equal(got_id[sent], s["i_id"][lo:hi][sent])
            assert bool((got_seq[~sent] == 0).all()) and bool((got_id[~sent] == 0).all())
            # the ack every sent packet carries is the conn's ack after the preceding receive batch
            assert np.array_equal(s["t_ack"][lo:hi][sent], ack[conn[sent]])
        else:
            ack = oracle.tcp_recv_ack_batch(conn, s["ret"][lo:hi] >= 0, s["a"][lo:hi], ack)
        assert np.array_equal(seq, G.state_after(s, hi, "conn_seq", G.init_rows(s)[0]))
        assert np.array_equal(ack, G.state_after(s, hi, "conn_ack", G.init_rows(s)[1]))
        assert ipn == int(s["ip_id_next"][hi - 1])


@pytest.mark.parametrize("name", G.names())
def test_model_equals_the_reference(name):
    s = G.script(name)
    assert G.model_differences(s, G.model(s)) == []


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_fixture_rejects_mutant(mutant):
    """The fixture discriminates: a model with one rule broken differs from it.  Which scripts catch it: the
    send rules every send script; a per-conn IP id every one with more than one conn; the ack rules every
    script with receives; the ISNs every script."""
    caught = {n for n in G.names() if G.model_differences(G.script(n), G.model(G.script(n), mutant))}
    want = {"wire_len": G.names("send") + G.names("mixed"), "reject_seq": G.names("send") + G.names("mixed"),
            "reject_ipid": G.names("send") + G.names("mixed"),
            "ipid_per_conn": [n for n in G.names("send") + G.names("mixed") if len(G.script(n)["key"]) > 1],
            "serial_compare": G.names("recv") + G.names("mixed"), "ack_when_refused": G.names("recv") + G.names("mixed")}
    assert caught == set(want.get(mutant, G.names())), mutant
    if mutant.startswith("isn_ack"):  # the sends alone show it: libnet_build_tcp's ack argument
        s = G.script("send_k7_rr_frames")
        assert "t_ack" in G.model_differences(s, G.model(s, mutant))


@pytest.mark.parametrize("eth", [False, True], ids=["raw4", "eth"])
@pytest.mark.parametrize("name", G.names("frames"))
def test_build_wire_fields_equal_libnet_arguments(oracle, name, eth):
    """orc_build_wire fed with the fixture's TcpInfo rows, the recorded frame and the ORACLE's seq / ip_id / ack:
    every header field equals the recorded libnet argument, the bytes behind the TCP header the recorded frame."""
    s = G.script(name)
    seq, ack = G.init_rows(s)
    ipn = int(s["ip_id0"])
    L = 14 if eth else 0
    n_checked = 0
    for lo, hi, kind in G.batches(s):
        conn = s["conn"][lo:hi]
        if kind == G.RECV:
            ack = oracle.tcp_recv_ack_batch(conn, s["ret"][lo:hi] >= 0, s["a"][lo:hi], ack)
            continue
        status = G.status_of(s, lo, hi)
        pseq, pid, seq, ipn = oracle.tcp_send_seq_batch(conn, status, seq, ipn)
        idx = lo + np.nonzero(status > 0)[0]
        pkts = np.zeros((len(idx), 40 + int(s["frame_cap"])), np.uint8)
        lens = np.zeros(len(idx), np.int64)
        for j, i in enumerate(idx.tolist()):
            c = int(s["conn"][i])
            src, dst, sp, dp, _, _, flag = s["info"][c].tolist()
            frame = s["frames"][i, :int(s["t_payload_s"][i])].tobytes()
            w = oracle.build_wire(frame, src, dst, sp, dp, int(pseq[i - lo]), int(ack[c]), flag, int(pid[i - lo]),
                                  eth=ETH if eth else None)
            assert w[:L] == (ETH if eth else b"")
            pkts[j, :len(w) - L] = np.frombuffer(w[L:], np.uint8)
            lens[j] = len(w) - L
        G.check_packets(s, idx, pkts, lens)
        n_checked += len(idx)
    assert n_checked > 150


def test_packet_checker_rejects_wrong_packets(oracle):
    """The checker the CPU and GPU tests share fails on a packet that differs in any one header byte (but the
    checksums' own, which the fold covers), in one frame byte, or in its length."""
    s = G.script("send_k7_rr_frames")
    seq, ack = G.init_rows(s)
    lo, hi, _ = G.batches(s)[0]
    status = G.status_of(s, lo, hi)
    pseq, pid, _, _ = oracle.tcp_send_seq_batch(s["conn"][lo:hi], status, seq, int(s["ip_id0"]))
    idx = lo + np.nonzero(status > 0)[0][:4]
    pkts, lens = np.zeros((len(idx), 40 + int(s["frame_cap"])), np.uint8), np.zeros(len(idx), np.int64)
    for j, i in enumerate(idx.tolist()):
        c = int(s["conn"][i])
        src, dst, sp, dp, _, _, flag = s["info"][c].tolist()
        w = oracle.build_wire(s["frames"][i, :int(s["t_payload_s"][i])].tobytes(), src, dst, sp, dp, int(pseq[i - lo]),
                              int(ack[c]), flag, int(pid[i - lo]))
        pkts[j, :len(w)], lens[j] = np.frombuffer(w, np.uint8), len(w)
    G.check_packets(s, idx, pkts, lens)
    for at in list(range(40)) + [40, 40 + 8, 40 + 22, int(lens[2]) - 1]:
        bad = pkts.copy()
        bad[2, at] ^= 0x10
        with pytest.raises(AssertionError):
            G.check_packets(s, idx, bad, lens)
    with pytest.raises(AssertionError):
        G.check_packets(s, idx, pkts, lens + np.array([0, 0, 1, 0]))


@pytest.mark.parametrize("name", G.names())
def test_golden_is_the_reference(name):
    """The fixture still equals a fresh run of the reference (where it is present and oracle/_ref built)."""
    if not ref_tcpstate_available():
        pytest.skip("oracle/_ref not built (needs /root/reference)")
    s = G.script(name)
    fresh = G.run_reference(s)
    for k in (*G.RECORDED, "state0", "head_size") + (("frames",) if int(s["frame_cap"]) else ()):
        assert np.array_equal(fresh[k], s[k]), k


def test_empty_payload_data_packet_is_unreachable(oracle):
    """A frame whose head's len byte leaves zero payload bytes never passes RConn::OnRecv: hash_equal refuses
    data_len <= 0 (util/rhash.cpp:71-92), whatever the tag.  So INetGroup::Input's `nread <= 0` return
    (conn/INetGroup.cpp:57-83) cannot be met by a DATA packet from the wire, and rsk_conn_resolve_batch never
    sees a VALID packet with pay_len 0.  The reference's outcomes are recorded; the oracle agrees."""
    z = G._load()
    st = z["empty_status"]
    assert len(st) == 5 * 257 * 2 and bool((st == -1).all()) and bool((z["empty_pay_len"] == -1).all())
    for f, nread, close in zip(z["empty_frames"], z["empty_nread"].tolist(), z["empty_close"].tolist()):
        d = oracle.rconn_onrecv(G.KEY, f.tobytes(), nread=nread, close=bool(close))
        assert d.status == A.RECV_DROP and d.pay_len == 0
    if ref_available():
        from tests.oracle_lib import RefOracle

        ref = RefOracle()
        for f, nread, close in list(zip(z["empty_frames"], z["empty_nread"].tolist(), z["empty_close"].tolist()))[::7]:
            assert ref.rconn_onrecv(G.KEY, f.tobytes(), nread=nread, close=bool(close))[0] == -1
