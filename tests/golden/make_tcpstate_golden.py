"""Writes tests/golden/tcpstate.npz: scripts of sends and receives run through the REFERENCE's own FakeTcp /
INetConn / RConn / RawTcp (oracle/_ref/librsk_ref_tcpstate.so, oracle/ref_tcpstate_harness.cpp), with what it
did recorded per event, and the empty-payload OnRecv cases run through the reference's DecodeBuf / hash_equal
(oracle/_ref/librsk_ref.so).  Only inputs and recorded columns are stored; tests/tcpstate_golden.py reads them.

    make -C oracle ref && python tests/golden/make_tcpstate_golden.py

Deterministic: a second run writes the same bytes."""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import tcpstate_golden as G  # noqa: E402
from tests.oracle_lib import RefOracle  # noqa: E402

ID8 = b"\x11\x22\x33\x44\x55\x66\x77\x88"
FRAME_CAP = 96  # 31 + 64 and one to spare


def conns(rng, k, isn_ack, isn_seq, low_entropy=False):
    """K TcpInfo rows (src, dst, sp, dp, seq, ack, flag) and keys.  isn_ack / isn_seq: the values the first
    conns take for info.ack / info.seq; the others are random.  Both ISNs come from info.ack: seq = ack + 1,
    ack = ack + 2."""
    info = np.zeros((k, 7), np.uint32)
    info[:, 0] = 0x0100000A + (np.arange(k, dtype=np.uint32) % 3 << 24)   # 10.0.0.1 .. .3, as stored
    info[:, 1] = 0x6400A8C0                                                # 192.168.0.100
    info[:, 2] = 40000 + np.arange(k) % 256
    info[:, 3] = 10001 + np.arange(k) // 256
    r = lambda: rng.integers(0, 2**32, k, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    if low_entropy:  # the big scripts: values that spread over the whole range, two random bytes each
        r = lambda: (rng.integers(0, 2**16, k, dtype=np.uint64).astype(np.uint32) << 16) | np.uint32(0x8000)  # noqa: E731
    info[:, 4], info[:, 5] = r(), r()
    if low_entropy:  # FakeTcp::Init never reads info.seq (see tests/tcpstate_golden.init_rows): the small scripts vary it
        info[:, 4] = 0x2000
    info[:min(k, len(isn_seq)), 4] = isn_seq[:k]
    info[:min(k, len(isn_ack)), 5] = isn_ack[:k]
    info[:, 6] = np.where(np.arange(k) % 5 == 0, 0x18, 0x10)               # ACK, some PSH | ACK
    key = (np.uint64(0x10000000) | (info[:, 3].astype(np.uint64) << 16) | info[:, 2].astype(np.uint64))
    return info, key


def order(rng, how, k, n):
    if how == "rr":
        return (np.arange(n) + int(rng.integers(0, k))) % k
    if how == "random":
        return rng.integers(0, k, n)
    if how == "one":
        return np.full(n, k - 1)
    runs = rng.integers(1, 201, n // 50 + 2)  # bursts of 1-200 packets of one conn
    return np.repeat(rng.integers(0, k, runs.size), runs)[:n]


LENS = np.array([1, 2, 8, 9, 33, 64, 100, 512, 1000, 1399, 1400, 1460, 1467, 1468, 1469])


def send_batch(rng, how, k, n, small, reject_every, low_entropy):
    conn = order(rng, how, k, n)
    nread = rng.integers(1, 65, n) if small else rng.integers(1, 1470, n)
    if low_entropy:  # the big scripts draw from a few lengths over the same range: the fixture stays small
        nread = rng.choice(LENS, n)
    if not small and n >= 8:
        nread[rng.integers(0, n, 3)] = [1, 1469, 1468]
    nread[(np.arange(n) + 1) % reject_every == 0] = 1470  # RConn::Output rejects 8 + 23 + 1470 > 1500
    return conn, nread


def recv_batch(rng, k, n, ack_now, low_entropy=False):
    conn = rng.integers(0, k, n)
    seq = rng.integers(0, 2**32, n, dtype=np.uint64)
    if low_entropy:
        seq = (rng.integers(0, 2**16, n, dtype=np.uint64) << 16) | 0x8000
    # a third of the packets lie just either side of their conn's ack ISN, and just either side of 2^32
    near = rng.random(n) < 0.33
    seq[near] = (ack_now[conn[near]].astype(np.int64) + rng.integers(-3, 4, int(near.sum()))) % 2**32
    edge = rng.random(n) < 0.1
    seq[edge] = rng.choice([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0x80000001, 0xFFFFFFFE, 0xFFFFFFFF], int(edge.sum()))
    up = rng.choice([0, 1, 1400, 0, 1, 1400, -1, -20], n)  # what the upstream callback returns
    return conn, seq.astype(np.uint32), up.astype(np.int32)


def build(name, rng, k, plan, isn_ack=(), isn_seq=(), ip_id0=0, frames=False, low_entropy=False):
    """plan: [("send", how, n) | ("recv", n)].  Frame scripts keep payloads at 64 B or below (and the
    rejected 1470), each its own random bytes; the others share one 1470-B arena and record lengths only."""
    info, key = conns(rng, k, np.array(isn_ack, np.uint32), np.array(isn_seq, np.uint32), low_entropy)
    arena = [rng.integers(0, 256, 1470, dtype=np.uint64).astype(np.uint8)]
    at = 1470
    cols = {c: [] for c in ("kind", "conn", "a", "b", "conv", "pay_off")}
    batch_off = [0]
    ack_now = info[:, 5] + np.uint32(2)
    for step in plan:
        if step[0] == "send":
            _, how, n = step
            conn, nread = send_batch(rng, how, k, n, small=frames, reject_every=7 if n >= 7 else 1000,
                                     low_entropy=low_entropy)
            off = np.zeros(n, np.int64)
            if frames:
                for i in np.nonzero(nread <= 64)[0]:
                    arena.append(rng.integers(0, 256, int(nread[i]), dtype=np.uint64).astype(np.uint8))
                    off[i] = at
                    at += int(nread[i])
            new = {"kind": np.full(n, G.SEND), "conn": conn, "a": nread, "b": np.zeros(n), "pay_off": off,
                   "conv": rng.integers(0, 2**32, n, dtype=np.uint64) if frames else 7 + conn % 5}
        else:
            _, n = step
            conn, seq, up = recv_batch(rng, k, n, ack_now, low_entropy)
            new = {"kind": np.full(n, G.RECV), "conn": conn, "a": seq, "b": up, "pay_off": np.zeros(n),
                   "conv": np.zeros(n)}
        for c, v in new.items():
            cols[c].append(np.asarray(v))
        batch_off.append(batch_off[-1] + n)
    dt = {"kind": np.uint8, "conn": np.uint32, "a": np.uint32, "b": np.int32, "conv": np.uint32, "pay_off": np.uint64}
    s = {c: np.concatenate(v).astype(dt[c]) for c, v in cols.items()}
    s.update(info=np.asfortranarray(info), key=key, ip_id0=np.uint16(ip_id0), id8=np.frombuffer(ID8, np.uint8).copy(),
             arena=np.concatenate(arena), batch_off=np.array(batch_off, np.int64),
             frame_cap=np.int32(FRAME_CAP if frames else 0))
    s.update(G.run_reference(s))
    return name, s


def scripts():
    rng = np.random.default_rng(20261021)
    S = lambda how, n: ("send", how, n)  # noqa: E731
    R = lambda n: ("recv", n)  # noqa: E731
    near = 0xFFFFFFFF - 40000  # within one batch's bytes of 2^32
    # info.ack 0xFFFFFFFE / 0xFFFFFFFD / 0xFFFFFFFF: ack ISNs 0, 0xFFFFFFFF and 1
    out = [
        # sends: K around the per-tile table's 2048 rows (n_conn + 1 <= 2048), N around the tile sizes
        build("send_k1_one_a", rng, 1, [S("one", 1), S("one", 64), S("one", 65)], isn_ack=[0], ip_id0=0),
        build("send_k1_one_b", rng, 1, [S("one", 2049), S("one", 63), S("one", 1)], isn_ack=[0xFFFFFFFF], ip_id0=65000),
        build("send_k7_rr_frames", rng, 7, [S("rr", 63), S("rr", 64), S("rr", 65)], isn_ack=[0, 0xFFFFFFFF, near],
              ip_id0=65500, frames=True),
        build("send_k7_random", rng, 7, [S("random", 2047), S("random", 1), S("random", 65)],
              isn_ack=[near, 0, 0xFFFFFFFF], ip_id0=65000),
        build("send_k64_bursts", rng, 64, [S("bursts", 2048), S("bursts", 65), S("bursts", 63)],
              isn_ack=[0xFFFFFFFF, near, 0], ip_id0=0),
        build("send_k64_random_frames", rng, 64, [S("random", 64), S("bursts", 63), S("random", 65)],
              isn_ack=[0, 0xFFFFFFFF, near], ip_id0=65400, frames=True),
        build("send_k2047_rr", rng, 2047, [S("rr", 2048), S("rr", 63), S("rr", 1)], isn_ack=[0, 0xFFFFFFFF, near],
              ip_id0=65000, low_entropy=True),
        build("send_k2047_bursts", rng, 2047, [S("bursts", 4097), S("bursts", 1), S("bursts", 64)],
              isn_ack=[near, 0xFFFFFFFF, 0], ip_id0=0, low_entropy=True),
        build("send_k2048_random", rng, 2048, [S("random", 2049), S("random", 65), S("random", 64)],
              isn_ack=[0, near, 0xFFFFFFFF], ip_id0=65000, low_entropy=True),
        build("send_k2048_bursts", rng, 2048, [S("bursts", 2047), S("bursts", 64), S("one", 1)],
              isn_ack=[0xFFFFFFFF, 0, near], ip_id0=0, low_entropy=True),
        build("send_k2049_random", rng, 2049, [S("random", 4097), S("random", 64), S("random", 63)],
              isn_ack=[0, 0xFFFFFFFF, near], ip_id0=65000, low_entropy=True),
        build("send_k2049_rr", rng, 2049, [S("rr", 2048), S("bursts", 65), S("rr", 1)], isn_ack=[near, 0, 0xFFFFFFFF],
              ip_id0=0, low_entropy=True),
        # receives: K around the ack kernel's 8192-row table
        build("recv_k3", rng, 3, [R(400), R(300), R(300)], isn_ack=[0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF], isn_seq=[0, 0xFFFFFFFF]),
        build("recv_k5000", rng, 5000, [R(1500), R(1500)], isn_ack=[0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF], isn_seq=[0, 0xFFFFFFFF], low_entropy=True),
        build("recv_k8192", rng, 8192, [R(10000), R(10000)], isn_ack=[0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF], isn_seq=[0xFFFFFFFF, 0], low_entropy=True),
        build("recv_k8193", rng, 8193, [R(10000), R(10000)], isn_ack=[0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFF], isn_seq=[0, 0xFFFFFFFF], low_entropy=True),
        # a receive batch, then a send batch on the same conns, three times over
        build("mixed_k7_frames", rng, 7, [R(65), S("random", 64), R(64), S("bursts", 65), R(63), S("rr", 63)],
              isn_ack=[0xFFFFFFFF, 0, near], isn_seq=[0, 0xFFFFFFFF], ip_id0=65450, frames=True),
        build("mixed_k64_frames", rng, 64, [R(200), S("bursts", 65), R(200), S("random", 64), R(200), S("random", 63)],
              isn_ack=[near, 0xFFFFFFFF, 0], isn_seq=[0xFFFFFFFF, 0], ip_id0=0, frames=True),
    ]
    return out


def onrecv_empty(ref: RefOracle):
    """Frames whose head's len byte is longer than the minimum 23, so that nread leaves zero payload bytes
    behind the head: tag [8] | len | cmd | id [8] | conv | connKey [8] | reserved | (len - 23 filler bytes).
    The tag covers MD5(key || first payload byte) and there is no such byte; every tag a sender could have
    computed is tried: each of the 256 possible first bytes (compute_hash asserts data_len > 0, so no tag over
    no data exists), and a zero tag.  Recorded: the reference's
    OnRecv outcome (1 valid, 0 close-notify, -1 drop) and, when valid, its payload length."""
    frames, lens, close, st, plen = [], [], [], [], []
    for hlen in (24, 25, 31, 64, 255):
        head = bytes([hlen, 0]) + ID8 + (77).to_bytes(4, "little") + (0x1000271140001).to_bytes(8, "big") + b"\0"
        head += bytes(range(1, hlen - 23 + 1))
        assert len(head) == hlen
        tags = [bytes(8)] + [ref.tag(G.KEY, bytes([b])) for b in range(256)]
        for t in tags:
            for fin in (0, 1):
                f = t + head
                r, dec = ref.rconn_onrecv(G.KEY, f + b"\0" * 8, nread=len(f), close=bool(fin))
                frames.append(np.frombuffer(f.ljust(8 + 255, b"\0"), np.uint8))
                lens.append(len(f))
                close.append(fin)
                st.append(r)
                plen.append(dec[6] if dec else -1)
    return {"empty_frames": np.stack(frames), "empty_nread": np.array(lens, np.int32),
            "empty_close": np.array(close, np.uint8), "empty_status": np.array(st, np.int8),
            "empty_pay_len": np.array(plen, np.int32)}


def main():
    out = {}
    names = []
    for i, (name, s) in enumerate(scripts()):
        names.append(name)
        stored = G.pack(s)
        back = G.unpack(stored)
        assert all(np.array_equal(back[k], s[k]) and back[k].dtype == s[k].dtype for k in (*G.RECORDED, "state0")), name
        for k, v in stored.items():
            out[f"s{i}_{k}"] = v
    out["names"] = np.array(names)
    out.update(onrecv_empty(RefOracle()))
    path = os.path.join(HERE, "tcpstate.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes", len(names), "scripts")


if __name__ == "__main__":
    main()
