#!/usr/bin/env python3
"""Generates tests/golden/conncreate.npz from the REFERENCE's own way from a handshake to a fake-TCP conn
(RawTcp::RawInput, TcpAckPool, ServerNetManager::GetTcp / OnFlush, SNetGroup::CreateNetConn, INetGroup::Input /
AddNetConn / doSend, FakeTcp::Init / OnRecv, compiled by `make -C oracle ref` into
oracle/_ref/librsk_ref_conncreate.so; oracle/ref_conncreate_harness.cpp names its stand-ins).  Run in the build
container:

    make -C oracle ref && python tests/golden/make_conncreate_golden.py

The scripts (tests/conncreate_golden.py describes events and records):
  size_*        batches of 1, 63, 64, 65, 2047, 2048, 2049 and 4097 packets over 1, 3 and 65 groups: all conns born in
                one batch, born conns interleaved with known ones, bursts of 1-200 packets per key, one key on every
                packet, every packet a different key; a twentieth of the keys without an accepted socket
  two_keys      one tuple named by two keys, and by one connKey under two IdBufs: the first takes it
  half_offers   handshakes without a socket, sockets without a handshake (each blocks the reference for its 500 ms
                BLOCK_WAIT_MS: 6 in the whole fixture), the missing half arriving later
  repeated_syn  two handshakes of a tuple with different numbers, before and after the accept, and an expiry that
                only the second one's stamp survives
  refused_syn   a handshake with port 0: the pool refuses it, the parse reports it
  edges         record acks 0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF; DATA flags other than ACK; packet seqs
                one below, at and one above the new conn's ack
  expiry        both pools flushed between batches, at and around the stamps
  sends         scripted draws after a create and after a second create into the same groups
  orientation   an incoming plain SYN: its reversed record is not the DATA packets' tuple
  client_*      (stored apart) the dial sequence of ClientNetManager::createINetConn for 1, 64 and 2049 dials
  deviation_*   a refused key whose later packet carries another tuple that has an offer: the reference creates there,
                the batch rule at the next call (include/rsk_codec.h).  Kept apart: `deviation` is set.
Every script's conns stay below the capacity the device tests give it (257 or 4097): the reference has no full
table.  Fixtures are data only (inputs and the reference's outputs); no reference source is stored.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import conncreate_golden as G  # noqa: E402

SYN, ACCEPT, DATA, FLUSH_ACK, FLUSH_NET, SEND = range(6)
SERVER, SPORT = 0x0100000A, 10001  # 10.0.0.1 as s_addr holds it


def client(f):
    """Flow f's client end: (address, port)."""
    f = np.asarray(f, np.int64)
    return (0x0A | ((1 + (f >> 16)) << 8) | (((f >> 8) & 255) << 16) | ((f & 255) << 24)).astype(np.uint32), \
        (1024 + f * 7 % 60000).astype(np.uint16)


class Script:
    def __init__(self, n_groups, seed, deviation=False):
        self.rng = np.random.default_rng(seed)
        self.n_groups, self.deviation = n_groups, deviation
        self.ids = self.rng.permutation(1 << 20)[:n_groups].astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1)
        self.ev = []
        self.syn_c = {k: [] for k in ("src", "dst", "sport", "dport", "seq", "ack", "flags")}
        self.acc, self.d, self.draws = [], {k: [] for k in ("flow", "seq", "flags", "group", "key")}, []
        self.sent = {}  # flow -> DATA packets so far

    # a flow's handshake numbers: the server's ISN (the record's ack) and the client's ISN + 1
    def isn(self, f):
        f = np.asarray(f, np.int64)
        r = (f * 2654435761 + 12345) % (1 << 32)
        return np.where(f < 32, r, 0x7FFFF000 + 5 * f).astype(np.uint32), (0x1000 + 3 * f).astype(np.uint32)

    def syn(self, flows, ts, seq=None, ack=None, flags=0x12, plain=False, port0=False):
        """The server's SYN|ACK of each flow as its own capture card sees it (plain: the client's SYN coming in)."""
        flows = np.atleast_1d(np.asarray(flows, np.int64))
        ca, cp = client(flows)
        s0, a0 = self.isn(flows)
        k = len(flows)
        srv_a, srv_p = np.full(k, SERVER, np.uint32), np.full(k, SPORT, np.uint16)
        if port0:
            cp = np.zeros(k, np.uint16)
        src, dst, sp, dp = (ca, srv_a, cp, srv_p) if plain else (srv_a, ca, srv_p, cp)
        lo = len(self.syn_c["src"])
        for name, v in (("src", src), ("dst", dst), ("sport", sp), ("dport", dp),
                        ("seq", s0 if seq is None else np.full(k, seq, np.uint32)),
                        ("ack", a0 if ack is None else np.full(k, ack, np.uint32)), ("flags", np.full(k, flags, np.uint8))):
            self.syn_c[name].extend(v.tolist())
        self.ev.append((SYN, ts, lo, lo + k, 0))

    def accept(self, flows, ts):
        flows = np.atleast_1d(np.asarray(flows, np.int64))
        ca, cp = client(flows)
        lo = len(self.acc)
        self.acc.extend([[SERVER, int(a), SPORT, int(p)] for a, p in zip(ca, cp)])
        self.ev.append((ACCEPT, ts, lo, lo + len(flows), 0))

    def data(self, group, key, flow, seq=None, flags=None):
        """One batch.  Without seq a flow's packets count up from above its conn's first ack, one in ten arriving
        late (a lower seq than the one before)."""
        group, key, flow = np.asarray(group, np.int64), np.asarray(key, np.uint64), np.asarray(flow, np.int64)
        n = len(key)
        if seq is None:
            seq = np.zeros(n, np.uint32)
            base = self.isn(flow)[0].astype(np.int64) + 100
            late = self.rng.random(n) < 0.1
            for i in range(n):
                j = self.sent.get(int(flow[i]), 0)
                self.sent[int(flow[i])] = j + 1
                seq[i] = (base[i] + 16 * j - (64 if late[i] else 0)) & 0xFFFFFFFF
        lo = len(self.d["key"])
        for name, v in (("flow", flow), ("seq", np.asarray(seq, np.uint32)), ("group", group), ("key", key),
                        ("flags", np.full(n, 0x18, np.uint8) if flags is None else np.asarray(flags, np.uint8))):
            self.d[name].extend(v.tolist())
        self.ev.append((DATA, 0, lo, lo + n, 0))

    def flush(self, kind, ts):
        self.ev.append((kind, ts, 0, 0, 0))

    def send(self, group, n):
        lo = len(self.draws)
        self.draws.extend(self.rng.integers(0, 2**31, n).tolist())
        self.ev.append((SEND, 0, lo, lo + n, group))

    def inputs(self):
        ev = np.array(self.ev, np.int64).reshape(-1, 5)
        flow = np.array(self.d["flow"], np.int64)
        ca, cp = client(flow)
        n = len(flow)
        return {"n_groups": np.uint32(self.n_groups), "ids": self.ids.view(np.uint8).reshape(-1, 8).copy(),
                "deviation": np.uint8(self.deviation), "ev_kind": ev[:, 0].astype(np.uint8), "ev_ts": ev[:, 1].astype(np.uint64),
                "ev_lo": ev[:, 2].astype(np.uint32), "ev_hi": ev[:, 3].astype(np.uint32), "ev_arg": ev[:, 4].astype(np.uint32),
                "syn_src": np.array(self.syn_c["src"], np.uint32), "syn_dst": np.array(self.syn_c["dst"], np.uint32),
                "syn_sport": np.array(self.syn_c["sport"], np.uint16), "syn_dport": np.array(self.syn_c["dport"], np.uint16),
                "syn_seq": np.array(self.syn_c["seq"], np.uint32), "syn_ack": np.array(self.syn_c["ack"], np.uint32),
                "syn_flags": np.array(self.syn_c["flags"], np.uint8), "acc_tuple": np.array(self.acc, np.uint32).reshape(-1, 4),
                "d_src": ca, "d_dst": np.full(n, SERVER, np.uint32), "d_sport": cp, "d_dport": np.full(n, SPORT, np.uint16),
                "d_seq": np.array(self.d["seq"], np.uint32), "d_flags": np.array(self.d["flags"], np.uint8),
                "d_group": np.array(self.d["group"], np.uint8), "d_key": np.array(self.d["key"], np.uint64),
                "s_draws": np.array(self.draws, np.uint32)}


def keys_of(rng, k):
    return (rng.permutation(1 << 22)[:k].astype(np.uint64) + np.uint64(1)) * np.uint64(0x100000001B3) + np.uint64(1 << 40)


def size_script(n, n_groups, comp, seed):
    """One measured batch of n packets; conn c is (group c % G, keys[c], flow c)."""
    s = Script(n_groups, seed)
    rng = s.rng
    if comp == "one_key":
        which = np.zeros(n, np.int64)
    elif comp == "all_different":
        k = min(n, 4000)
        which = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])
    elif comp == "bursts":
        parts, c = [], 0
        while sum(map(len, parts)) < n:
            parts.append(np.full(int(rng.integers(1, 201)), c))
            c += 1
        which = np.concatenate(parts)[:n]
    else:  # all_born / interleaved: every conn at least once, in random arrival order
        k = max(1, n // 3)
        which = np.concatenate([np.arange(k), rng.integers(0, k, n - k)])[rng.permutation(n)]
    k = int(which.max()) + 1
    keys, group = keys_of(rng, k), np.arange(k) % n_groups
    flows = np.arange(k)
    no_socket = (flows % 20 == 7) & (k > 1)
    s.syn(flows, 0)
    s.accept(flows[~no_socket], 0)
    if comp == "interleaved":  # a first batch makes every other conn known
        known = flows[::2]
        s.data(group[known], keys[known], known)
    s.data(group[which], keys[which], which)
    return s


def two_keys():
    s = Script(3, 101)
    s.syn([0, 1, 2, 3], 0)
    s.accept([0, 1, 2, 3], 0)
    A_, B_, C_, D_ = (np.uint64(x) for x in (0x1111, 0x2222, 0x3333, 0x4444))
    #         the first takes flow 0 | one connKey, two IdBufs, one tuple | one connKey, two IdBufs, two tuples
    s.data([0, 0, 0, 0, 1, 0, 1, 1, 2, 1, 2], [A_, B_, A_, C_, C_, B_, C_, D_, D_, D_, D_], [0, 0, 0, 1, 1, 0, 1, 2, 3, 2, 3])
    s.data([0, 0, 1, 0], [B_, A_, C_, C_], [0, 0, 1, 1])  # the refused ones again: nothing is left for them
    return s


def half_offers():
    s = Script(1, 102)
    k = keys_of(s.rng, 12)
    s.syn([0, 1, 2, 3, 7, 8, 9, 10], 0)      # 0-3, 9, 10: a handshake and no socket
    s.accept([4, 5, 6, 7, 8], 0)             # 4-6: a socket and no handshake
    f = np.array([0, 4, 7, 1, 5, 8, 2, 6, 3, 7, 0, 4])
    s.data(np.zeros(len(f)), k[f], f)        # 7, 8 born; the others refused, and what they had is gone
    s.accept([3, 9, 10], 10)                 # the missing halves arrive
    s.syn([4], 10)
    f = np.array([3, 9, 4, 10, 9, 0])
    s.data(np.zeros(len(f)), k[f], f)        # 9, 10 born; 3 has a socket only now, 4 a handshake only
    s.syn([3, 4], 20)
    s.accept([4], 20)
    f = np.array([3, 4, 4])
    s.data(np.zeros(len(f)), k[f], f)        # 4 born at last; 3 a handshake only
    return s


def repeated_syn():
    s = Script(1, 103)
    k = keys_of(s.rng, 3)
    s.syn([0], 100, seq=0x11110000, ack=0x22220000)
    s.syn([1], 100, seq=0x55550000, ack=0x66660000)
    s.syn([2], 100, seq=0x99990000, ack=0xAAAA0000)
    s.syn([0], 600, seq=0x33330000, ack=0x44440000)   # before the accept: the first one's numbers stay
    s.accept([0, 1, 2], 600)
    s.syn([1], 650, seq=0x77770000, ack=0x88880000)   # after the accept
    s.flush(FLUSH_ACK, 1100)                          # flow 2's stamp (1100) is due, the moved ones (1600, 1650) are not
    s.data([0, 0, 0, 0], k[[0, 1, 2, 0]], [0, 1, 2, 0])
    return s


def refused_syn():
    s = Script(1, 104)
    k = keys_of(s.rng, 2)
    s.syn([0], 0, port0=True)
    s.syn([0], 0, port0=True, flags=0x02)
    s.syn([1], 0)
    s.accept([1], 0)
    s.data([0, 0], k[[1, 1]], [1, 1])
    return s


def edges():
    s = Script(3, 105)
    acks = [0, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF, 0x7FFFFFFE, 1, 0xFFFFFFFD]
    flags = [0x10, 0x18, 0x11, 0x04, 0x14, 0x38, 0x00, 0x19]
    k = keys_of(s.rng, len(acks))
    for f, a in enumerate(acks):
        s.syn([f], 0, seq=a, ack=0xC0000000 + f)
    s.accept(np.arange(len(acks)), 0)
    g, key, flow, seq, fl = [], [], [], [], []
    for rnd, order in enumerate(((0, 1, -1), (-1, 1, 0), (1, 0, -1))):
        for f, a in enumerate(acks):
            for d in order:  # TcpInfo.seq = the conn's ack after Init (a + 2), one more per round, + d
                g.append(f % 3); key.append(k[f]); flow.append(f)
                seq.append((a + 2 + rnd + d - G.PAYLOAD) & 0xFFFFFFFF)
                fl.append(flags[(f + rnd + d) % len(flags)])
        if rnd == 0:
            s.data(g, key, flow, seq, fl)
            g, key, flow, seq, fl = [], [], [], [], []
    s.data(g, key, flow, seq, fl)
    return s


def expiry():
    s = Script(1, 106)
    k = keys_of(s.rng, 6)
    s.syn([0, 1, 2], 0)        # due at 1000
    s.syn([3, 4, 5], 500)      # due at 1500
    s.accept([0, 1, 3], 0)     # due at 1000
    s.accept([2, 4, 5], 600)   # due at 1600
    s.flush(FLUSH_ACK, 999)
    s.flush(FLUSH_NET, 999)
    s.flush(FLUSH_ACK, 1000)   # 0, 1, 2 go: expiry <= ts
    s.flush(FLUSH_NET, 1000)   # the sockets of 0, 1, 3 are closed: ts >= expiry
    f = np.array([0, 4, 1, 3, 5, 4])
    s.data(np.zeros(len(f)), k[f], f)  # 4, 5 born; 3 had a handshake only; 2's socket is not asked for
    s.flush(FLUSH_NET, 1599)
    s.flush(FLUSH_NET, 1600)   # 2's socket
    s.flush(FLUSH_ACK, 5000)
    return s


def sends():
    s = Script(3, 107)
    key = lambda c: np.uint64(10_000_000 + 37 * c)  # noqa: E731  -- creation order is the string order of the keys
    s.syn(np.arange(14), 0)
    s.accept(np.arange(14), 0)
    c = np.array([0, 1, 2, 0, 3, 4, 5, 6, 7, 1])
    s.data(np.where(c < 5, 0, 1), [key(x) for x in c], c)     # group 0: conns 0-4, group 1: 5-7
    s.send(0, 64)
    s.send(1, 64)
    c = np.array([8, 9, 10, 11, 8, 12, 13, 0])
    s.data(np.where(c < 12, 0, 2), [key(x) for x in c], c)    # group 0 grows by 8-11, group 2 is new
    s.send(0, 64)
    s.send(2, 32)
    s.send(1, 16)
    return s


def orientation():
    s = Script(1, 108)
    k = keys_of(s.rng, 2)
    s.syn([0], 0, plain=True, flags=0x02)  # the client's SYN coming in: reversed, it is not the DATA packets' tuple
    s.syn([1], 0)
    s.accept([0, 1], 0)
    s.data([0, 0, 0], k[[0, 1, 0]], [0, 1, 0])
    return s


def deviation():
    s = Script(1, 109, deviation=True)
    k = keys_of(s.rng, 3)
    s.syn([1, 2], 0)
    s.accept([1, 2], 0)
    #            D on flow 0 (nothing there), E born, D on flow 1 (an offer): the reference creates D there
    s.data([0, 0, 0, 0, 0], k[[0, 1, 0, 0, 1]], [0, 2, 1, 1, 2])
    s.data([0, 0, 0], k[[0, 1, 0]], [1, 2, 1])
    return s


def client_case(ref_cls, k, seed):
    """k dials (stored apart: c<k>_*): the handshakes as the client's card sees them (the server's SYN|ACK coming
    in, no server flag), then the createINetConn sequence per dialled socket."""
    rng = np.random.default_rng(seed)
    flows = rng.permutation(60000)[:k]
    ca, cp = client(flows)
    cp = (1024 + np.arange(k) * 3 % 60000).astype(np.uint16)  # KeyForTcp is made of the ports: distinct ones
    seq = np.where(np.arange(k) < 8, np.array([0, 0xFFFFFFFE, 0xFFFFFFFF, 0x7FFFFFFF, 5, 6, 7, 8], np.uint32)[np.arange(k) % 8],
                   0x7FFFF000 + 5 * np.arange(k)).astype(np.uint32)
    ack = (0x2000 + 7 * np.arange(k)).astype(np.uint32)
    f = G.frames(np.full(k, SERVER, np.uint32), ca, np.full(k, SPORT, np.uint16), cp, seq, ack, np.full(k, 0x12, np.uint8), 0)
    ref = ref_cls(1, G.PERSIST_MS)
    try:
        took = ref.syn([bytes(x) for x in f], 0, server=False)
        tuples = np.stack([ca, np.full(k, SERVER, np.uint32), cp.astype(np.uint32), np.full(k, SPORT, np.uint32)], axis=1)
        d = ref.dial(tuples)
        left = ref.pools()
    finally:
        ref.close()
    assert took.all() and d["ok"].all() and d["found"].all() and len(left["ack"]) == 0
    return {"syn_src": np.full(k, SERVER, np.uint32), "syn_dst": ca, "syn_sport": np.full(k, SPORT, np.uint16), "syn_dport": cp,
            "syn_seq": seq, "syn_ack": ack, "tuple": tuples.astype(np.uint32), "key": d["key"], "info": d["info"]}


SIZES = ((1, 1, "all_born"), (63, 3, "interleaved"), (64, 65, "bursts"), (65, 1, "all_different"), (2047, 3, "bursts"),
         (2048, 65, "interleaved"), (2049, 1, "all_different"), (4097, 3, "one_key"), (4097, 65, "all_different"),
         (2049, 65, "all_born"), (65, 3, "one_key"))


def scripts():
    out = [(f"size_{n}_g{g}_{comp}", size_script(n, g, comp, 1000 + i)) for i, (n, g, comp) in enumerate(SIZES)]
    out += [("two_keys", two_keys()), ("half_offers", half_offers()), ("repeated_syn", repeated_syn()),
            ("refused_syn", refused_syn()), ("edges", edges()), ("expiry", expiry()), ("sends", sends()),
            ("orientation", orientation()), ("deviation_other_tuple", deviation())]
    return out


def main():
    from tests.oracle_lib import RefConnCreate

    out, names = {}, []
    for i, (name, sc) in enumerate(scripts()):
        s = sc.inputs()
        s["capacity"] = np.uint32(0)
        rec = G.run_reference(s)
        s.update(rec)
        conns = len(s["c_key"])
        s["capacity"] = np.uint32(257 if conns < 257 else 4097)
        assert conns < 4097, (name, conns)
        z = G.pack(s)
        back = G.unpack(z)
        assert all(np.array_equal(back[k], s[k]) for k in s), name
        for k, v in z.items():
            out[f"s{i}_{k}"] = np.asarray(v)
        names.append(name)
        ex = G.expected(s)
        print(f"{name}: {len(s['d_key'])} packets, {conns} conns, {int((s['r_ret'] == G.ERR_NO_CONN).sum())} without a conn, "
              f"{int(s['closed'][-1]) if len(s['closed']) else 0} sockets closed, moved {ex['moved']}")
    out["names"] = np.array(names)
    for k in (1, 64, 2049):
        for f, v in client_case(RefConnCreate, k, 7000 + k).items():
            out[f"c{k}_{f}"] = v
    path = os.path.join(HERE, "conncreate.npz")
    np.savez_compressed(path, **out)
    print(f"conncreate.npz: {len(names)} scripts, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
