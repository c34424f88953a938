"""TEST INFRASTRUCTURE: tests/golden/conncreate.npz -- scripts of handshakes, accepts, DATA batches, pool flushes and
sends as the REFERENCE's own RawTcp / TcpAckPool / ServerNetManager / SNetGroup / INetGroup / FakeTcp ran them
(oracle/ref_conncreate_harness.cpp through tests/oracle_lib.RefConnCreate; written by
tests/golden/make_conncreate_golden.py) -- and the checker that holds rsk_conn_create_batch TOGETHER WITH the host
procedure INTEGRATION.md documents around it against that record.  Every comparison is integer-exact.

A script is a list of events over G groups (one SNetGroup / IdBuf each):
  SYN        captures through RawInput with the server flag (the socket pool untouched), stamped ts
  ACCEPT     tuples into ServerNetManager::mPool, stamped ts
  DATA       a batch of captures, each with its group and connKey
  FLUSH_ACK  TcpAckPool::OnFlush(ts)          FLUSH_NET  ServerNetManager::OnFlush(ts)
  SEND       sends through one group's INetGroup::Send with scripted draws
Recorded: per DATA packet Input's return, whether CreateNetConn ran and what it returned, the conn (creation ordinal)
the key names afterwards and that conn's mInfo.ack; per created conn its group, IntKey, creating packet and mInfo
after Init; after every event both pools (the ack pool with its stored seq / ack, both with their expiry) and the
sockets closed so far; per send the sending conn's IntKey and the draws consumed.

check(script, backend) replays a script on a device under test using ONLY the documented procedure (HostModel):
offers are harvested from the parse's RSK_PARSE_SYN rows and joined with the accepted tuples, the batch runs
resolve -> conn_create -> recv_ack, the pools are kept by the after-batch rules, the pick runs the scripted draws.
Backends: Twin ("cpu": the host twins), Twin(gpu, codec) (the batch calls), Model (conn_create_ref.create_ref, or the
packet walk below with one rule bent: the mutants that show the fixture sees each rule).

THE DEVIATION the header documents (a refused key is not asked again at its later packets) is the one place the
expected outcome is not the recorded one: expected() moves a conn the reference made at a later packet of a refused
key to the next batch that carries the key, and check() asserts that nothing else differs."""
from __future__ import annotations

import functools
import os

import numpy as np

from rsock_amd import _abi as A
from tests import conn_close_ref as K
from tests import conn_create_ref as R
from tests import conn_ref as CR
from tests import pick_ref as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conncreate.npz")
EV_SYN, EV_ACCEPT, EV_DATA, EV_FLUSH_ACK, EV_FLUSH_NET, EV_SEND = range(6)
TH_SYN, TH_ACK = 0x02, 0x10
PARSE_DELIVER, PARSE_SYN = 1, 2
PARSE_FLAGS = 3  # RSK_PARSE_HAS_ACK_POOL | RSK_PARSE_IS_SERVER
PAYLOAD = 16     # bytes behind every DATA packet's TCP header (RawInput drops fewer than 9)
PERSIST_MS = 1000
ERR_NO_CONN = CR.ERR_NO_CONN
NONE = A.CONN_NONE
NOT_DELIVERED = -2**31
FRAME = 14 + 20 + 20
MUTANTS = ("flag_from_syn", "last_syn_wins", "no_purge", "unreversed", "ack_from_seq", "retry_refused",
           "second_key_takes", "swapped_addresses")

INPUTS = ("n_groups", "ids", "capacity", "deviation", "ev_kind", "ev_ts", "ev_lo", "ev_hi", "ev_arg",
          "syn_src", "syn_dst", "syn_sport", "syn_dport", "syn_seq", "syn_ack", "syn_flags", "acc_tuple",
          "d_src", "d_dst", "d_sport", "d_dport", "d_seq", "d_flags", "d_group", "d_key", "s_draws")
RECORDED = {"r_ret": np.int32, "r_created": np.uint8, "r_conn": np.int32, "r_ack": np.uint32,
            "c_group": np.int32, "c_key": np.uint64, "c_packet": np.uint32, "c_info": np.uint32,
            "pa_off": np.uint32, "pa_rows": np.uint32, "pa_exp": np.uint64, "pn_off": np.uint32, "pn_rows": np.uint32,
            "pn_exp": np.uint64, "closed": np.uint32, "s_sender": np.uint64, "s_consumed": np.uint32}


# ---- storage ---------------------------------------------------------------------------------------------------
# Deflate cannot shrink a column of 32-bit numbers that follows another one; the difference of the two it can.  The
# fixture stores these recorded columns as their difference (modulo 2^32) to an INPUT column of the same packet or
# to another recorded column.  Lossless: pack / unpack are inverses and the generator checks the round trip.
def _seq_after(s):  # the TcpInfo.seq RawInput hands over: th_seq + the payload length
    return s["d_seq"].astype(np.int64) + PAYLOAD


def pack(s: dict) -> dict:
    out = dict(s)
    out["r_ack"] = (s["r_ack"].astype(np.int64) - np.where(s["r_conn"] >= 0, _seq_after(s), 0)).astype(np.uint32)
    info = s["c_info"].astype(np.int64).reshape(-1, 7).copy()
    info[:, 5] -= info[:, 4]  # ack after Init rides on seq after Init
    out["c_info"] = info.astype(np.uint32)
    return out


def unpack(z: dict) -> dict:
    s = dict(z)
    s["r_ack"] = (z["r_ack"].astype(np.int64) + np.where(z["r_conn"] >= 0, _seq_after(z), 0)).astype(np.uint32)
    info = z["c_info"].astype(np.int64).reshape(-1, 7).copy()
    info[:, 5] += info[:, 4]
    s["c_info"] = info.astype(np.uint32)
    return s


@functools.lru_cache(maxsize=None)
def _npz():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def names(deviation=None) -> list[str]:
    out = _npz()["names"].tolist()
    return [n for n in out if deviation is None or bool(script(n)["deviation"]) == deviation]


@functools.lru_cache(maxsize=None)
def script(name: str) -> dict:
    z = _npz()
    p = f"s{z['names'].tolist().index(name)}_"
    return unpack({k[len(p):]: v for k, v in z.items() if k.startswith(p)})


def capacities(s: dict) -> list[int]:
    """The table sizes a script runs at: both where its conns fit the small one."""
    return [257, 4097] if int(s["capacity"]) == 257 else [4097]


# ---- packets ---------------------------------------------------------------------------------------------------
def frames(src, dst, sport, dport, seq, ack, flags, payload) -> np.ndarray:
    """Ethernet / IPv4 / TCP captures without options (RFC 791 / 793 layouts), one per row: [n, 54 + payload].
    src / dst are addresses as s_addr holds them (network order in memory); checksums zero, as the parse ignores
    them."""
    n = len(src)
    f = np.zeros((n, FRAME + payload), np.uint8)
    f[:, 0:6], f[:, 6:12], f[:, 12], f[:, 13] = 2, 4, 0x08, 0x00
    ip = f[:, 14:34]
    ip[:, 0] = 0x45
    tot = 40 + payload
    ip[:, 2], ip[:, 3] = tot >> 8, tot & 255
    ip[:, 4], ip[:, 5], ip[:, 6], ip[:, 8], ip[:, 9] = 0x12, 0x34, 0x40, 64, 6
    ip[:, 12:16] = np.ascontiguousarray(src, np.uint32).view(np.uint8).reshape(n, 4)
    ip[:, 16:20] = np.ascontiguousarray(dst, np.uint32).view(np.uint8).reshape(n, 4)
    t = f[:, 34:54]
    be16 = lambda a: np.ascontiguousarray(a, np.uint16).astype(">u2").view(np.uint8).reshape(n, 2)  # noqa: E731
    be32 = lambda a: np.ascontiguousarray(a, np.uint32).astype(">u4").view(np.uint8).reshape(n, 4)  # noqa: E731
    t[:, 0:2], t[:, 2:4], t[:, 4:8], t[:, 8:12] = be16(sport), be16(dport), be32(seq), be32(ack)
    t[:, 12], t[:, 13] = 0x50, np.ascontiguousarray(flags, np.uint8)
    t[:, 14], t[:, 15] = 0xFF, 0xFF
    return f


def syn_frames(s, lo, hi):
    c = lambda k: s[k][lo:hi]  # noqa: E731
    return frames(c("syn_src"), c("syn_dst"), c("syn_sport"), c("syn_dport"), c("syn_seq"), c("syn_ack"), c("syn_flags"), 0)


def data_frames(s, lo, hi):
    c = lambda k: s[k][lo:hi]  # noqa: E731
    return frames(c("d_src"), c("d_dst"), c("d_sport"), c("d_dport"), c("d_seq"), np.ones(hi - lo, np.uint32),
                  c("d_flags"), PAYLOAD)


def events(s):
    return list(zip(s["ev_kind"].tolist(), s["ev_ts"].tolist(), s["ev_lo"].tolist(), s["ev_hi"].tolist(),
                    s["ev_arg"].tolist()))


# ---- the reference run --------------------------------------------------------------------------------------------
def run_reference(s: dict) -> dict:
    """The script's inputs through the reference (needs oracle/_ref): -> the recorded columns, typed."""
    from tests.oracle_lib import RefConnCreate

    ref = RefConnCreate(int(s["n_groups"]), PERSIST_MS)
    n = len(s["d_key"])
    out = {"r_ret": np.zeros(n, np.int32), "r_created": np.zeros(n, np.uint8), "r_conn": np.full(n, -1, np.int32),
           "r_ack": np.zeros(n, np.uint32)}
    pa, pae, pn, pne, pa_off, pn_off, closed = [], [], [], [], [0], [0], []
    senders, consumed = [], []
    try:
        for kind, ts, lo, hi, arg in events(s):
            if kind == EV_SYN:
                ref.syn([bytes(f) for f in syn_frames(s, lo, hi)], ts)
            elif kind == EV_ACCEPT:
                ref.accept(s["acc_tuple"][lo:hi], ts)
            elif kind == EV_DATA:
                d = ref.data([bytes(f) for f in data_frames(s, lo, hi)], s["d_group"][lo:hi], s["d_key"][lo:hi])
                assert not (d["ret"] == NOT_DELIVERED).any(), "RawInput did not hand a DATA packet over"
                assert np.array_equal(d["info"][:, 4], (s["d_seq"][lo:hi] + np.uint32(PAYLOAD)).astype(np.uint32))
                out["r_ret"][lo:hi], out["r_created"][lo:hi] = d["ret"], d["created"]
                out["r_conn"][lo:hi], out["r_ack"][lo:hi] = d["conn"], d["ack"]
            elif kind in (EV_FLUSH_ACK, EV_FLUSH_NET):
                ref.flush(kind - EV_FLUSH_ACK, ts)
            else:
                o = ref.send(arg, s["s_draws"][lo:hi])
                senders.append(o["sender"])
                consumed.append(o["consumed"])
            p = ref.pools()
            pa.append(p["ack"]); pae.append(p["ack_exp"]); pn.append(p["net"]); pne.append(p["net_exp"])
            pa_off.append(pa_off[-1] + len(p["ack"])); pn_off.append(pn_off[-1] + len(p["net"]))
            closed.append(p["closed"])
        c = ref.conns()
    finally:
        ref.close()
    # a conn's packet as an index into the script's DATA columns: creation order is packet order
    made = np.nonzero(out["r_created"] == 2)[0]
    assert len(made) == len(c["key"])
    cat = lambda a, dt, w=None: (np.concatenate(a) if a else np.zeros((0,) if w is None else (0, w))).astype(dt)  # noqa: E731
    out.update(c_group=c["group"].astype(np.int32), c_key=c["key"], c_packet=made.astype(np.uint32), c_info=c["info"],
               pa_off=np.array(pa_off, np.uint32), pa_rows=cat(pa, np.uint32, 6), pa_exp=cat(pae, np.uint64),
               pn_off=np.array(pn_off, np.uint32), pn_rows=cat(pn, np.uint32, 4), pn_exp=cat(pne, np.uint64),
               closed=np.array(closed, np.uint32), s_sender=cat(senders, np.uint64), s_consumed=cat(consumed, np.uint32))
    return {k: np.ascontiguousarray(out[k], dt) for k, dt in RECORDED.items()}


# ---- what the documented rule is expected to give -----------------------------------------------------------------
def expected(s: dict) -> dict:
    """Per DATA packet the conn (creation ordinal, -1 none) the batch rule reaches, per conn the packet that makes
    it; `moved` = the conns the reference made at a later packet of a key its first packet left refused (the
    documented deviation): the batch rule makes them at the key's first packet of the next batch that carries it.
    `pending` [(first event, last event, ordinal)]: the events after which such a conn's offer is still unconsumed."""
    conn, packet = s["r_conn"].copy(), s["c_packet"].astype(np.int64).copy()
    moved, pending = [], []
    ev = events(s)
    batches = [(e, lo, hi) for e, (kind, _ts, lo, hi, _a) in enumerate(ev) if kind == EV_DATA]
    for b, (e, lo, hi) in enumerate(batches):
        gk = list(zip(s["d_group"][lo:hi].tolist(), s["d_key"][lo:hi].tolist()))
        first = {}
        for i, k in enumerate(gk):
            first.setdefault(k, lo + i)
        for o in np.nonzero((packet >= lo) & (packet < hi))[0].tolist():
            k = (int(s["c_group"][o]), int(s["c_key"][o]))
            if k not in first or first[k] == packet[o] or s["r_conn"][first[k]] >= 0:
                continue
            moved.append(o)
            at = np.nonzero((s["d_group"][lo:hi] == k[0]) & (s["d_key"][lo:hi] == np.uint64(k[1])))[0] + lo
            conn[at] = -1
            nxt = None
            for e2, lo2, hi2 in batches[b + 1:]:
                at2 = np.nonzero((s["d_group"][lo2:hi2] == k[0]) & (s["d_key"][lo2:hi2] == np.uint64(k[1])))[0]
                if len(at2):
                    nxt = (e2, lo2 + int(at2[0]))
                    break
            assert nxt is not None, "a deviation script must show the key again in a later batch"
            packet[o] = nxt[1]
            pending.append((e, nxt[0] - 1, o))
    return {"conn": conn, "packet": packet, "moved": moved, "pending": pending}


# ---- the devices under test -------------------------------------------------------------------------------------
def empty_table(capacity: int) -> dict:
    """A BY_ID table without a LIVE row: every other bit and column random."""
    rng = np.random.default_rng(capacity)
    cols = CR.random_columns(rng, capacity, by_id=True)
    cols["state"][:] = rng.choice(np.array([0, R.ALIVE, R.NEW], np.uint8), capacity)
    return cols


def parse_cpu(oracle, f: np.ndarray, flags: int) -> dict:
    """tests/oracle_lib.Oracle.rawinput (pinned to the reference by tests/golden/parse.npz) over the rows of f."""
    n = len(f)
    out = {k: np.zeros(n, dt) for k, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
                                            ("seq", np.uint32), ("ack", np.uint32), ("flag", np.uint8), ("parse_status", np.int8))}
    w = f.shape[1]
    for i in range(n):
        t = oracle.rawinput(f[i].tobytes() + bytes(64), w, w, 1, flags)
        for k in out:
            out[k][i] = getattr(t, k)
    return out


def table_rows(tab) -> dict:
    """A ConnTable's columns as numpy."""
    cols = (("state", np.uint8), ("conn_key", np.uint64), ("id", np.uint8), ("src", np.uint32), ("dst", np.uint32),
            ("sp", np.uint16), ("dp", np.uint16), ("seq", np.uint32), ("ack", np.uint32), ("flag", np.uint8))
    return {k: K.host(getattr(tab, k), dt) for k, dt in cols if getattr(tab, k) is not None}


class Twin:
    """The library: device "cpu" = the host twins (parse: the oracle), a cuda device = the batch calls of `codec`."""

    def __init__(self, rc, capacity, device="cpu", codec=None, oracle=None):
        self.rc, self.device, self.codec, self.oracle = rc, device, codec, oracle
        self.h = R.Harness(rc, empty_table(capacity), True, device, codec)

    def parse(self, f, flags):
        if self.codec is None:
            return parse_cpu(self.oracle, f, flags)
        import torch

        n, w = f.shape
        dev = self.device
        cap = P.tensor(np.concatenate([f.reshape(-1), np.zeros(64, np.uint8)]), dev)
        off = torch.arange(n, dtype=torch.int64, device=dev) * w
        ln = torch.full((n,), w, dtype=torch.int32, device=dev)
        tcp, dec = self.rc.TcpInfoBuffers.alloc(n, dev), self.rc.DecodeBuffers.alloc(n, dev)
        self.codec.rawinput_batch(cap, off, ln, ln, 1, flags, tcp, dec)
        torch.cuda.synchronize()
        th = tcp.to_host()
        return {k: th[k].view(dt) for k, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
                                                ("seq", np.uint32), ("ack", np.uint32), ("flag", np.uint8),
                                                ("parse_status", np.int8))}

    def batch(self, b, offers, n_offer):
        """resolve -> conn_create -> recv_ack; -> the create's outputs."""
        h, n = self.h, len(b["conn_key"])
        status = np.full(n, A.RECV_VALID, np.int8)
        if self.codec is None:
            conn, hit, miss, _ = self.rc.conn_resolve_host(h.tab, status, b["conn_key"], id=b["id"])
        else:
            import torch

            e = lambda dt: torch.empty(n, dtype=dt, device=self.device)  # noqa: E731
            conn, hit, miss, nm = e(torch.int32), e(torch.uint8), e(torch.int8), torch.empty(1, dtype=torch.int32, device=self.device)
            self.codec.conn_resolve_batch(h.tab, h.t(status, np.int8), h.t(b["conn_key"], np.uint64), conn, id=h.t(b["id"], np.uint8),
                                          hit=hit, miss=miss, n_miss=nm)
            torch.cuda.synchronize()
            conn, hit, miss = K.host(conn, np.uint32), K.host(hit, np.uint8), K.host(miss, np.int8)
        m_max = max(len(offers["src"]), 1)
        got = h.raw_create(offers, n_offer, m_max, b, conn, hit, miss, u_max=n, now_ms=1)
        if self.codec is None:
            ack = self.oracle.tcp_recv_ack_batch(got["conn"], got["hit"], b["seq"], K.host(h.tab.ack, np.uint32))
            h.tab.load(ack=ack)
        else:
            self.codec.tcp_recv_ack_batch(h.t(got["conn"], np.uint32), h.t(got["hit"], np.uint8), h.t(b["seq"], np.uint32), h.tab.ack)
            torch.cuda.synchronize()
        return got

    def rows(self):
        return table_rows(self.h.tab)

    def pick(self, id8, draws):
        n = len(draws)
        conn, n_none, _ = P.run_pick(self.rc, self.h.tab, n, self.device, self.codec, id=np.tile(id8, n), draw=draws)
        assert n_none == int((conn == NONE).sum())
        return conn


class Model:
    """The rule in Python: conn_create_ref.create_ref, or (walk=True, or a mutant of the create rule) the packet walk
    below; conn_ref.resolve_ref, FakeTcp::OnRecv's compare and pick_ref.rule_ref around it."""

    def __init__(self, capacity, oracle, mutant=None, walk=False):
        self.cols, self.oracle, self.mutant = empty_table(capacity), oracle, mutant
        self.walk = walk or mutant in ("retry_refused", "second_key_takes", "swapped_addresses")

    def parse(self, f, flags):
        return parse_cpu(self.oracle, f, flags)

    def batch(self, b, offers, n_offer):
        cols, n = self.cols, len(b["conn_key"])
        tmap, _ = CR.table_map(cols["state"], cols["conn_key"], cols["id"])
        conn, hit, miss, _ = CR.resolve_ref(tmap, np.full(n, A.RECV_VALID, np.int8), b["conn_key"], id=b["id"])
        if self.walk:
            got = walk(cols, offers, n_offer, b, miss, conn, hit, self.mutant)
        else:
            got = R.create_ref(cols, True, offers, n_offer, max(len(offers["src"]), 1), b, miss, conn, hit, n)
        cols = self.cols = got["cols"]
        for i in np.nonzero(got["hit"])[0].tolist():  # FakeTcp::OnRecv: a plain unsigned compare
            r = int(got["conn"][i])
            if cols["ack"][r] < b["seq"][i]:
                cols["ack"][r] = b["seq"][i]
        return {k: (np.array([got[k]], np.uint32) if k.startswith("n_") else got[k]) for k in
                ("conn", "hit", "miss", "n_new", "n_full", "n_refused", "new_rows", "new_first", "new_offer")}

    def rows(self):
        return self.cols

    def pick(self, id8, draws):
        n = len(draws)
        return P.rule_ref(self.cols, True, n, id=np.tile(id8, n), draw=draws)[0]


def walk(cols, offers, n_offer, b, miss, conn, hit, mutant=None):
    """INetGroup::Input's miss path in packet order with the two batch rules of the header (a key is decided at its
    first missing packet; an offer is taken once), each of which a mutant can bend."""
    cols = {k: v.copy() for k, v in cols.items()}
    miss, conn, hit = miss.copy(), conn.copy(), hit.copy()
    w = CR.id_words(b["id"], len(miss))
    vacant = iter(np.nonzero((cols["state"] & R.LIVE) == 0)[0].tolist())
    tuple_offer = {}
    for o in range(n_offer):
        tuple_offer.setdefault(tuple(int(offers[k][o]) for k in ("src", "sp", "dst", "dp")), o)
    taken, decided, made, refused = set(), set(), {}, set()
    new_rows, new_first, new_offer = [], [], []
    for i in np.nonzero(miss == A.RECV_VALID)[0].tolist():
        k = (int(w[i]), int(b["conn_key"][i]))
        if k in made or (k in decided and mutant != "retry_refused"):
            continue
        decided.add(k)
        o = tuple_offer.get(tuple(int(b[c][i]) for c in ("src", "sp", "dst", "dp")))
        if o is None or (o in taken and mutant != "second_key_takes"):
            refused.add(k)
            continue
        taken.add(o)
        row = next(vacant)
        cols["conn_key"][row] = k[1]
        cols["id"].reshape(-1, 8)[row] = np.array([k[0]], np.uint64).view(np.uint8)
        names = ("dst", "src", "dp", "sp") if mutant == "swapped_addresses" else ("src", "dst", "sp", "dp")
        for c, f in zip(("src", "dst", "sp", "dp"), names):
            cols[c][row] = offers[f][o]
        cols["flag"][row] = offers["flag"][o]
        cols["seq"][row] = (int(offers["ack"][o]) + 1) & 0xFFFFFFFF
        cols["ack"][row] = (int(offers["ack"][o]) + 2) & 0xFFFFFFFF
        cols["state"][row] = R.BORN
        made[k] = row
        refused.discard(k)
        new_rows.append(row); new_first.append(i); new_offer.append(o)
    for i in np.nonzero(miss == A.RECV_VALID)[0].tolist():
        row = made.get((int(w[i]), int(b["conn_key"][i])))
        if row is not None:
            conn[i], hit[i], miss[i] = row, 1, A.RECV_DROP
    u32 = lambda a: np.array(a, np.uint32)  # noqa: E731
    return {"cols": cols, "conn": conn, "hit": hit, "miss": miss, "n_new": len(new_rows), "n_full": 0, "n_refused": len(refused),
            "new_rows": u32(new_rows), "new_first": u32(new_first), "new_offer": u32(new_offer)}


# ---- the documented host procedure ----------------------------------------------------------------------------------
class HostModel:
    """What INTEGRATION.md tells the host to keep around rsk_conn_create_batch: the two pools (4-tuple in the
    orientation of a DATA packet's TcpInfo -> the record), the join that makes the offers, the after-batch rules."""

    def __init__(self, mutant=None):
        self.ack, self.net, self.closed, self.mutant = {}, {}, 0, mutant

    def harvest(self, t, ts):
        """The parse's rows of a batch of SYN captures: a record per RSK_PARSE_SYN row whose ports are not 0; the
        FIRST handshake of a tuple keeps its numbers, a later one only moves the expiry."""
        for i in np.nonzero(t["parse_status"] == PARSE_SYN)[0].tolist():
            if int(t["sp"][i]) == 0 or int(t["dp"][i]) == 0:
                continue
            k = (int(t["src"][i]), int(t["sp"][i]), int(t["dst"][i]), int(t["dp"][i]))
            rec = self.ack.get(k)
            if rec is None or self.mutant == "last_syn_wins":
                rec = self.ack[k] = {"seq": int(t["seq"][i]), "ack": int(t["ack"][i]), "flag": int(t["flag"][i])}
            rec["exp"] = ts + PERSIST_MS

    def accept(self, tuples, ts):
        for src, dst, sp, dp in np.asarray(tuples).tolist():
            self.net.setdefault((src, sp, dst, dp), ts + PERSIST_MS)

    def offers(self):
        """-> (offer columns, n_offer, the tuples in offer order)."""
        keys = sorted(k for k in self.ack if k in self.net)
        rec = [self.ack[k] for k in keys]
        col = lambda v, dt: np.array(v if keys else [0], dt)  # noqa: E731
        o = {"src": col([k[0] for k in keys], np.uint32), "sp": col([k[1] for k in keys], np.uint16),
             "dst": col([k[2] for k in keys], np.uint32), "dp": col([k[3] for k in keys], np.uint16),
             "ack": col([r["seq" if self.mutant == "ack_from_seq" else "ack"] for r in rec], np.uint32),
             "flag": col([r["flag"] if self.mutant == "flag_from_syn" else TH_ACK for r in rec], np.uint8)}
        return o, len(keys), keys

    def after_batch(self, keys, got, b):
        """new_offer[j]: the socket is the conn's, both entries go.  A packet still in miss: what its tuple has in
        either pool goes, and a socket among it is closed -- unless the tuple is a whole offer this call did not
        consume (the documented deviation, or a full table)."""
        for o in got["new_offer"][: int(got["n_new"][0])].tolist():
            self.ack.pop(keys[o], None)
            self.net.pop(keys[o], None)
        if self.mutant == "no_purge":
            return
        for i in np.nonzero(got["miss"] == A.RECV_VALID)[0].tolist():
            k = (int(b["src"][i]), int(b["sp"][i]), int(b["dst"][i]), int(b["dp"][i]))
            if k in self.ack and k in self.net:
                continue
            self.ack.pop(k, None)
            if self.net.pop(k, None) is not None:
                self.closed += 1

    def flush(self, kind, ts):
        if kind == EV_FLUSH_ACK:  # TcpAckPool::OnFlush: expiry <= ts
            self.ack = {k: r for k, r in self.ack.items() if r["exp"] > ts}
        else:                     # ServerNetManager::OnFlush: ts >= expiry, the socket closed
            gone = [k for k, e in self.net.items() if ts >= e]
            for k in gone:
                del self.net[k]
            self.closed += len(gone)

    def snapshot(self):
        """Both pools in the reference's map order (TcpCmpFn: src, sp, dst, dp)."""
        ak, nk = sorted(self.ack), sorted(self.net)
        a = np.array([[k[0], k[2], k[1], k[3], self.ack[k]["seq"], self.ack[k]["ack"]] for k in ak], np.uint32).reshape(-1, 6)
        n = np.array([[k[0], k[2], k[1], k[3]] for k in nk], np.uint32).reshape(-1, 4)
        return (a, np.array([self.ack[k]["exp"] for k in ak], np.uint64), n, np.array([self.net[k] for k in nk], np.uint64),
                self.closed)


# ---- the checker ---------------------------------------------------------------------------------------------------
def check(s: dict, dev, mutant=None) -> dict:
    """Replay script s on `dev` by the documented procedure and compare with the record.  -> counts of what was
    compared.  An AssertionError names the first difference."""
    host = HostModel(mutant)
    exp = expected(s)
    assert bool(exp["moved"]) == bool(s["deviation"]), "only a deviation script may deviate, and it must"
    ids = np.ascontiguousarray(s["ids"], np.uint8).reshape(-1, 8)
    row_of = {}   # creation ordinal -> row
    born = 0      # conns made so far, in the expected order
    order = np.argsort(exp["packet"], kind="stable")  # the expected creation order
    seen = {"packets": 0, "conns": 0, "snapshots": 0, "sends": 0, "refused": 0}
    send_at = 0
    for e, (kind, ts, lo, hi, arg) in enumerate(events(s)):
        if kind == EV_SYN:
            t = dev.parse(syn_frames(s, lo, hi), 1 if mutant == "unreversed" else PARSE_FLAGS)
            assert bool((t["parse_status"] == PARSE_SYN).all()), "a SYN capture the parse does not report as one"
            host.harvest(t, ts)
        elif kind == EV_ACCEPT:
            host.accept(s["acc_tuple"][lo:hi], ts)
        elif kind in (EV_FLUSH_ACK, EV_FLUSH_NET):
            host.flush(kind, ts)
        elif kind == EV_DATA:
            t = dev.parse(data_frames(s, lo, hi), PARSE_FLAGS)
            assert bool((t["parse_status"] == PARSE_DELIVER).all())
            b = {k: t[k] for k in ("src", "dst", "sp", "dp", "seq")}
            b["conn_key"] = s["d_key"][lo:hi]
            b["id"] = np.ascontiguousarray(ids[s["d_group"][lo:hi]]).reshape(-1)
            offers, n_offer, keys = host.offers()
            got = dev.batch(b, offers, n_offer)
            host.after_batch(keys, got, b)
            # the conns born here, in creation order
            mine = [o for o in order[born:].tolist() if lo <= exp["packet"][o] < hi]
            assert int(got["n_new"][0]) == len(mine), ("n_new", int(got["n_new"][0]), len(mine))
            assert int(got["n_full"][0]) == 0
            assert got["new_first"][: len(mine)].tolist() == [int(exp["packet"][o]) - lo for o in mine], "new_first"
            rows = dev.rows()
            for j, o in enumerate(mine):
                r = int(got["new_rows"][j])
                row_of[o] = r
                info = s["c_info"][o]
                want = (int(s["c_key"][o]), ids[s["c_group"][o]].tobytes(), *info[[0, 1, 2, 3, 6, 4]].tolist(), R.BORN)
                have = (int(rows["conn_key"][r]), rows["id"].reshape(-1, 8)[r].tobytes(), int(rows["src"][r]), int(rows["dst"][r]),
                        int(rows["sp"][r]), int(rows["dp"][r]), int(rows["flag"][r]), int(rows["seq"][r]), int(rows["state"][r]))
                assert have == want, ("row", o, have, want)
                # the offer's ack is the record's: ack after Init = it + 2, before any packet moved it
                assert (int(offers["ack"][got["new_offer"][j]]) + 2) & 0xFFFFFFFF == int(info[5]), ("ack after Init", o)
            born += len(mine)
            seen["conns"] += len(mine)
            # conn / hit / miss per packet
            ec = exp["conn"][lo:hi]
            want_conn = np.array([row_of[c] if c >= 0 else NONE for c in ec.tolist()], np.uint32)
            assert np.array_equal(got["conn"], want_conn), ("conn", np.nonzero(got["conn"] != want_conn)[0][:8])
            assert np.array_equal(got["hit"], (ec >= 0).astype(np.uint8)), "hit"
            assert np.array_equal(got["miss"], np.where(ec >= 0, A.RECV_DROP, A.RECV_VALID).astype(np.int8)), "miss"
            same = exp["conn"][lo:hi] == s["r_conn"][lo:hi]  # everywhere but at a moved conn's packets
            assert np.array_equal((s["r_ret"][lo:hi] == ERR_NO_CONN)[same], (ec < 0)[same])
            assert bool((s["r_ret"][lo:hi][ec >= 0] == PAYLOAD).all())
            refused = {(int(g), int(k)) for g, k, c in zip(s["d_group"][lo:hi], s["d_key"][lo:hi], ec) if c < 0}
            assert int(got["n_refused"][0]) == len(refused), ("n_refused", int(got["n_refused"][0]), len(refused))
            seen["refused"] += len(refused)
            # the rows' ack after recv_ack: the reference's mInfo.ack behind the conn's last packet of the batch
            last = {}
            for i, c in enumerate(ec.tolist()):
                if c >= 0:
                    last[c] = lo + i
            unmoved = [c for c in last if c not in exp["moved"]]
            assert [int(rows["ack"][row_of[c]]) for c in unmoved] == [int(s["r_ack"][last[c]]) for c in unmoved], "ack"
            seen["packets"] += hi - lo
        else:
            draws = s["s_draws"][lo:hi]
            rows = dev.rows()
            assert bool((s["s_consumed"][lo:hi] == 1).all())
            # doSend walks the group's conns in the string order of their keys: the script keeps that the row order
            grp = [r for o, r in sorted(row_of.items(), key=lambda x: x[1]) if int(s["c_group"][o]) == arg]
            keys_in_rows = [int(rows["conn_key"][r]) for r in grp]
            assert keys_in_rows == sorted(keys_in_rows, key=str), "the send script's keys do not stand in string order"
            conn = dev.pick(ids[arg], draws)
            assert [int(rows["conn_key"][r]) for r in conn.tolist()] == s["s_sender"][lo:hi].tolist(), "pick"
            assert bool(np.isin(conn, grp).all())
            seen["sends"] += hi - lo
        # both pools after the event; a moved conn's offer is still whole here, consumed there
        a, ae, n, ne, closed = host.snapshot()
        ra, rae = s["pa_rows"][s["pa_off"][e]:s["pa_off"][e + 1]], s["pa_exp"][s["pa_off"][e]:s["pa_off"][e + 1]]
        rn, rne = s["pn_rows"][s["pn_off"][e]:s["pn_off"][e + 1]], s["pn_exp"][s["pn_off"][e]:s["pn_off"][e + 1]]
        for e0, e1, o in exp["pending"]:
            if e0 <= e <= e1:
                tup = s["c_info"][o][:4]
                keep_a = ~(a[:, :4] == tup).all(axis=1)
                keep_n = ~(n == tup).all(axis=1)
                assert int((~keep_a).sum()) == 1 and int((~keep_n).sum()) == 1, "the moved conn's offer is not held"
                a, ae, n, ne = a[keep_a], ae[keep_a], n[keep_n], ne[keep_n]
        assert np.array_equal(a, ra) and np.array_equal(ae, rae), ("ack pool after event", e, a.tolist()[:4], ra.tolist()[:4])
        assert np.array_equal(n, rn) and np.array_equal(ne, rne), ("socket pool after event", e, n.tolist()[:4], rn.tolist()[:4])
        assert closed == int(s["closed"][e]), ("sockets closed after event", e, closed, int(s["closed"][e]))
        seen["snapshots"] += 1
    assert born == len(s["c_key"])
    return seen


# ---- the client's list form ------------------------------------------------------------------------------------------
def client_case(k):
    z = _npz()
    return {f[len(f"c{k}_"):]: v for f, v in z.items() if f.startswith(f"c{k}_")}


def client_offers(c, oracle):
    """The documented client procedure: the handshakes harvested from the parse (ack pool, no server flag), one
    list-form offer per dialled socket with the key KeyForConnInfo makes of its ports, flag TH_ACK."""
    from rsock_amd.codec import key_for_tcp

    k = len(c["key"])
    f = frames(c["syn_src"], c["syn_dst"], c["syn_sport"], c["syn_dport"], c["syn_seq"], c["syn_ack"],
               np.full(k, 0x12, np.uint8), 0)
    t = parse_cpu(oracle, f, 1)
    assert bool((t["parse_status"] == PARSE_SYN).all())
    pool = {(int(t["src"][i]), int(t["sp"][i]), int(t["dst"][i]), int(t["dp"][i])): int(t["ack"][i]) for i in range(k)}
    tup = c["tuple"]
    ack = [pool[(int(a), int(sp), int(b), int(dp))] for a, b, sp, dp in tup.tolist()]
    key = [key_for_tcp(int(sp), int(dp)) for _a, _b, sp, dp in tup.tolist()]
    return {"src": tup[:, 0].astype(np.uint32), "dst": tup[:, 1].astype(np.uint32), "sp": tup[:, 2].astype(np.uint16),
            "dp": tup[:, 3].astype(np.uint16), "ack": np.array(ack, np.uint32), "flag": np.full(k, TH_ACK, np.uint8),
            "conn_key": np.array(key, np.uint64), "id": np.zeros(8 * k, np.uint8)}


def check_client(c, offers, rows, new_rows):
    k = len(c["key"])
    assert np.array_equal(offers["conn_key"], c["key"]), "KeyForConnInfo"
    assert len(new_rows) == k
    r = new_rows.astype(np.int64)
    assert np.array_equal(rows["conn_key"][r], c["key"])
    for j, col in enumerate(("src", "dst", "sp", "dp", "seq", "ack", "flag")):
        assert np.array_equal(rows[col][r].astype(np.uint32), c["info"][:, j]), col
    assert bool((rows["state"][r] == R.BORN).all())
