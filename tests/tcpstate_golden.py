"""TEST INFRASTRUCTURE: tests/golden/tcpstate.npz, what the REFERENCE's own FakeTcp / RConn / RawTcp did with
scripts of sends and receives (oracle/ref_tcpstate_harness.cpp through tests/oracle_lib.RefTcpState), and the
helpers the CPU and GPU tests share: the script reader, the table state after each batch, a packet-by-packet
model whose mutants show the fixture discriminates, and a plain IPv4 / TCP header unpacker.

A script is K conns (the TcpInfo and key each FakeTcp was made from), a start value of RawTcp::mIpId and
events in batches; a batch is all sends or all receives.
  send      conn, a = nread, the payload at arena[pay_off : pay_off + nread], conv for the head
  receive   conn, a = the packet's TcpInfo.seq, b = what the upstream OnRecv callback returns
Recorded per event: `ret` (FakeTcp::Output's / IConn::Input's return), the number of libnet calls, every
argument of libnet_build_tcp (t_*) and libnet_build_ipv4 (i_*), mInfo.seq / mInfo.ack (conn_seq / conn_ack)
and mIpId (ip_id_next) afterwards; scripts with frame_cap > 0 also hold `frames`, the bytes behind
libnet_build_tcp's payload pointer.  state0 is each conn's (mInfo.seq, mInfo.ack) after FakeTcp::Init."""
from __future__ import annotations

import os

import numpy as np

from rsock_amd import _abi as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tcpstate.npz")
KEY = b"hello135"
SEND, RECV = 0, 1
HEAD = 31  # RSK_HEAD_SIZE; the fixture's head_size is the reference's RConn::HEAD_SIZE
MAX_PAYLOAD = 1469

INPUTS = ("info", "key", "ip_id0", "id8", "kind", "conn", "a", "b", "conv", "arena", "pay_off", "batch_off",
          "frame_cap")
# recorded columns and the narrowest type each value fits (the generator checks the cast loses nothing)
RECORDED = {"ret": np.int32, "n_tcp": np.uint8, "n_ip": np.uint8, "n_write": np.uint8, "conn_seq": np.uint32,
            "conn_ack": np.uint32, "ip_id_next": np.uint16,
            "t_sp": np.uint16, "t_dp": np.uint16, "t_seq": np.uint32, "t_ack": np.uint32, "t_control": np.uint8,
            "t_win": np.uint16, "t_sum": np.uint16, "t_urg": np.uint16, "t_len": np.uint16, "t_payload_s": np.uint32,
            "t_ptag": np.int32, "t_payload_set": np.uint8,
            "i_len": np.uint16, "i_tos": np.uint8, "i_id": np.uint16, "i_frag": np.uint16, "i_ttl": np.uint8,
            "i_prot": np.uint8, "i_sum": np.uint16, "i_src": np.uint32, "i_dst": np.uint32, "i_payload_set": np.uint8,
            "i_payload_s": np.uint32, "i_ptag": np.int32}

# The fixture stores these recorded columns as their difference (modulo the column's width) to another value of
# the SAME event (a column, or the event's conn's TcpInfo row), (ip_id_next) to the event before, or (state0) to
# the conn's info.ack: deflate cannot shrink a ramp or two columns that move together, a difference of them it can.  Lossless: pack / unpack are inverses, and the generator checks that
# unpack gives back exactly what the reference recorded.  Order matters: a column's partner is unpacked first.
def _row(col):
    return lambda s: np.asarray(s["info"])[s["conn"], col].astype(np.int64)


def _sent_row(col):
    return lambda s: s["n_tcp"] * np.asarray(s["info"])[s["conn"], col].astype(np.int64)


PACKED = (("conn_seq", _row(5)), ("conn_ack", _row(5)), ("t_sp", _sent_row(2)), ("t_dp", _sent_row(3)),
          ("i_src", _sent_row(0)), ("i_dst", _sent_row(1)), ("t_control", _sent_row(6)),
          ("ret", lambda s: np.where(s["kind"] == SEND, s["a"].astype(np.int64), s["b"].astype(np.int64))),
          ("t_payload_s", lambda s: s["n_tcp"] * s["ret"].astype(np.int64)),
          ("t_len", lambda s: s["t_payload_s"].astype(np.int64)),
          ("i_len", lambda s: s["t_payload_s"].astype(np.int64)),
          ("i_id", lambda s: s["n_ip"] * s["ip_id_next"].astype(np.int64)),
          ("t_seq", lambda s: s["n_tcp"] * s["conn_seq"].astype(np.int64)),
          ("t_ack", lambda s: s["n_tcp"] * s["conn_ack"].astype(np.int64)))


def pack(s: dict) -> dict:
    """Recorded columns -> stored columns (a new dict; the inputs ride along)."""
    out = dict(s)
    for k, partner in PACKED:
        out[k] = (s[k].astype(np.int64) - partner(s)).astype(RECORDED[k])
    out["state0"] = s["state0"] - np.asarray(s["info"])[:, 5:6].astype(np.uint32)
    nxt = s["ip_id_next"].astype(np.int64)
    out["ip_id_next"] = np.diff(nxt, prepend=int(s["ip_id0"])).astype(np.uint16)
    return out


def unpack(z: dict) -> dict:
    s = dict(z)
    s["ip_id_next"] = (int(z["ip_id0"]) + np.cumsum(z["ip_id_next"].astype(np.int64))).astype(np.uint16)
    for k, partner in PACKED:  # in order: a column's partner is complete before it is used
        s[k] = (z[k].astype(np.int64) + partner(s)).astype(RECORDED[k])
    s["state0"] = z["state0"] + np.asarray(z["info"])[:, 5:6].astype(np.uint32)
    return s


_z = None
_scripts: dict = {}


def _load():
    global _z
    if _z is None:
        with np.load(GOLDEN) as z:
            _z = {k: z[k] for k in z.files}
    return _z


def names(kind: str | None = None) -> list[str]:
    """Script names; kind "send" / "recv" / "mixed" / "frames" (scripts that recorded frame bytes) filters."""
    out = _load()["names"].tolist()
    if kind == "frames":
        return [n for n in out if int(script(n)["frame_cap"]) > 0]
    return [n for n in out if kind is None or n.startswith(kind + "_")]


def script(name: str) -> dict:
    if name not in _scripts:
        z = _load()
        p = f"s{z['names'].tolist().index(name)}_"
        _scripts[name] = unpack({k[len(p):]: v for k, v in z.items() if k.startswith(p)})
    return _scripts[name]


def batches(s: dict):
    """-> (lo, hi, kind) per batch."""
    bo = s["batch_off"].tolist()
    return [(lo, hi, int(s["kind"][lo])) for lo, hi in zip(bo[:-1], bo[1:])]


def run_reference(s: dict) -> dict:
    """The script's inputs through the reference (needs oracle/_ref): -> the recorded columns, typed."""
    from tests.oracle_lib import RefTcpState

    r = RefTcpState(KEY, s["info"], s["key"], int(s["ip_id0"]))
    try:
        cap = int(s["frame_cap"])
        o = r.run(s["kind"], s["conn"], s["a"], s["b"], s["arena"], s["pay_off"], s["conv"], s["id8"].tobytes(),
                  frame_cap=cap)
        out = {"state0": r.state0.copy(), "head_size": np.int32(r.head_size())}
        final, ip = r.state()  # the conns' final state is what their last events recorded
        n = len(s["kind"])
        assert np.array_equal(final[:, 0], state_after(o, n, "conn_seq", r.state0[:, 0], s["conn"]))
        assert np.array_equal(final[:, 1], state_after(o, n, "conn_ack", r.state0[:, 1], s["conn"]))
        assert ip == (int(o["ip_id_next"][-1]) if n else int(s["ip_id0"]))
    finally:
        r.close()
    for k, dt in RECORDED.items():
        out[k] = o[k].astype(dt)
        assert np.array_equal(out[k].astype(np.int64), o[k]), k
    if cap:
        out["frames"] = o["frames"]
    return out


def init_rows(s: dict):
    """The table's row initialisation as INTEGRATION.md gives it: seq = info.ack + 1, ack = info.ack + 2.
    FakeTcp::Init hands TcpUtil::SetISN and SetAckISN the conn's OWN mInfo: SetISN writes seq = info.ack + 1,
    and SetAckISN's `info.seq + 1` then reads that seq, not the handshake packet's (FakeTcp.cpp:27-28,
    TcpUtil.cpp:15,28).  -> (seq [K], ack [K]) uint32."""
    info = s["info"].astype(np.uint32)
    return info[:, 5] + np.uint32(1), info[:, 5] + np.uint32(2)


def status_of(s: dict, lo: int, hi: int) -> np.ndarray:
    """A send batch's rsk_tcp_send_seq_batch status column from the recorded returns, as include/rsk_codec.h
    documents it: the frame length 31 + nread when the reference framed and sent the packet (its return),
    RSK_SEND_OVERSIZE for the frame RConn::Output rejected (return < 0)."""
    ret, nread = s["ret"][lo:hi], s["a"][lo:hi].astype(np.int64)
    assert bool(((ret >= 0) == (nread <= MAX_PAYLOAD)).all()) and bool((ret[ret >= 0] == HEAD + nread[ret >= 0]).all())
    return np.where(ret >= 0, ret, A.SEND_OVERSIZE).astype(np.int32)


def state_after(s: dict, hi: int, col: str, start: np.ndarray, conn=None) -> np.ndarray:
    """Each conn's recorded mInfo.seq (col "conn_seq") or mInfo.ack ("conn_ack") after event hi - 1."""
    st = start.copy()
    conn = (s["conn"] if conn is None else conn)[:hi]
    # the last event of a conn holds its state: walk backwards over first occurrences
    rev = conn[::-1]
    u, first = np.unique(rev, return_index=True)
    st[u] = s[col][:hi][::-1][first]
    return st


# ---- the packet-by-packet model and its mutants -------------------------------------------------------------
MUTANTS = ("wire_len", "reject_seq", "reject_ipid", "ipid_per_conn", "serial_compare", "ack_when_refused",
           "isn_seq_no_plus1", "isn_ack_no_plus1", "isn_ack_from_info_seq")
MODEL_COLS = ("ret", "n_tcp", "t_seq", "t_ack", "i_id", "conn_seq", "conn_ack", "ip_id_next")


def model(s: dict, mutant: str | None = None) -> dict:
    """FakeTcp::Output / RawTcp::Output / FakeTcp::OnRecv walked in Python; `mutant` breaks one rule."""
    assert mutant is None or mutant in MUTANTS
    M32 = 0xFFFFFFFF
    info = s["info"].tolist()
    seq = [(r[5] + (0 if mutant == "isn_seq_no_plus1" else 1)) & M32 for r in info]
    ack = [(r[5] + 1 + (0 if mutant == "isn_ack_no_plus1" else 1)) & M32 for r in info]
    if mutant == "isn_ack_from_info_seq":  # SetAckISN read as if it were handed the handshake packet's TcpInfo
        ack = [(r[4] + 1) & M32 for r in info]
    ip0 = int(s["ip_id0"])
    ipid = [ip0] * (len(info) if mutant == "ipid_per_conn" else 1)
    n = len(s["kind"])
    out = {k: np.zeros(n, np.int64) for k in MODEL_COLS}
    for i, (kind, c, a, b) in enumerate(zip(s["kind"].tolist(), s["conn"].tolist(), s["a"].tolist(), s["b"].tolist())):
        j = c if mutant == "ipid_per_conn" else 0
        if kind == SEND:
            if a <= MAX_PAYLOAD:
                out["ret"][i], out["n_tcp"][i] = HEAD + a, 1
                out["t_seq"][i], out["t_ack"][i], out["i_id"][i] = seq[c], ack[c], ipid[j]
                ipid[j] = (ipid[j] + 1) & 0xFFFF
                seq[c] = (seq[c] + HEAD + a + (40 if mutant == "wire_len" else 0)) & M32
            else:
                out["ret"][i] = -1
                if mutant == "reject_seq":
                    seq[c] = (seq[c] + HEAD + a) & M32
                if mutant == "reject_ipid":
                    ipid[j] = (ipid[j] + 1) & 0xFFFF
        else:
            out["ret"][i] = b
            if b >= 0 or mutant == "ack_when_refused":
                if mutant == "serial_compare":
                    d = (a - ack[c]) & M32
                    newer = 0 < d < 0x80000000
                else:
                    newer = ack[c] < a
                if newer:
                    ack[c] = a
        out["conn_seq"][i], out["conn_ack"][i], out["ip_id_next"][i] = seq[c], ack[c], ipid[j]
    return out


def model_differences(s: dict, m: dict) -> list[str]:
    """The model columns that differ from the script's recorded ones."""
    return [k for k in MODEL_COLS if not np.array_equal(m[k], s[k].astype(np.int64))]


# ---- IPv4 / TCP headers, unpacked plainly -------------------------------------------------------------------
def unpack_headers(pkts: np.ndarray) -> dict:
    """pkts [n, >= 40] uint8, each row an IPv4 packet: -> every header field as an int64 column (RFC 791 /
    793 layout; src / dst as the stored little-endian words TcpInfo holds)."""
    p = pkts.astype(np.int64)
    be16 = lambda o: (p[:, o] << 8) | p[:, o + 1]  # noqa: E731
    be32 = lambda o: (p[:, o] << 24) | (p[:, o + 1] << 16) | (p[:, o + 2] << 8) | p[:, o + 3]  # noqa: E731
    le32 = lambda o: p[:, o] | (p[:, o + 1] << 8) | (p[:, o + 2] << 16) | (p[:, o + 3] << 24)  # noqa: E731
    return {"version": p[:, 0] >> 4, "ihl": p[:, 0] & 15, "tos": p[:, 1], "tot_len": be16(2), "id": be16(4),
            "frag": be16(6), "ttl": p[:, 8], "proto": p[:, 9], "ip_sum": be16(10), "src": le32(12), "dst": le32(16),
            "sp": be16(20), "dp": be16(22), "seq": be32(24), "ack": be32(28), "doff": p[:, 32] >> 4,
            "x2": p[:, 32] & 15, "flags": p[:, 33], "win": be16(34), "tcp_sum": be16(36), "urg": be16(38)}


# header field -> the recorded libnet argument it must equal
FIELD_ARGS = (("tot_len", "i_len"), ("tos", "i_tos"), ("id", "i_id"), ("frag", "i_frag"), ("ttl", "i_ttl"),
              ("proto", "i_prot"), ("src", "i_src"), ("dst", "i_dst"), ("sp", "t_sp"), ("dp", "t_dp"), ("seq", "t_seq"),
              ("ack", "t_ack"), ("flags", "t_control"), ("win", "t_win"), ("urg", "t_urg"))


def fold(words_be: np.ndarray) -> np.ndarray:
    """One's-complement sum of each row's big-endian 16-bit words [n, k] (int64), folded to 16 bits."""
    t = words_be.sum(axis=1)
    for _ in range(3):
        t = (t & 0xFFFF) + (t >> 16)
    return t


def check_packets(s: dict, idx: np.ndarray, pkts: np.ndarray, lens: np.ndarray) -> None:
    """Packets pkts [m, width] (IPv4 header first, lens [m] bytes each) of the script's framed sends idx [m]
    against the recorded libnet arguments: every header field, the bytes behind the headers, and both
    checksums folding to 0xffff."""
    assert len(idx) == len(pkts) == len(lens) and len(idx) > 0
    h = unpack_headers(pkts)
    assert bool((h["version"] == 4).all()) and bool((h["ihl"] == 5).all())
    assert bool((h["doff"] == 5).all()) and bool((h["x2"] == 0).all())
    for field, arg in FIELD_ARGS:
        assert np.array_equal(h[field], s[arg][idx].astype(np.int64)), (field, arg)
    plen = s["t_payload_s"][idx].astype(np.int64)
    assert np.array_equal(lens, 40 + plen) and np.array_equal(s["t_len"][idx].astype(np.int64), 20 + plen)
    body = pkts[:, 40:]
    k = min(int(s["frame_cap"]), body.shape[1])
    assert int(plen.max()) <= k
    inside = np.arange(k)[None, :] < plen[:, None]
    assert np.array_equal(np.where(inside, body[:, :k], 0), np.where(inside, s["frames"][idx][:, :k], 0)), \
        "bytes behind the TCP header"
    # checksums: the IPv4 header alone; TCP over the pseudo-header, header and payload (odd lengths zero-padded)
    p = pkts.astype(np.int64)
    assert bool((fold((p[:, 0:20:2] << 8) | p[:, 1:20:2]) == 0xFFFF).all()), "IPv4 checksum"
    w = pkts.shape[1] - 20
    seg = np.where(np.arange(w)[None, :] < (20 + plen)[:, None], p[:, 20:], 0)
    if w % 2:
        seg = np.concatenate([seg, np.zeros((len(seg), 1), np.int64)], axis=1)
    words = (seg[:, 0::2] << 8) | seg[:, 1::2]
    pseudo = np.stack([(p[:, 12] << 8) | p[:, 13], (p[:, 14] << 8) | p[:, 15], (p[:, 16] << 8) | p[:, 17],
                       (p[:, 18] << 8) | p[:, 19], np.full(len(p), 6, np.int64), 20 + plen], axis=1)
    assert bool((fold(np.concatenate([pseudo, words], axis=1)) == 0xFFFF).all()), "TCP checksum"
