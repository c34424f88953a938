"""Numpy reference of rsk_verify_wire_batch's per-packet rule (include/rsk_codec.h): the IPv4 header
checksum and the TCP checksum of captured packets (RFC 791, RFC 793, RFC 1071), and helpers that
fill correct checksums into tests/pkt.ipv4_tcp packets.

Two statements of the rule: `verify_one` walks one packet the way the rule is written, `verify_ref`
does a whole batch at once with prefix sums over the arena (the tests compare the two)."""
from __future__ import annotations

import struct

import numpy as np

IP_CHECKED, IP_OK, TCP_CHECKED, TCP_OK, TCP_TRUNC = 0x01, 0x02, 0x04, 0x08, 0x10
ALL_OK = IP_CHECKED | IP_OK | TCP_CHECKED | TCP_OK
DLT_NULL, DLT_EN10MB, DLT_RAW = 0, 1, 12
LINK = {DLT_EN10MB: 14, DLT_NULL: 4, DLT_RAW: 0}
VALID, DROP = 1, -1


def halfword_sum(b, init: int = 0) -> int:
    """Ones'-complement sum of b as big-endian halfwords (an odd last byte is the high byte) plus
    init, folded to 16 bits: 0 only when everything is zero, 0xFFFF for other multiples of 0xFFFF."""
    a = np.frombuffer(bytes(b), np.uint8).astype(np.int64)
    s = int(a[0::2].sum()) * 256 + int(a[1::2].sum()) + init
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def verify_one(pkt, c: int, datalink: int) -> int:
    """CSUM_* bits of one packet: its first c bytes are captured (pkt holds at least those)."""
    p, L = bytes(pkt), LINK[datalink]
    if datalink == DLT_EN10MB and not (c >= 14 and p[12:14] == b"\x08\x00"):
        return 0
    if datalink == DLT_NULL and not (c >= 4 and struct.unpack("<I", p[:4])[0] == 2):
        return 0
    if c < L + 20 or p[L] >> 4 != 4 or (p[L] & 15) < 5 or c < L + 4 * (p[L] & 15):
        return 0
    H = 4 * (p[L] & 15)
    f = IP_CHECKED | (IP_OK if halfword_sum(p[L:L + H]) == 0xFFFF else 0)
    tot, frag = struct.unpack("!H", p[L + 2:L + 4])[0], struct.unpack("!H", p[L + 6:L + 8])[0]
    if p[L + 9] != 6 or frag & 0x3FFF or tot < H + 20:
        return f
    if L + tot > c:
        return f | TCP_TRUNC
    T = tot - H
    s = halfword_sum(p[L + 12:L + 20] + p[L + H:L + tot], 6 + T)
    return f | TCP_CHECKED | (TCP_OK if s == 0xFFFF else 0)


def is_bad(csum):
    csum = np.asarray(csum)
    return (((csum & IP_CHECKED) != 0) & ((csum & IP_OK) == 0)) | (((csum & TCP_CHECKED) != 0) & ((csum & TCP_OK) == 0))


def _fold(s):
    """s (int64 >= 0) folded to 16 bits, vectorised: 0 stays 0, other multiples of 0xFFFF give 0xFFFF."""
    return np.where(s == 0, 0, (s - 1) % 0xFFFF + 1)


def verify_ref(arena, cap_off, cap_len, datalink: int, status=None):
    """The rule over a batch -> (csum uint8 [n], status_out int8 [n] or None, n_bad).  Packets that a
    given `status` gates out are never indexed (their cap_off may lie outside the arena)."""
    arena = np.asarray(arena, np.uint8)
    off, c = np.asarray(cap_off).astype(np.int64), np.asarray(cap_len).astype(np.int64)
    n, L = len(off), LINK[datalink]
    ex = np.ones(n, bool) if status is None else np.asarray(status) == VALID
    off = np.where(ex, off, 0)
    c = np.where(ex, c, 0)
    a64 = arena.astype(np.int64)
    a64z = np.concatenate([a64, [0]])
    idx = np.arange(len(arena))
    # prefix sums of the bytes at even / odd arena positions
    pe = np.concatenate([[0], np.cumsum(np.where(idx % 2 == 0, a64, 0))])
    po = np.concatenate([[0], np.cumsum(np.where(idx % 2 == 1, a64, 0))])

    def at(k):  # byte k of every packet (0 where it lies past the arena; the c checks gate its use)
        return a64z[np.minimum(off + k, len(arena))]

    def rsum(lo, hi):  # big-endian halfword sum of arena[lo:hi) per packet, unfolded
        lo, hi = np.clip(lo, 0, len(arena)), np.clip(hi, 0, len(arena))
        hi = np.maximum(hi, lo)
        e, o = pe[hi] - pe[lo], po[hi] - po[lo]
        return np.where(lo % 2 == 0, 256 * e + o, 256 * o + e)

    ok = ex.copy()
    if datalink == DLT_EN10MB:
        ok &= (c >= 14) & (at(12) == 8) & (at(13) == 0)
    elif datalink == DLT_NULL:
        ok &= (c >= 4) & (at(0) == 2) & (at(1) == 0) & (at(2) == 0) & (at(3) == 0)
    ihl = at(L) & 15
    H = 4 * ihl
    ok &= (c >= L + 20) & ((at(L) >> 4) == 4) & (ihl >= 5) & (c >= L + H)
    ip_ok = ok & (_fold(rsum(off + L, off + L + H)) == 0xFFFF)
    tot, frag = at(L + 2) * 256 + at(L + 3), at(L + 6) * 256 + at(L + 7)
    tcp_try = ok & (at(L + 9) == 6) & ((frag & 0x3FFF) == 0) & (tot >= H + 20)
    trunc = tcp_try & (L + tot > c)
    chk = tcp_try & ~trunc
    T = tot - H
    s = rsum(off + L + 12, off + L + 20) + rsum(off + L + H, off + L + tot) + 6 + T
    tcp_ok = chk & (_fold(s) == 0xFFFF)
    csum = (ok * IP_CHECKED + ip_ok * IP_OK + chk * TCP_CHECKED + tcp_ok * TCP_OK + trunc * TCP_TRUNC).astype(np.uint8)
    bad = is_bad(csum)
    sout = None if status is None else np.where(bad, DROP, np.asarray(status)).astype(np.int8)
    return csum, sout, int(bad.sum())


def fill_checksums(pkt: bytes, datalink: int, tcp_field: int | None = None) -> bytes:
    """pkt (a tests/pkt.ipv4_tcp packet of any ihl_words / thl_words, link header included) with its
    IPv4 header checksum and TCP checksum filled in; tcp_field overrides the stored TCP checksum."""
    b, L = bytearray(pkt), LINK[datalink]
    H = 4 * (b[L] & 15)
    tot = struct.unpack("!H", b[L + 2:L + 4])[0]
    b[L + 10:L + 12] = b"\0\0"
    b[L + 10:L + 12] = struct.pack("!H", ~halfword_sum(b[L:L + H]) & 0xFFFF)
    t = L + H
    b[t + 16:t + 18] = b"\0\0"
    ck = ~halfword_sum(bytes(b[L + 12:L + 20]) + bytes(b[t:L + tot]), 6 + tot - H) & 0xFFFF
    b[t + 16:t + 18] = struct.pack("!H", ck if tcp_field is None else tcp_field)
    return bytes(b)


def tcp_packet(rng, datalink: int, seg_len: int, ihl_words: int = 5, thl_words: int = 5, payload: bytes | None = None,
               **kw) -> bytes:
    """A packet with a TCP segment of seg_len bytes (header + options + payload), random addresses,
    ports and payload, and correct checksums."""
    from tests.pkt import ipv4_tcp

    if payload is None:
        payload = rng.integers(0, 256, seg_len - 4 * thl_words, dtype=np.uint8).tobytes()
    ip = lambda: ".".join(str(int(x)) for x in rng.integers(0, 256, 4))  # noqa: E731
    raw = ipv4_tcp(ip(), int(rng.integers(0, 65536)), ip(), int(rng.integers(0, 65536)), int(rng.integers(0, 2**32)),
                   int(rng.integers(0, 2**32)), int(rng.integers(0, 256)), payload, ihl_words=ihl_words,
                   thl_words=thl_words, datalink=1 if datalink == DLT_EN10MB else 0, **kw)
    if datalink == DLT_RAW:
        raw = raw[4:]  # the DLT_NULL form without its family word
    return fill_checksums(raw, datalink)


def pack_exact(pkts, base_pad: int = 0, fill: int = 0, tail: int = 0):
    """Packets back to back from base_pad on -> (arena, cap_off, cap_len); the arena ends `tail` bytes
    after the last packet, and every byte outside the packets is `fill`."""
    lens = np.array([len(p) for p in pkts], np.int64)
    offs = base_pad + np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(pkts) else np.zeros(0, np.int64)
    arena = np.full(base_pad + int(lens.sum()) + tail, fill, np.uint8)
    if len(pkts):
        arena[base_pad:base_pad + int(lens.sum())] = np.frombuffer(b"".join(pkts), np.uint8)
    return arena, offs.astype(np.uint64), lens.astype(np.uint32)
