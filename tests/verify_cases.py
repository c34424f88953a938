"""Batches of captured packets for the checksum-verification tests (tests/test_verify_host.py on the
CPU twin, tests/test_gpu_verify.py on the kernel): each builder returns a Case whose expected outputs
come from tests/csum_ref.verify_ref.  The shapes are the smallest that can break a kernel that walks a
packet in aligned 16-B chunks with a fixed group of lanes."""
from __future__ import annotations

import functools
import struct
from dataclasses import dataclass

import numpy as np

from tests import csum_ref as R

DATALINKS = [R.DLT_EN10MB, R.DLT_NULL, R.DLT_RAW]
# segment lengths: every value across the first steps of any group width, then the 512 / 1024-B step
# borders, the MTU-sized segments and the longest ones a 1500-B packet holds
SEG_LENS = list(range(20, 301)) + [511, 512, 513, 1023, 1024, 1025, 1459, 1460, 1461, 1479, 1480]


@dataclass
class Case:
    arena: np.ndarray    # uint8
    cap_off: np.ndarray  # uint64
    cap_len: np.ndarray  # uint32
    datalink: int
    status: np.ndarray | None = None  # int8

    @property
    def n(self) -> int:
        return len(self.cap_len)

    def expected(self):
        return R.verify_ref(self.arena, self.cap_off, self.cap_len, self.datalink, self.status)


def pack(records, caps=None, base_pad=0, gap=0, fill=0, tail=0):
    """records `gap` bytes apart from base_pad on; every byte outside them is `fill`; the arena ends
    `tail` bytes after the last record.  caps: the cap_len of each record (default: its length)."""
    lens = np.array([len(r) for r in records], np.int64)
    offs = base_pad + np.concatenate([[0], np.cumsum(lens + gap)[:-1]]) if len(records) else np.zeros(0, np.int64)
    end = int(offs[-1] + lens[-1]) if len(records) else base_pad
    arena = np.full(end + tail, fill, np.uint8)
    for o, r in zip(offs, records):
        arena[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    caps = lens if caps is None else np.asarray(caps)
    return arena, offs.astype(np.uint64), caps.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def pool(datalink: int):
    """One correct packet per SEG_LENS entry (built once per datalink)."""
    rng = np.random.default_rng(100 + datalink)
    return [R.tcp_packet(rng, datalink, T) for T in SEG_LENS]


def flip_covered(arena, cap_off, cap_len, datalink, which, rng):
    """One flipped bit at a random byte of IP header + segment (up to cap_len) of the packets `which`."""
    L = R.LINK[datalink]
    for i in which:
        o, c = int(cap_off[i]), int(cap_len[i])
        arena[o + L + int(rng.integers(0, c - L))] ^= 1 << int(rng.integers(0, 8))


def alignment_case(datalink: int, base_pad: int) -> Case:
    """1. every segment length, back to back from base_pad on (every start residue mod 16), the arena
    ending at the last packet's last byte; every other packet with one flipped bit."""
    pk = pool(datalink)
    rng = np.random.default_rng(1000 * datalink + base_pad)
    order = rng.permutation(len(pk))
    arena, off, cl = pack([pk[j] for j in order], base_pad=base_pad)
    flip_covered(arena, off, cl, datalink, range(base_pad % 2, len(pk), 2), rng)
    return Case(arena, off, cl, datalink)


def every_byte_case():
    """2. one 100-B-payload Ethernet packet, and one copy per byte of its IP header + segment with a
    bit of that byte flipped -> (case, the byte flipped in packet 1 + j)."""
    rng = np.random.default_rng(2)
    p = R.tcp_packet(rng, R.DLT_EN10MB, 120)
    recs, where = [p], []
    for k in range(14, len(p)):
        b = bytearray(p)
        b[k] ^= 0x10
        recs.append(bytes(b))
        where.append(k)
    return Case(*pack(recs, base_pad=3), R.DLT_EN10MB), where


def neighbours_case(fill: int) -> Case:
    """3. correct packets with `fill` bytes around them, and a 46-B-payload frame whose cap_len
    includes 6 nonzero Ethernet trailer bytes."""
    rng = np.random.default_rng(3)
    recs = [R.tcp_packet(rng, R.DLT_EN10MB, T) for T in (20, 21, 35, 66, 100, 127, 128, 129, 300, 1460)]
    recs.append(R.tcp_packet(rng, R.DLT_EN10MB, 66) + bytes([0xDE, 0xAD, 0xBE, 0xEF, 0x01, 0xFF]))
    return Case(*pack(recs, base_pad=5, gap=7, fill=fill, tail=40), R.DLT_EN10MB)


def carries_case(datalink: int) -> Case:
    """4. 1480 / 1479 payload bytes of 0xFF, and a packet whose correct TCP checksum field is 0x0000,
    stored as 0x0000 and as 0xFFFF."""
    rng = np.random.default_rng(4)
    L = R.LINK[datalink]
    recs = [R.tcp_packet(rng, datalink, 20 + k, payload=b"\xff" * k) for k in (1480, 1479)]
    p = bytearray(R.tcp_packet(rng, datalink, 60))
    t = L + 20
    p[t + 16:t + 18] = b"\0\0"
    p[t + 20:t + 22] = b"\0\0"  # the payload halfword that steers the sum to 0xFFFF
    s = R.halfword_sum(bytes(p[L + 12:L + 20]) + bytes(p[t:]), 6 + 60)
    p[t + 20:t + 22] = struct.pack("!H", 0xFFFF - s)
    zero = R.fill_checksums(bytes(p), datalink)
    assert zero[t + 16:t + 18] == b"\0\0"
    recs += [zero, R.fill_checksums(bytes(p), datalink, tcp_field=0xFFFF)]
    return Case(*pack(recs, base_pad=9), datalink)


def ladder_case(datalink: int) -> Case:
    """5. every rung of the rule: link mismatches, bad version / ihl, options, other protocols,
    fragments, a total length below the headers, and cap_len cut in each part of the packet."""
    rng = np.random.default_rng(5)
    L = R.LINK[datalink]
    mk = lambda T=80, **kw: R.tcp_packet(rng, datalink, T, **kw)  # noqa: E731
    recs, caps = [], []

    def add(p, cap=None):
        recs.append(bytes(p))
        caps.append(len(p) if cap is None else cap)

    def patched(fn, **kw):
        b = bytearray(mk(**kw))
        fn(b)
        return R.fill_checksums(bytes(b), datalink)

    add(mk())
    if datalink == R.DLT_EN10MB:
        add(mk(ethertype=0x86DD))
        add(mk(ethertype=0x0806))
    if datalink == R.DLT_NULL:
        add(mk(null_family=24))
        add(mk(null_family=0x0200))
    for v in (0x65, 0x43, 0x40):  # version 6; ihl 3; ihl 0
        b = bytearray(mk())
        b[L] = v
        add(b)
    add(mk(T=60 + 33, ihl_words=15))
    add(mk(T=60 + 33, thl_words=15))
    add(mk(T=64, ihl_words=15, thl_words=15))
    add(mk(proto=17))
    add(patched(lambda b: b.__setitem__(slice(L + 6, L + 8), b"\x20\x00")))  # MF
    add(patched(lambda b: b.__setitem__(slice(L + 6, L + 8), b"\x00\x01")))  # fragment offset 1
    add(patched(lambda b: b.__setitem__(slice(L + 6, L + 8), b"\xc0\x00")))  # reserved + DF: still checked
    add(mk(ip_len=39))   # tot < H + 20
    add(mk(ip_len=20))
    add(mk(T=40, ihl_words=6, ip_len=43))
    add(mk(ip_len=20 + 80 + 1))  # tot one past the captured bytes
    p = mk(T=200)
    for cap in (0, 1, L - 1, L, L + 1, L + 19, L + 20, L + 39, L + 40, L + 41, len(p) - 1, len(p)):
        if cap >= 0:
            add(p, cap)
    q = mk(T=60, ihl_words=7)
    for cap in (L + 20, L + 27, L + 28, len(q) - 1):
        add(q, cap)
    return Case(*pack(recs, caps, base_pad=11), datalink)


def gated_case(datalink: int):
    """6. a status column: the packets that are not VALID get 0 and are not read -- their cap_off
    points far outside the arena."""
    c = alignment_case(datalink, 6)
    rng = np.random.default_rng(6)
    st = rng.choice(np.array([1, 1, 0, -1], np.int8), c.n)
    off = c.cap_off.copy()
    off[st != 1] = np.uint64(1) << np.uint64(46)
    return Case(c.arena, off, c.cap_len, datalink, st)


def sized_case(n: int, datalink: int = R.DLT_EN10MB) -> Case:
    """7. n packets of mixed lengths drawn from the pool (short ones mostly), about half of them with
    one flipped bit."""
    pk = pool(datalink)
    rng = np.random.default_rng(7000 + n)
    pick = np.where(rng.random(n) < 0.97, rng.integers(0, 281, n), rng.integers(281, len(pk), n))
    lens = np.array([len(p) for p in pk], np.int64)[pick]
    arena = np.frombuffer(b"".join(pk[j] for j in pick), np.uint8).copy()
    off = np.concatenate([[0], np.cumsum(lens)[:-1]])
    L = R.LINK[datalink]
    hit = np.nonzero(rng.random(n) < 0.5)[0]
    pos = off[hit] + L + (rng.random(len(hit)) * (lens[hit] - L)).astype(np.int64)
    arena[pos] ^= (1 << rng.integers(0, 8, len(hit))).astype(np.uint8)
    return Case(arena, off.astype(np.uint64), lens.astype(np.uint32), datalink)
