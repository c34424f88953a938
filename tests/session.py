"""TEST INFRASTRUCTURE: a server session of many batches through the chain INTEGRATION.md documents ("A server's
receive batch and its tick, in order"), compared after every event with tests/session_ref.Walk, which handles the same
packets one at a time.

  script(seed, shape)   the events of one session: ACCEPT (tuples), CAPTURE (packets), TICK (now_ms, timers), SEND
                        (conv rows, draws, payloads).  The generator asks a Walk of its own what exists, so that the
                        traffic never enters a documented deviation; the Walk's guards make that a checked property.
  ServerChain(side)     the documented procedure and nothing else, on the host twins ("host": device "cpu", the
                        stages without a twin -- parse, recv_ack, demux, send_seq, the wire build -- on the C oracle),
                        on a device call by call ("device"), or on a device with the DATA chain and the tick's closes
                        replayed from two captured graphs ("graph").  MUTANTS names the one-step breakages of the
                        chain that tests/test_session_host.py shows the scripts see.
  run(script, chain)    drives both, compares after EVERY event, returns the walk's `seen` counts.
  run_split(...)        split invariance: a capture whole against the same capture cut at safe_cuts' points; no model.
No packet and no row of any script is excluded from a comparison."""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import collide
from tests import session_ref as W

KEY = b"hello135"
ETH = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
SERVER_IP, SERVER_PORT = 0x0100000A, 443  # 10.0.0.1 as s_addr holds it
PERSIST_MS = 1000
PARSE_FLAGS = A.PARSE_HAS_ACK_POOL | A.PARSE_IS_SERVER
DEMUX_FIELDS = A.DEMUX_ID | A.DEMUX_DST | A.DEMUX_CONV | A.DEMUX_GROUP_BARRIER
HOME = collide.WIDE - 3

# shape -> table sizes, IdBufs, the capture sizes in order, and the floors: the least EACH count of Walk.seen must reach,
# so that a script cannot quietly stop exercising something.  The floors are about three quarters of the smaller of
# what the WALK ALONE counts for seeds 1 and 2 (run on the CPU, no library involved; that number stands in the
# comment behind each shape, in the order of COUNTS).  A floor of 0 is a count the shape cannot produce; why, is said.
COUNTS = ("conns_born", "conns_reset", "conns_timed_out", "rows_reused", "convs_born", "convs_reset", "convs_reborn",
          "offers_refused", "pool_expired", "ka_answers", "csum_drops")


def _floors(*v):
    return dict(zip(COUNTS, v))


SHAPES = {
    # conns and convs born in the first capture, then only DATA and keepalives.  Nothing is reset or refused (0, 0, 0, 0);
    # every handshake is consumed by the capture that brings it, so no pool entry is left to expire (0); the conns
    # that time out leave at the last ticks and nothing is born behind them, so no row is reused (0).
    "steady": dict(cap_conn=67, cap_conv=131, cap_pool=67, n_ids=3, sizes=(63, 2049, 1, 2047), churn=False,
                   floors=_floors(12, 0, 4, 0, 57, 0, 0, 0, 0, 8, 57)),
    #                             15  0  6  0  76  0  0  0  0  11  76
    # every capture creates and resets conns and convs, ticks time rows out and expire pool entries, rows are reused
    "churn": dict(cap_conn=67, cap_conv=131, cap_pool=67, n_ids=3, sizes=(63, 2047, 2049, 63), churn=True, split=True,
                  floors=_floors(44, 6, 3, 66, 66, 11, 7, 6, 11, 12, 82)),
    #                            59  9  4  88  88  15  10  8  15  16  110
    # one conv carries 90 % of a 4097-packet capture, with resets of it in the middle.  Three captures leave room for
    # three keepalive ticks only, and a conn times out at its fourth unanswered one (0).
    "skew": dict(cap_conn=67, cap_conv=131, cap_pool=67, n_ids=1, sizes=(63, 4097, 63), churn=True, skew=True,
                 floors=_floors(28, 2, 0, 40, 49, 6, 4, 3, 24, 9, 83)),
    #                           38  3  0  54  66  8  6  4  32  12  111
    # churn with every conn key, IdBuf, tuple and conv probing from one index entry, WIDE - 3: one run that wraps
    "clustered": dict(cap_conn=1025, cap_conv=2053, cap_pool=1025, n_ids=65, sizes=(2049, 2047, 63, 2049), churn=True,
                      clustered=True, floors=_floors(457, 52, 69, 500, 813, 75, 49, 21, 41, 13, 111)),
    #                                                610  70  92  667  1085  100  66  29  55  18  149
    # 4097, 2049, 63, 1, 4097 on one stream with no reserve in between: a smaller call on scratch a larger one filled.
    # Five captures leave room for three ticks only (the session has 16 events at the most): no conn times out (0).
    "shrinking": dict(cap_conn=1025, cap_conv=2053, cap_pool=1025, n_ids=3, sizes=(4097, 2049, 63, 1, 4097), churn=True,
                      split=True, floors=_floors(459, 60, 0, 511, 808, 159, 104, 21, 36, 13, 194)),
    #                                            612  81  0  682  1078  213  139  29  48  18  259
}


def id_bytes(word) -> bytes:
    return int(word).to_bytes(8, "little")


# ---- the scripts ---------------------------------------------------------------------------------------------------
class Gen:
    """Builds one session against a Walk of its own (self.w), so that every packet names things that exist -- or, on
    purpose, things that do not -- and never enters a deviation."""

    def __init__(self, seed, shape):
        p = SHAPES[shape]
        self.p, self.rng = p, np.random.default_rng([seed, sorted(SHAPES).index(shape)])
        self.w = W.Walk(p["cap_conn"], p["cap_conv"], p["cap_pool"], p["cap_pool"], PERSIST_MS)
        g = p["n_ids"]
        self.clustered = bool(p.get("clustered"))
        if self.clustered:
            self.ids = [id_bytes(x) for x in collide.ids_at(HOME, g)]
            k = 4 * p["cap_pool"]
            src, dst, sp, dp = collide.tuples_at(HOME, k)
            self.tuples = [t for t in zip(src.tolist(), sp.tolist(), dst.tolist(), dp.tolist()) if t[1] and t[3]]
            self.conv_lo = {}
            self.conv_pool = {}  # (IdBuf, peer address) -> the convs of that pair that probe from HOME, not yet used
        else:
            self.ids = [bytes(self.rng.integers(0, 256, 8, dtype=np.uint8)) for _ in range(g)]
        self.next_tuple, self.next_key = 0, 0
        self.cseq = {}       # tuple -> the client's next th_seq
        self.anchor = {}     # id8 -> the key of the conn that is never reset and always answers
        self.mute = set()    # (id8, key) of the conns whose client stops answering keepalive requests
        self.want_resp = []  # (id8, key, tuple) the requests of the last tick that will be answered
        self.late = []       # (id8, key, tuple) handshake and socket are pooled, the first DATA packet comes a capture later
        self.captures = 0
        self.events = []
        self.now = 1000

    # ---- names ----
    def new_tuple(self, gi):
        """(src, sp, dst, dp) in the orientation of a DATA packet's TcpInfo: src the server, dst the client."""
        j = self.next_tuple
        self.next_tuple += 1
        if self.clustered:
            return self.tuples[j]
        return (SERVER_IP, SERVER_PORT, 0x0A000000 + 0x10000 * (gi + 1) + 0x14, 1024 + j)

    def new_key(self, gi):
        j = self.next_key
        self.next_key += 1
        if self.clustered:  # the keys of one IdBuf probe from one home under that IdBuf
            return int(collide.keys_at(HOME, 1, int.from_bytes(self.ids[gi], "little"), salt=j + 1)[0])
        return int(self.rng.integers(1, 2**63)) | 1

    def new_conv(self, gi, dst):
        """A conv no conv of (IdBuf gi, peer address dst) has had.  clustered: one whose key in a server's conv table,
        (IdBuf, dst << 32 | conv), probes from HOME -- collide.convs_at's search, over the table's full key (convs_at
        itself searches the conv-only key of a client's table) -- so that the conv index is one run that wraps too."""
        if not self.clustered:
            return int(self.rng.integers(1, 2**32))
        pool = self.conv_pool.get((gi, dst))
        if not pool:
            slots = collide.conn_slots(self.p["cap_conv"])
            lo = self.conv_lo.get((gi, dst), 1)
            cand = np.arange(lo, lo + (1 << 16), dtype=np.uint64)
            homes = collide.homes_np(cand | (np.uint64(dst) << np.uint64(32)), np.full(len(cand), int.from_bytes(self.ids[gi], "little"), np.uint64), slots)
            pool = self.conv_pool[(gi, dst)] = cand[homes == HOME % slots].tolist()[::-1]
            self.conv_lo[(gi, dst)] = lo + (1 << 16)
            assert pool, "no conv of this pair probes from HOME in 65536 candidates"
        return int(pool.pop())

    # ---- packets ----
    def frame(self, tup, cmd, id8, conv, key, payload, seq=None):
        src, sp, dst, dp = tup
        if seq is None:
            seq = self.cseq.setdefault(tup, int(self.rng.integers(1, 2**31)))
            self.cseq[tup] = (seq + W.HEAD + len(payload)) & W.M32
        return W.Packet(dst, src, dp, sp, seq, 1, 0x18, cmd, id8, conv, key, payload)

    def data(self, tup, id8, conv, key):
        return self.frame(tup, W.DATA, id8, conv, key, bytes(self.rng.integers(0, 256, int(self.rng.integers(1, 24)), dtype=np.uint8)))

    def synack(self, tup):
        src, sp, dst, dp = tup  # the server's own SYN|ACK, as its capture sees it
        return W.Packet(src, dst, sp, dp, int(self.rng.integers(0, 2**32)), int(self.rng.integers(0, 2**32)), 0x12)

    # ---- events ----
    def accept(self, tuples):
        self.events.append(("ACCEPT", list(tuples), self.now))
        self.w.accept(tuples, self.now)

    def capture(self, n, first):
        p, rng, w = self.p, self.rng, self.w
        chains, singles, accepted = [], [], []  # a chain: packets whose order must hold
        live = [(g, k, c) for g, grp in w.conns.items() for k, c in grp.items()]
        old_alive = [(g, k, c) for g, k, c in live if c.alive]
        gi_of = {g: i for i, g in enumerate(self.ids)}
        churn = bool(p["churn"]) and not first and n >= 63
        room = lambda: n - sum(len(c) for c in chains) - len(singles)  # noqa: E731  the packets this capture can still take
        # conns born here: the handshake first, then the DATA packets that use it
        n_new = min(p["cap_conn"] // 3 if first else p["cap_conn"] // 8, max(1, n // 4), len(w.r_conn.free) - 2)
        if not (first or p["churn"]) or n < 63:
            n_new = 0
        budget = (len(w.r_conv.free) - 8) // 3  # the conv rows this capture may take: most stay for the later ones
        fresh = []
        for j in range(max(min(n_new, n // 4), 0)):
            gi = j % len(self.ids)
            g, k, t = self.ids[gi], self.new_key(gi), self.new_tuple(gi)
            accepted.append(t)
            fresh.append((g, k, t))
            self.anchor.setdefault(g, k)
            if (j % 3 == 2) and self.anchor[g] != k:
                self.mute.add((g, k))
            chains.append([self.synack(t), self.data(t, g, self.new_conv(gi, t[2]), k)])
            budget -= 1
        used = set()  # conns a control packet of this capture names: named once
        self.captures += 1
        keep = []
        for g, k, t in self.late:  # the conns whose handshake an earlier capture harvested: more conns than handshakes here
            if room() < 40:  # no room here: its first packet comes in a later capture
                keep.append((g, k, t))
                continue
            chains.append([self.data(t, g, self.new_conv(gi_of[g], t[2]), k)])
            budget -= 1
        self.late = keep
        if churn:
            for j in range(min(20 if self.captures == 2 else 3, len(w.r_conn.free) - n_new - 6, max(0, room() - 30))):
                gi = j % len(self.ids)
                g, k, t = self.ids[gi], self.new_key(gi), self.new_tuple(gi)
                accepted.append(t)
                self.late.append((g, k, t))
                singles.append(self.synack(t))
            # refused: a handshake without a socket, and a socket without a handshake
            t1, t2 = self.new_tuple(0), self.new_tuple(0)
            accepted.append(t2)
            g = self.ids[0]
            chains.append([self.synack(t1), self.data(t1, g, 7, self.new_key(0))])
            singles.append(self.data(t2, g, 7, self.new_key(0)))
            # a second handshake of a pooled tuple only moves the expiry; a zero port is dropped
            t3 = self.new_tuple(0)
            chains.append([self.synack(t3), self.synack(t3)])
            singles.append(W.Packet(SERVER_IP, 0x0A0A0A0A, 0, 999, 5, 6, 0x12))
            # conns reset by their peer
            stay = {}  # a group keeps a conn that has sent before, answers its keepalives and is not reset here
            for g, k, c in old_alive:
                if (g, k) not in self.mute and not c.new:
                    stay.setdefault(g, []).append(c.row)
            cand = [(g, k, c) for g, k, c in old_alive if (g, k) not in self.mute and len(stay.get(g, [])) >= 2 and c.row != min(stay[g])]
            for g, k, c in cand[: max(1, len(cand) // 6)]:
                if len(stay[g]) < 2 or room() < 24:
                    continue
                stay[g].remove(c.row) if c.row in stay[g] else None
                used.add((g, k))
                singles.append(self.frame(c.tup, W.NETCONN_RST, g, 0, k, k.to_bytes(8, "little")))
        if accepted:
            self.accept(accepted)
        if not first and n >= 63:
            # keepalive requests of the peer: for a conn that lives, and for one the server does not know
            cand = sorted(((g, k, c) for g, k, c in old_alive if (g, k) not in used), key=lambda x: (-x[2].est, x[2].row))
            for g, k, c in cand[:3 if room() >= 16 else 0]:  # the newest first: a conn born in the capture before answers here
                used.add((g, k))
                singles.append(self.frame(c.tup, W.KA_REQ, g, 0, k, k.to_bytes(8, "little")))
                ghost = (1 << 63) | self.new_key(gi_of[g])
                singles.append(self.frame(c.tup, W.KA_REQ, g, 0, k, ghost.to_bytes(8, "little")))
            # a FIN, a frame of an unknown command and a control frame with a short body
            if old_alive and room() >= 8:
                g, k, c = old_alive[0]
                singles.append(W.Packet(c.tup[2], c.tup[0], c.tup[3], c.tup[1], 5, 6, 0x11))
                singles.append(self.frame(c.tup, 9, g, 0, k, b"\1\2\3\4\5\6\7\10"))
                singles.append(self.frame(c.tup, W.KA_REQ, g, 0, k, b"\1\2\3"))
        # the answers to the last tick's requests
        for g, k, t in self.want_resp:
            c = w.conns.get(g, {}).get(k)
            if c is not None and (g, k) not in used and room() >= 5:
                used.add((g, k))
                singles.append(self.frame(t, W.KA_RESP, g, 0, k, k.to_bytes(8, "little")))
        self.want_resp = []  # a request that found no room is asked again by the next tick
        # the conns that carry this capture's DATA, by (IdBuf, peer address): a conv's key holds the peer's address
        carriers = [(g, k, c) for g, k, c in old_alive if (g, k) not in used]
        by_gd = {}
        for g, k, c in carriers:
            by_gd.setdefault((g, c.tup[2]), []).append((k, c))
        convs = [(v.id8, v.dst, v.conv) for r, v in sorted(w.conv_at.items()) if (v.id8, v.dst) in by_gd]
        skew = convs[0] if p.get("skew") and convs and n > 1000 else None
        quiet = set()
        if churn:  # convs reset by their peer, most of them with DATA behind the reset: the reborn conv
            for j, (g, dst, conv) in enumerate(convs[1: 1 + max(2, len(convs) // 5)] + ([skew] if skew else [])):
                if room() < 4:
                    break
                k, c = by_gd[(g, dst)][j % len(by_gd[(g, dst)])]
                ch = [self.data(c.tup, g, conv, k), self.frame(c.tup, W.CONV_RST, g, 0, k, conv.to_bytes(4, "little"))]
                if j % 3 != 1 or (g, dst, conv) == skew:
                    ch += [self.data(c.tup, g, conv, k), self.data(c.tup, g, conv, k)]
                else:  # a second reset with no DATA between: it finds nothing, so no other packet of the capture names the conv
                    quiet.add((g, dst, conv))
                    ch += [self.frame(c.tup, W.CONV_RST, g, 0, k, conv.to_bytes(4, "little"))]
                chains.append(ch)
                budget -= 1
        # the rest: DATA on the conns that stay, for convs old and new
        assert room() >= 0, ("the capture's packets do not fit", n, room())
        convs = [x for x in convs if x not in quiet]
        for j in range(room()):
            if skew is not None and j % 10 != 0:
                g, dst, conv = skew
                k, c = by_gd[(g, dst)][j % len(by_gd[(g, dst)])]
                singles.append(self.data(c.tup, g, conv, k))
            elif convs and rng.random() < 0.8:
                g, dst, conv = convs[int(rng.integers(0, len(convs)))]
                k, c = by_gd[(g, dst)][int(rng.integers(0, len(by_gd[(g, dst)])))]
                singles.append(self.data(c.tup, g, conv, k))
            elif fresh:  # a later packet of a conn born here, on a conv born here: behind its handshake and first packet
                ci = int(rng.integers(0, len(fresh)))
                g, k, t = fresh[ci]
                old = rng.random() < 0.7 or budget <= 0
                budget -= 0 if old else 1
                chains[ci].append(self.data(t, g, chains[ci][1].conv if old else self.new_conv(gi_of[g], t[2]), k))
            elif carriers and budget > 0:
                g, k, c = carriers[int(rng.integers(0, len(carriers)))]
                singles.append(self.data(c.tup, g, self.new_conv(gi_of[g], c.tup[2]), k))
                budget -= 1
            else:
                singles.append(W.Packet(1, 2, 3, 4, 5, 6, 0x10))  # a bare ACK: the parse drops it
        # interleave: every chain keeps its order
        keys = []
        for ch in [[x] for x in singles] + chains:
            ks = np.sort(rng.random(len(ch)))
            keys += [(float(ks[j]), x) for j, x in enumerate(ch)]
        keys.sort(key=lambda z: z[0])
        pk = [x for _, x in keys]
        assert len(pk) == n, (len(pk), n)  # nothing generated is cut off
        for i, x in enumerate(pk):  # every 37th packet arrives damaged: a payload byte, or the TCP checksum
            x.corrupt = bool(i % 37 == 36 and x.id8 and not x.flags & 0x07)
        draws = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        cuts = safe_cuts(w, pk, self.now, draws) if p.get("split") and n >= 63 else []
        self.events.append(("CAPTURE", pk, self.now, draws, cuts))
        w.capture(pk, self.now)
        w.send_queued(draws)

    def send(self, frac=1.0, clear_new=True):
        """DATA from the convs to their peers; with clear_new every alive conn of a group carries one."""
        w, rng = self.w, self.rng
        rows, draws = [], []
        groups = {g: sorted((c for c in grp.values() if c.alive), key=lambda c: c.row) for g, grp in w.conns.items()}
        per_group = {}
        for r in sorted(w.conv_at):
            v = w.conv_at[r]
            if not groups.get(v.id8):
                continue
            per_group.setdefault(v.id8, []).append(r)
            if (r % 3 != 2) or frac >= 1.0:
                rows.append(r)
                draws.append(int(rng.integers(0, 2**32)))
        if clear_new:
            for g, rs in per_group.items():
                for j in range(len(groups[g])):
                    rows.append(rs[j % len(rs)])
                    draws.append(j)
        if not rows:
            return
        pays = [bytes(rng.integers(0, 256, 1 + (j % 17), dtype=np.uint8)) for j in range(len(rows))]
        self.events.append(("SEND", np.array(rows, np.uint32), np.array(draws, np.uint32), pays))
        w.send(rows, draws, pays)

    def tick(self, dt, which):
        w = self.w
        self.now += dt
        res = w.tick(self.now, which)
        draws = []
        for cmd, body, id8, avoid, src in res["requests"]:
            cand = sorted((c for c in w.conns.get(id8, {}).values() if c.alive), key=lambda c: c.row)
            ok = [j for j, c in enumerate(cand) if not c.new]
            assert ok, "a request without a carrier that has sent before"
            draws.append(ok[len(draws) % len(ok)] + len(cand) * (len(draws) % 5))
            c = w.conns.get(id8, {}).get(body)
            if c is not None and c.alive and (id8, body) not in self.mute:
                self.want_resp.append((id8, body, c.tup))
        draws = np.array(draws + [0], np.uint32)
        self.events.append(("TICK", self.now, tuple(which), draws))
        w.send_queued(draws, tick=True)


def walk_parts(walk, pk, now, draws, cuts):
    """The capture through `walk` whole (cuts = []) or cut into consecutive batches, the answers of each batch sent
    behind it with the next draws: -> everything an observer can see afterwards."""
    cols, delivered, sends, k = {}, {}, [], 0
    for lo, hi in zip([0] + list(cuts), list(cuts) + [len(pk)]):
        r = walk.capture(pk[lo:hi], now)
        for name in ("parse_status", "status", "conn", "hit", "miss", "kind", "arg", "cconn", "conv_row"):
            cols.setdefault(name, []).extend(r[name])
        for row, b in r["delivered"].items():
            delivered[row] = delivered.get(row, b"") + b
        out = walk.send_queued(draws[k:])
        k += len(out)
        sends += out
    return cols, delivered, sends, walk.snapshot()


def safe_cuts(walk, pk, now, draws):
    """The cut points of a capture at which cutting it into consecutive batches changes nothing an observer can see:
    tried on copies of the walk, one cut at a time and then together.  A cut is unsafe where the batch interface
    itself makes the two runs differ (a row vacated in the first part is vacant for the second; an answer of the
    first part is picked before a reset of the second).  -> 1 to 4 cuts (2 to 5 batches), [] when none is safe."""
    import copy

    n = len(pk)
    whole = walk_parts(copy.deepcopy(walk), pk, now, draws, [])
    cand = sorted({c for c in (1, 2, 3, 5, 8, 13, 21, 34, 55, n // 4, n // 2, n - 55, n - 34, n - 21, n - 13, n - 8, n - 5, n - 3,
                               n - 2, n - 1) if 0 < c < n})
    safe = []
    for c in cand:
        try:
            if walk_parts(copy.deepcopy(walk), pk, now, draws, [c]) == whole:
                safe.append(c)
        except W.SessionDeviation:
            pass
    while safe:
        pick = sorted({safe[0], safe[len(safe) // 3], safe[2 * len(safe) // 3], safe[-1]})
        try:
            if walk_parts(copy.deepcopy(walk), pk, now, draws, pick) == whole:
                return pick
        except W.SessionDeviation:
            pass
        safe = safe[:-1]
    return []


_SCRIPTS = {}


def script(seed, shape):
    """-> {"shape", "seed", "params", "events", "ids"}; 12 to 16 events.  Built once per process: nothing changes it."""
    if (seed, shape) not in _SCRIPTS:
        _SCRIPTS[(seed, shape)] = _script(seed, shape)
    return _SCRIPTS[(seed, shape)]


def _script(seed, shape):
    g = Gen(seed, shape)
    sizes = g.p["sizes"]
    g.capture(sizes[0], True)              # ACCEPT, CAPTURE
    g.send()
    g.tick(16000, ("ka", "conv", "pool"))  # the first keepalive requests
    for j, n in enumerate(sizes[1:]):
        g.capture(n, False)                # (ACCEPT,) CAPTURE: the answers, the churn
        if j < 2:
            g.send(frac=0.66)
        if j < 2 or (j == 2 and len(sizes) == 4):
            g.tick(1500 if j else 500, ("ka", "conv", "pool") if j != 1 else ("ka", "pool"))
    while len(g.events) < 12:
        g.tick(1500, ("ka", "conv", "pool"))
    assert 12 <= len(g.events) <= 16, len(g.events)
    return {"shape": shape, "seed": seed, "params": g.p, "events": g.events, "ids": g.ids}


# ---- frames --------------------------------------------------------------------------------------------------------
def build_capture(oracle, packets):
    """The packets as an Ethernet capture: (arena uint8, offsets uint64, lengths uint32).  Frames by the oracle's
    encoder and its libnet-style wire build (both checksums right); a damaged packet has a payload byte flipped
    behind payload[0] -- the tag still verifies -- or, with a one-byte payload, its TCP checksum."""
    out, offs, lens, cur = [], [], [], 0
    for i, p in enumerate(packets):
        frame = b""
        if p.id8:
            st, frame = oracle.rconn_output(KEY, p.payload, p.cmd, p.id8, p.conv, p.key)
            assert st == W.HEAD + len(p.payload)
        b = bytearray(oracle.build_wire(frame, p.ip_src, p.ip_dst, p.sport, p.dport, p.th_seq, p.th_ack, p.flags, i & 0xFFFF, ETH))
        if p.corrupt:
            at = 54 + W.HEAD + 1 if len(p.payload) > 1 else 14 + 20 + 16
            b[at] ^= 0x40
        out.append(bytes(b))
        offs.append(cur)
        lens.append(len(b))
        cur += len(b) + (i % 3)  # packets start at any byte of the ring
    arena = np.zeros(cur + 64, np.uint8)
    for o, b in zip(offs, out):
        arena[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return arena, np.array(offs, np.uint64), np.array(lens, np.uint32)


# ---- the driver ----------------------------------------------------------------------------------------------------
MUTANTS = ("no_second_recv_ack", "close_without_pick", "hold_not_cleared", "new_never_cleared", "settle_with_add_n_new",
           "conv_resolve_with_old_hit", "conv_close_without_hold", "no_sock_flush")

_SIGNED = {np.dtype(np.uint8): np.uint8, np.dtype(np.int8): np.int8, np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32,
           np.dtype(np.uint64): np.int64, np.dtype(np.int32): np.int32, np.dtype(np.int64): np.int64, np.dtype(np.int16): np.int16}


def H(t, dt):
    """A tensor on the host as the unsigned C type it stores."""
    return t.detach().cpu().numpy().view(dt).copy()  # a copy: a "cpu" tensor's numpy view would follow later calls


class ServerChain:
    """The documented server procedure, one call after the other ("A server's receive batch and its
    tick, in order").  Every host step between calls is one the document names."""

    def __init__(self, side, params, oracle, codec=None, device="cpu", mutant=None, stream=None, fixed=0, arena_max=0):
        """side "host" (the twins), "device" (call by call) or "graph": the device with the DATA chain (offers ..
        the second conv create) and the tick's closes replayed from two graphs, each captured on `stream` behind one
        eager run.  fixed = n_max > 0 (any side; required for "graph"): every capture runs as n_max packets over
        buffers that never move, the packets behind the capture's own having wire length 0 -- the parse drops them."""
        assert side in ("host", "device", "graph") and (side == "host") == (codec is None)
        assert side != "graph" or (fixed > 0 and stream is not None)
        self.fixed, self.arena_max, self.kept, self._ns, self._seq, self.graphs, self.replays = fixed, arena_max, {}, None, 0, {}, 0
        assert mutant is None or mutant in MUTANTS
        self.side, self.cx, self.dev, self.orc, self.mutant, self.stream = side, codec, device, oracle, mutant, stream
        p = params
        self.tab = rc.ConnTable.alloc(p["cap_conn"], device, by_id=True)
        self.ctab = rc.ConvTable.alloc(p["cap_conv"], device, by_dst=True, by_id=True)
        self.ackp = rc.PoolTable.alloc(p["cap_pool"], device)
        self.sockp = rc.PoolTable.alloc(p["cap_pool"], device, vals=False)
        self.ka = torch.full((p["cap_conn"],), A.KA_NONE, dtype=torch.uint8, device=device)
        self.est = torch.zeros(p["cap_conn"], dtype=torch.int64, device=device)
        self.ip_id_next = torch.zeros(1, dtype=torch.int16, device=device)
        if codec is not None:
            torch.cuda.synchronize()
        with self.on():
            for t in (self.tab, self.ctab, self.ackp, self.sockp):
                t.rebuild(codec)
            self.tab.rebuild_pick(codec)
            self.sync()
        self.m_max = p["cap_pool"]
        self.bound, self.closed, self.sock_of = {}, [], {}  # conn row -> tuple; tuples closed; socket-pool row -> tuple

    # ---- plumbing ----
    def T(self, a, dt=None):
        a = np.ascontiguousarray(a, dt)
        return torch.from_numpy(a.view(_SIGNED[a.dtype])).to(self.dev)

    def keep(self, make):
        """make(), or with `fixed` inside a capture or a tick the object the same place of the sequence made before:
        the calls of a captured graph must find their buffers where they were."""
        if not self.fixed or self._ns is None:
            return make()
        key = (self._ns, self._seq)
        self._seq += 1
        if key not in self.kept:
            self.kept[key] = make()
        return self.kept[key]

    def e(self, n, dt=torch.int32, fill=None):
        t = self.keep(lambda: torch.empty(max(n, 1), dtype=dt, device=self.dev))
        t.view(torch.uint8).fill_(0xA5 if fill is None else fill)
        return t

    def table_tensors(self):
        ts = [self.ka, self.est]
        for t in (self.tab, self.ctab, self.ackp, self.sockp):
            ts += [v for v in vars(t).values() if isinstance(v, torch.Tensor)]
        return ts

    def graphed(self, name, body):
        """body() -- library calls on kept buffers only -- as it stands, or on the "graph" side: eagerly once, then
        captured (the tables put back as the eager run left them: a capture runs nothing), then replayed."""
        if self.side != "graph":
            return body()
        if name not in self.graphs:
            body()
            self.sync()
            saved = [t.clone() for t in self.table_tensors()]
            self.sync()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=self.stream):
                body()
            for t, v in zip(self.table_tensors(), saved):
                t.copy_(v)
            self.sync()
            self.graphs[name] = g
        else:
            self.graphs[name].replay()
            self.replays += 1

    def sync(self):
        if self.cx is not None:
            torch.cuda.current_stream().synchronize()

    def on(self):
        """The context in which every call and every tensor operation of this chain runs: its own stream."""
        return contextlib.nullcontext() if self.stream is None else torch.cuda.stream(self.stream)

    def call(self, name, *a, **kw):
        """Codec.<name> on the chain's stream, or the host twin of the same arguments."""
        if self.cx is None:
            host = {"pool_add_batch": "pool_add_host", "pool_offers": "pool_offers_host", "pool_settle_batch": "pool_settle_host",
                    "pool_flush": "pool_flush_host", "conn_create_batch": "conn_create_host", "control_batch": "control_host",
                    "conn_close_batch": "conn_close_host", "conv_resolve_batch": "conv_resolve_host",
                    "conv_create_batch": "conv_create_host", "conv_close_batch": "conv_close_host",
                    "conv_send_batch": "conv_send_host", "conv_flush": "conv_flush_host", "keepalive_flush": "keepalive_flush_host"}
            return getattr(rc, host[name])(*a, **kw)
        return getattr(self.cx, name)(*a, **kw)  # on torch's current stream: the chain's, inside self.on()

    def u32(self, t):
        return H(t, np.uint32)

    # ---- the stages without a host twin ----
    def parse_verify(self, arena, off, ln):
        """-> the capture on the chain's side, parsed and verified; with `fixed`, as fixed packets in kept buffers."""
        n = len(off)
        if self.fixed:
            assert n <= self.fixed and len(arena) <= self.arena_max, "a capture larger than the chain was made for"
            off, ln = (np.concatenate([a, np.zeros(self.fixed - n, a.dtype)]) for a in (off, ln))
            arena = np.concatenate([arena, np.zeros(self.arena_max - len(arena), np.uint8)])
        N = len(off)
        tcp, dec = self.keep(lambda: rc.TcpInfoBuffers.alloc(N, self.dev)), self.keep(lambda: rc.DecodeBuffers.alloc(N, self.dev))
        cap, coff, clen = (self.keep(lambda a=a: torch.empty_like(self.T(a))) for a in (arena, off, ln))
        cap.copy_(self.T(arena)), coff.copy_(self.T(off)), clen.copy_(self.T(ln))
        n_bad = self.e(1)
        if self.cx is None:
            o = self.orc.parse_decode_batch(KEY, arena, off, ln, ln, A.DLT_EN10MB, PARSE_FLAGS)
            for f in ("src", "dst", "sp", "dp", "seq", "ack", "flag", "parse_status", "cap_pay_off", "cap_pay_len"):
                getattr(tcp, f).copy_(self.T(o[f]))
            for f in ("hlen", "cmd", "id", "conv", "conn_key", "pay_off", "pay_len", "status"):
                getattr(dec, f).copy_(self.T(o[f]))
            _c, so, nb = rc.verify_wire_host(arena, off, ln, A.DLT_EN10MB, status=o["status"], want_status_out=True)
            dec.status.copy_(self.T(so))
            n_bad.copy_(self.T(np.array([nb], np.uint32)))
        else:
            self.cx.rawinput_batch(cap, coff, clen, clen, A.DLT_EN10MB, PARSE_FLAGS, tcp, dec)
            self.cx.verify_wire_batch(cap, coff, clen, A.DLT_EN10MB, self.e(N, torch.uint8), status=dec.status, status_out=dec.status,
                                      n_bad=n_bad)
        return cap, coff, tcp, dec, n_bad

    def recv_ack(self, conn, hit, seq):
        if self.cx is None:
            ack = self.orc.tcp_recv_ack_batch(self.u32(conn), H(hit, np.uint8), self.u32(seq), self.u32(self.tab.ack))
            self.tab.load(ack=ack)
        else:
            self.cx.tcp_recv_ack_batch(conn, hit, seq, self.tab.ack)

    def resolve(self, dec, conn, hit, miss, n_miss):
        if self.cx is None:
            c, h, m, nm = rc.conn_resolve_host(self.tab, H(dec.status, np.int8), H(dec.conn_key, np.uint64), cmd=H(dec.cmd, np.uint8),
                                               id=H(dec.id, np.uint8))
            conn[: len(c)].copy_(self.T(c)), hit[: len(c)].copy_(self.T(h)), miss[: len(c)].copy_(self.T(m))
            n_miss.copy_(self.T(np.array([nm], np.uint32)))
        else:
            self.cx.conn_resolve_batch(self.tab, dec.status, dec.conn_key, conn, cmd=dec.cmd, id=dec.id, hit=hit, miss=miss,
                                       n_miss=n_miss)

    def demux_deliver(self, cap, coff, tcp, dec, status, n):
        """-> (segments [(first, [packets])], the bytes of each segment)."""
        if self.cx is None:
            segs, nv = self.orc.demux_batch(H(status, np.int8), H(dec.cmd, np.uint8), DEMUX_FIELDS, id=H(dec.id, np.uint8),
                                            conv=self.u32(dec.conv), dst=self.u32(tcp.dst))
            perm = np.array([i for _f, idx in segs for i in idx], np.uint32)
            seg_off = np.cumsum([0] + [len(idx) for _f, idx in segs]).astype(np.uint32)
            arena, out_off, _tot = rc.deliver_host(H(cap, np.uint8), H(coff, np.uint64), H(dec.pay_off, np.uint16),
                                                   H(dec.pay_len, np.uint16), H(status, np.int8), inner_off=H(tcp.cap_pay_off, np.uint16),
                                                   order=np.concatenate([perm, np.zeros(1, np.uint32)]), n_order=nv)
        else:
            dmx = rc.DemuxBuffers.alloc(n, self.dev)
            self.cx.demux_batch(status, dec.cmd, DEMUX_FIELDS, dmx, id=dec.id, conv=dec.conv, dst=tcp.dst)
            out = rc.DeliverBuffers.alloc(n, self.dev, int(H(dec.pay_len, np.uint16).astype(np.int64).sum()) + 16)
            self.cx.deliver_batch(cap, coff, dec.pay_off, dec.pay_len, status, out, inner_off=tcp.cap_pay_off, order=dmx.perm,
                                  n_order=dmx.n_valid)
            self.sync()
            segs, arena, out_off, seg_off = dmx.segments(), H(out.arena, np.uint8), H(out.out_off, np.uint64), self.u32(dmx.seg_off)
        return segs, [bytes(rc.segment_bytes(arena, out_off, seg_off, s)) for s in range(len(segs))]

    # ---- ACCEPT ----
    def accept(self, tuples, now):
        k = len(tuples)
        t = np.array(tuples, np.uint64).reshape(k, 4)
        row, cnt = self.e(k), self.e(4)
        self.call("pool_add_batch", self.sockp, self.T(t[:, 0], np.uint32), self.T(t[:, 2], np.uint32), self.T(t[:, 1], np.uint16),
                  self.T(t[:, 3], np.uint16), now + PERSIST_MS, k, self.sockp.add_work(k), row=row, n_new=cnt[0:1], n_again=cnt[1:2],
                  n_full=cnt[2:3], n_zero_port=cnt[3:4])
        self.sync()
        rows = self.u32(row)[:k]
        for tup, r in zip(tuples, rows.tolist()):  # the host keeps the socket object by its row
            if r != A.CONN_NONE:
                self.sock_of.setdefault(r, tuple(int(x) for x in tup))
        assert self.u32(cnt)[2] == 0
        return rows.tolist()

    # ---- CAPTURE ----
    def capture(self, frames, now, draws):
        arena, off, ln = frames
        n, mu = len(off), self.mutant
        N = self.fixed or n
        self._ns, self._seq = "capture", 0
        cap, coff, tcp, dec, n_bad = self.parse_verify(arena, off, ln)
        tab, ctab, ackp, sockp = self.tab, self.ctab, self.ackp, self.sockp
        # harvest: the add carries the batch's expiry, a value: it stays in front of a captured chain
        acnt = self.e(4)
        self.call("pool_add_batch", ackp, tcp.src, tcp.dst, tcp.sp, tcp.dp, now + PERSIST_MS, N, self.keep(lambda: ackp.add_work(N)),
                  seq=tcp.seq, ack=tcp.ack, parse_status=tcp.parse_status, touch=True, n_new=acnt[0:1], n_again=acnt[1:2],
                  n_full=acnt[2:3], n_zero_port=acnt[3:4])
        # every buffer of the chain, then the chain: library calls only, so that it captures as it stands
        m = self.m_max
        mm, vm = min(m, tab.capacity), min(N, ctab.capacity)
        ob = {k: self.e(m, dt) for k, dt in (("src", torch.int32), ("dst", torch.int32), ("sp", torch.int16), ("dp", torch.int16),
                                            ("ack", torch.int32), ("flag", torch.uint8))}
        n_offer, oar, osr, n_over = self.e(1), self.e(m), self.e(m), self.e(1)
        offers = rc.ConnOffers(ob["src"], ob["dst"], ob["sp"], ob["dp"], ob["ack"], ob["flag"], n_offer, m_max=m)
        conn, hit, miss, n_miss = self.e(N), self.e(N, torch.uint8), self.e(N, torch.int8), self.e(1)
        hit_before = self.e(N, torch.uint8)
        co = {"new_rows": self.e(mm), "new_first": self.e(mm), "new_offer": self.e(mm), "offer_row": self.e(m), "n_new": self.e(1),
              "n_full": self.e(1), "n_refused": self.e(1), "pick_counts": self.e(2)}
        taken, closed_s, scnt = self.e(mm), self.e(sockp.capacity), self.e(2)
        ctl = self.keep(lambda: rc.ControlBuffers.alloc(N, self.dev, capacity=tab.capacity))
        marked, n_marked, pcnt = self.e(tab.capacity), self.e(1), self.e(2)
        conv_row, unknown, n_unk, crst = self.e(N), self.e(N, torch.int8), self.e(1), self.e(ctab.capacity)
        v1 = {"new_rows": self.e(vm), "new_first": self.e(vm), "n_new": self.e(1), "n_full": self.e(1)}
        v2 = {"new_rows": self.e(vm), "new_first": self.e(vm), "n_new": self.e(1), "n_full": self.e(1)}
        vclosed, vat, vcnt = self.e(ctab.capacity), self.e(ctab.capacity), self.e(3)
        w_create, w_settle = self.keep(lambda: tab.create_work(N, m)), self.keep(lambda: ackp.settle_work(sockp))
        w_close, w_conv = self.keep(tab.close_work), self.keep(lambda: ctab.create_work(N))

        def chain():
            # offers
            self.call("pool_offers", ackp, sockp, offers, offer_ack_row=oar, offer_sock_row=osr, n_over=n_over)
            # resolve -> recv_ack -> conn_create -> recv_ack -> settle
            self.resolve(dec, conn, hit, miss, n_miss)
            self.recv_ack(conn, hit, tcp.seq)
            hit_before.copy_(hit)
            self.call("conn_create_batch", tab, offers, w_create, u_max=N, id=dec.id, conn_key=dec.conn_key, src=tcp.src,
                      dst=tcp.dst, sp=tcp.sp, dp=tcp.dp, conn=conn, hit=hit, miss=miss, n_miss=n_miss, pick=True, now_ms=now,
                      established_ms=self.est, ka_tries=self.ka, **co)
            if mu != "no_second_recv_ack":
                self.recv_ack(conn, hit, tcp.seq)
            self.call("pool_settle_batch", ackp, sockp, w_settle, new_offer=co["new_offer"],
                      n_new=acnt[0:1] if mu == "settle_with_add_n_new" else co["n_new"], offer_ack_row=oar, offer_sock_row=osr, m_max=m,
                      miss=miss, src=tcp.src, dst=tcp.dst, sp=tcp.sp, dp=tcp.dp, new_max=mm, taken_sock_rows=taken,
                      closed_sock_rows=closed_s, n_closed=scnt[0:1], n_purged_ack=scnt[1:2])
            # control -> conn_close (the conns this batch killed)
            self.call("control_batch", tab, dec.status, dec.cmd, dec.pay_off, dec.pay_len, cap, coff, ctl, id=dec.id,
                      conn_key=dec.conn_key, inner_off=tcp.cap_pay_off, miss=miss, ka_tries=self.ka)
            self.call("conn_close_batch", tab, w_close, rst_first=ctl.rst_first, marked_rows=marked, n_marked=n_marked,
                      pick=mu != "close_without_pick", pick_counts=pcnt)
            # conv resolve -> create -> close (HOLD) -> create
            self.call("conv_resolve_batch", ctab, dec.status, dec.conv, conv_row, cmd=dec.cmd,
                      hit=hit_before if mu == "conv_resolve_with_old_hit" else hit, id=dec.id, dst=tcp.dst, ctl_kind=ctl.kind,
                      ctl_arg=ctl.arg, unknown=unknown, n_unknown=n_unk, rst_first=crst)
            self.call("conv_create_batch", ctab, dec.conv, conv_row, unknown, N, w_conv, id=dec.id, dst=tcp.dst, n_unknown=n_unk, **v1)
            self.call("conv_close_batch", ctab, rst_first=crst, ctl_kind=ctl.kind, conv_row=conv_row, unknown=unknown, n_unknown=n_unk,
                      hold=mu != "conv_close_without_hold", closed_rows=vclosed, closed_at=vat, n_closed=vcnt[0:1],
                      n_reopened=vcnt[1:2], n_rst_again=vcnt[2:3])
            self.call("conv_create_batch", ctab, dec.conv, conv_row, unknown, N, w_conv, id=dec.id, dst=tcp.dst, n_unknown=n_unk, **v2)

        self.graphed("data", chain)
        self._ns = None
        # the demux's status: the decode's, without the DATA packets that reached no conv (one elementwise pass)
        dstat = torch.where((dec.cmd == A.CMD_DATA) & (conv_row == -1), torch.full_like(dec.status, A.RECV_DROP), dec.status)
        self.sync()
        segs, seg_bytes = self.demux_deliver(cap, coff, tcp, dec, dstat, N)
        # host, after the batch: read the counts
        g = {k: int(self.u32(v)[0]) for k, v in (("n_bad", n_bad), ("n_offer", n_offer), ("n_over", n_over), ("n_miss", n_miss),
                                                 ("n_new", co["n_new"]), ("n_full", co["n_full"]), ("n_refused", co["n_refused"]),
                                                 ("n_marked", n_marked), ("n_ctl", ctl.n_ctl), ("n_msg", ctl.n_msg), ("n_unknown", n_unk),
                                                 ("v_new", v1["n_new"]), ("v_full", v1["n_full"]), ("v_reborn", v2["n_new"]),
                                                 ("v_full2", v2["n_full"]))}
        a4, s2, v3 = self.u32(acnt), self.u32(scnt), self.u32(vcnt)
        g.update(a_new=int(a4[0]), a_again=int(a4[1]), a_full=int(a4[2]), a_zero_port=int(a4[3]), closed_socks=int(s2[0]),
                 purged_ack=int(s2[1]), v_closed=int(v3[0]), n_reopened=int(v3[1]), n_rst_again=int(v3[2]))
        assert g["n_over"] == 0 and g["n_full"] == 0 and g["a_full"] == 0 and g["v_full"] == 0 and g["v_full2"] == 0
        # bind taken_sock_rows[j] to new_rows[j]; close closed_sock_rows
        new_rows = self.u32(co["new_rows"])[: g["n_new"]].tolist()
        if self.side == "graph" and new_rows:
            # a replayed create stamps the conns it bears with the now_ms of the capture (a value): the host writes theirs
            self.est[torch.tensor(new_rows, dtype=torch.int64, device=self.dev)] = now
        for srow, crow in zip(self.u32(taken)[: g["n_new"]].tolist(), new_rows):
            self.bound[crow] = self.sock_of.pop(srow, ("no pooled socket in row", srow))  # the comparison of `bound` reports it
        closed_rows = self.u32(closed_s)[: g["closed_socks"]].tolist()
        for srow in closed_rows:
            self.closed.append(self.sock_of.pop(srow, ("no pooled socket in row", srow)))
        # clear LIVE of the HOLD rows
        held = self.u32(vclosed)[: g["v_closed"]].tolist()
        if held and mu not in ("hold_not_cleared", "conv_close_without_hold"):
            ctab.state[torch.tensor(held, dtype=torch.int64, device=self.dev)] &= 0xFE
        for k, v in (("status", H(dec.status, np.int8)), ("hit", H(hit, np.uint8)), ("miss", H(miss, np.int8)), ("kind", H(ctl.kind, np.uint8))):
            assert not (v[n:] != {"status": A.RECV_DROP, "miss": A.RECV_DROP}.get(k, 0)).any(), ("a packet behind the capture's end was handled", k)
        out = {"parse_status": H(tcp.parse_status, np.int8)[:n], "status": H(dec.status, np.int8)[:n], "conn": self.u32(conn)[:n],
               "hit": H(hit, np.uint8)[:n], "miss": H(miss, np.int8)[:n], "kind": H(ctl.kind, np.uint8)[:n], "arg": H(ctl.arg, np.uint64)[:n],
               "cconn": self.u32(ctl.conn)[:n], "conv_row": self.u32(conv_row)[:n], "unknown": H(unknown, np.int8)[:n], "counts": g, "conn_new_rows": new_rows,
               "conn_new_first": self.u32(co["new_first"])[: g["n_new"]].tolist(), "closed_sock_rows": sorted(closed_rows),
               "conv_closed_rows": sorted(held), "conv_new_rows": self.u32(v1["new_rows"])[: g["v_new"]].tolist(),
               "conv_new_first": self.u32(v1["new_first"])[: g["v_new"]].tolist(),
               "conv_reborn_rows": self.u32(v2["new_rows"])[: g["v_reborn"]].tolist(),
               "conv_reborn_first": self.u32(v2["new_first"])[: g["v_reborn"]].tolist(), "messages": ctl.messages(),
               "segments": segs, "segment_bytes": seg_bytes}
        out["sends"] = self.send_messages(ctl, g["n_msg"], draws)
        return out

    # ---- the answers: pick (avoid_key) -> expand -> send_seq -> wire ----
    def send_messages(self, msgs, k, draws):
        if k == 0:
            return []
        sl = lambda t, w=1: t[: k * w]  # noqa: E731
        return self.wire(k, sl(msgs.msg_id, 8), self.T(np.asarray(draws[:k], np.uint32)), sl(msgs.msg_avoid_key),
                         msgs.msg_body.view(torch.uint8), sl(msgs.msg_pay_off), sl(msgs.msg_pay_len), sl(msgs.msg_cmd),
                         torch.zeros(k, dtype=torch.int32, device=self.dev))

    def wire(self, k, id8, draw, avoid, payload, pay_off, pay_len, cmd, conv):
        tab = self.tab
        conn, n_none, used = self.e(k), self.e(1), torch.zeros(tab.capacity, dtype=torch.uint8, device=self.dev)
        x = {"src": self.e(k), "dst": self.e(k), "sp": self.e(k, torch.int16), "dp": self.e(k, torch.int16), "ack": self.e(k),
             "flag": self.e(k, torch.uint8), "conn_key": self.e(k, torch.int64)}
        ok, seq, ipid = self.e(k, torch.uint8), self.e(k), self.e(k, torch.int16)
        status = (W.HEAD + pay_len.to(torch.int32)).contiguous()
        if self.cx is None:
            c, nn = rc.conn_pick_host(tab, k, id=H(id8, np.uint8), avoid_key=None if avoid is None else H(avoid, np.uint64),
                                      draw=self.u32(draw), used=used.numpy())
            conn[:k].copy_(self.T(c))
            n_none.copy_(self.T(np.array([nn], np.uint32)))
            xo, _nb = rc.conn_expand_host(tab, c)
            for f in x:
                x[f][:k].copy_(self.T(xo[f]))
            ok[:k].copy_(self.T(xo["ok"]))
            s, i, cs, ipn = self.orc.tcp_send_seq_batch(c, H(status, np.int32), self.u32(tab.seq), int(H(self.ip_id_next, np.uint16)[0]))
            tab.load(seq=cs)
            self.ip_id_next.copy_(self.T(np.array([ipn], np.uint16)))
            seq[:k].copy_(self.T(s)), ipid[:k].copy_(self.T(i))
            pay, po, pl = H(payload, np.uint8), H(pay_off, np.uint64), H(pay_len, np.uint16)
            wires = []
            for j in range(k):
                st, fr = self.orc.rconn_output(KEY, pay[int(po[j]):int(po[j]) + int(pl[j])].tobytes(), int(H(cmd, np.uint8)[j]),
                                               H(id8, np.uint8)[8 * j:8 * j + 8].tobytes(), int(self.u32(conv)[j]),
                                               int(xo["conn_key"][j]))
                wires.append(self.orc.build_wire(fr, int(xo["src"][j]), int(xo["dst"][j]), int(xo["sp"][j]), int(xo["dp"][j]), int(s[j]),
                                                 int(xo["ack"][j]), int(xo["flag"][j]), int(i[j]), ETH))
        else:
            cx = self.cx
            cx.conn_pick_batch(tab, conn[:k], id=id8, avoid_key=avoid, draw=draw, n_none=n_none, used=used)
            cx.conn_expand_batch(tab, conn[:k], ok[:k], **{f: v[:k] for f, v in x.items()})
            cx.tcp_send_seq_batch(conn[:k], status, tab.seq, self.ip_id_next, seq[:k], ipid[:k])
            wl = (14 + 40 + status.to(torch.int64))
            woff = (torch.cumsum(wl, 0) - wl).contiguous()
            self.sync()
            buf = torch.zeros(int(wl.sum().item()) + 64, dtype=torch.uint8, device=self.dev)
            wst = self.e(k)
            cx.output_wire_batch(payload, pay_off, pay_len, cmd, conv, x["conn_key"][:k], x["src"][:k], x["dst"][:k], x["sp"][:k],
                                 x["dp"][:k], seq[:k], x["ack"][:k], x["flag"][:k], ipid[:k], buf, woff, wst[:k], eth=ETH, id=id8,
                                 )
            self.sync()
            assert np.array_equal(self.u32(wst)[:k], H(wl, np.int64))
            hb, ho = H(buf, np.uint8), H(woff, np.int64)
            wires = [hb[int(ho[j]):int(ho[j]) + int(H(wl, np.int64)[j])].tobytes() for j in range(k)]
        self.sync()
        # a pick of NONE or of a row that is not alive (ok 0) leaves a packet that does not parse back: check_sends reports it
        # host: clear RSK_CONN_NEW at the rows that sent
        if self.mutant != "new_never_cleared":
            tab.state[used.bool()] &= 0xFB
        return [dict(conn=int(self.u32(conn)[j]), wire=wires[j]) for j in range(k)]

    # ---- SEND: conv_send -> pick -> expand -> send_seq -> wire -> conv_send (count) ----
    def send(self, conv_rows, draws, payloads):
        k = len(conv_rows)
        rows = self.T(conv_rows, np.uint32)
        conv, id8, ok = self.e(k), self.e(8 * k, torch.uint8), self.e(k, torch.uint8)
        self.call("conv_send_batch", self.ctab, rows, conv=conv[:k], id=id8[: 8 * k], ok=ok[:k])
        pl = np.array([len(b) for b in payloads], np.uint16)
        po = np.concatenate([[0], np.cumsum(pl[:-1].astype(np.uint64))]).astype(np.uint64)
        pay = np.frombuffer(b"".join(payloads) + bytes(16), np.uint8).copy()
        self.sync()
        assert bool((H(ok, np.uint8)[:k] == 1).all())
        out = self.wire(k, id8[: 8 * k], self.T(draws, np.uint32), None, self.T(pay), self.T(po), self.T(pl),
                        torch.zeros(k, dtype=torch.uint8, device=self.dev), conv[:k])
        sent = self.T((W.HEAD + pl.astype(np.int32)).astype(np.int32))
        self.call("conv_send_batch", self.ctab, rows, sent=sent)
        self.sync()
        return out

    # ---- TICK ----
    def tick(self, now, which, draws):
        tab, ctab, mu = self.tab, self.ctab, self.mutant
        out = {"ka_dead": [], "conn_closed": [], "conv_dead": [], "ack_dead": [], "sock_dead": [], "sends": []}
        ka, cv = "ka" in which, "conv" in which
        self._ns, self._seq = "tick", 0
        kb = self.keep(lambda: rc.ControlBuffers.alloc(0, self.dev, capacity=tab.capacity, m=tab.capacity))
        closed, n_closed, marked, n_marked, pcnt = self.e(tab.capacity), self.e(1), self.e(tab.capacity), self.e(1), self.e(2)
        dead, n_dead, n_alive, vclosed, vn_closed = self.e(ctab.capacity), self.e(1), self.e(1), self.e(ctab.capacity), self.e(1)
        w_close, w_conv = self.keep(tab.close_work), self.keep(ctab.close_work)
        if ka:  # the flush carries now_ms, a value: it stays in front of a captured tick
            self.call("keepalive_flush", tab, self.ka, self.est, now, kb)

        def closes(ka=ka, cv=cv):
            if ka:
                self.call("conn_close_batch", tab, w_close, close_rows=kb.dead_rows, n_close=kb.n_dead, m_max=tab.capacity, remove=True,
                          sweep=True, marked_rows=marked, n_marked=n_marked, closed_rows=closed, n_closed=n_closed,
                          pick=mu != "close_without_pick", pick_counts=pcnt)
            if cv:
                self.call("conv_flush", ctab, dead_rows=dead, n_dead=n_dead, n_alive=n_alive)
                self.call("conv_close_batch", ctab, close_rows=dead, n_close=n_dead, m_max=ctab.capacity, work=w_conv,
                          closed_rows=vclosed, n_closed=vn_closed)

        if ka and cv:
            self.graphed("tick", closes)  # the graph of the tick: the conns' close, the convs' flush and close
        else:
            closes()
        self._ns = None
        self.sync()
        if cv:
            out["conv_dead"] = self.u32(vclosed)[: int(self.u32(vn_closed)[0])].tolist()
        if ka:
            out["ka_dead"] = self.u32(kb.dead_rows)[: int(self.u32(kb.n_dead)[0])].tolist()
            out["conn_closed"] = self.u32(closed)[: int(self.u32(n_closed)[0])].tolist()
            for r in out["conn_closed"]:  # host: close the sockets of closed_rows
                self.closed.append(self.bound.pop(r))
            out["requests"] = kb.messages()
            out["sends"] = self.send_messages(kb, int(self.u32(kb.n_msg)[0]), draws)
        if "pool" in which:
            for name, pool in (("ack_dead", self.ackp), ("sock_dead", self.sockp)):
                if name == "sock_dead" and mu == "no_sock_flush":
                    continue
                pdead, pn_dead = self.e(pool.capacity), self.e(1)
                self.call("pool_flush", pool, now, dead_rows=pdead, n_dead=pn_dead)
                self.sync()
                out[name] = self.u32(pdead)[: int(self.u32(pn_dead)[0])].tolist()
            for r in out["sock_dead"]:  # host: close the sockets of the socket pool's dead_rows
                self.closed.append(self.sock_of.pop(r))
        return out

    # ---- the tables on the host ----
    def tables(self):
        self.sync()
        t = {"conn": {k: H(getattr(self.tab, k), dt) for k, dt in (("state", np.uint8), ("conn_key", np.uint64), ("id", np.uint8),
                                                                  ("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16),
                                                                  ("dp", np.uint16), ("seq", np.uint32), ("ack", np.uint32),
                                                                  ("flag", np.uint8))},
             "conv": {k: H(getattr(self.ctab, k), dt) for k, dt in (("state", np.uint8), ("conv", np.uint32), ("dst", np.uint32),
                                                                   ("id", np.uint8), ("cur_in", np.uint32), ("cur_out", np.uint32),
                                                                   ("prev_in", np.uint32), ("prev_out", np.uint32), ("alive", np.uint8))},
             "ack": {k: H(getattr(self.ackp, k), dt) for k, dt in (("state", np.uint8), ("src", np.uint32), ("dst", np.uint32),
                                                                  ("sp", np.uint16), ("dp", np.uint16), ("seq", np.uint32),
                                                                  ("ack", np.uint32), ("expiry", np.uint64))},
             "sock": {k: H(getattr(self.sockp, k), dt) for k, dt in (("state", np.uint8), ("src", np.uint32), ("dst", np.uint32),
                                                                    ("sp", np.uint16), ("dp", np.uint16), ("expiry", np.uint64))}}
        t["conn"]["ka_tries"], t["conn"]["established_ms"] = H(self.ka, np.uint8), H(self.est, np.uint64)
        t["index"] = {"conn": H(self.tab.index, np.uint32), "conv": H(self.ctab.index, np.uint32), "ack": H(self.ackp.index, np.uint32),
                      "sock": H(self.sockp.index, np.uint32), "pick": H(self.tab.pick, np.uint32)}
        t["ip_id"] = int(H(self.ip_id_next, np.uint16)[0])
        return t

    def pick_probe(self, ids, draw):
        """The pick index, by its results: one pick per IdBuf with a fixed draw."""
        k = len(ids)
        idb = np.frombuffer(b"".join(ids), np.uint8).copy()
        dr = np.full(k, draw, np.uint32)
        if self.cx is None:
            return rc.conn_pick_host(self.tab, k, id=idb, draw=dr)[0].tolist()
        conn = self.e(k)
        self.cx.conn_pick_batch(self.tab, conn[:k], id=self.T(idb), draw=self.T(dr))
        self.sync()
        return self.u32(conn)[:k].tolist()


# ---- the comparison ------------------------------------------------------------------------------------------------
def id_words(a):
    return np.ascontiguousarray(a).view("<u8")


def check_tables(walk, chain, ids, what):
    snap, t = walk.snapshot(), chain.tables()
    for name in ("conn", "conv", "ack", "sock"):
        cols, rows = t[name], snap[name]
        live = np.nonzero(cols["state"] & 1)[0].tolist()
        assert live == sorted(rows), (what, name, "the LIVE rows", live[:8], sorted(rows)[:8])
        for r, want in rows.items():
            for k, v in want.items():
                have = cols[k][8 * r:8 * r + 8].tobytes() if k == "id" else int(cols[k][r])
                assert have == v, (what, name, "row", r, k, have, v)
    # rsk_conn.h's contract on all four indexes
    c = t["conn"]
    collide.index_invariant(t["index"]["conn"], len(c["state"]), c["state"], c["conn_key"], id_words(c["id"]), True, what=what + " conn")
    v = t["conv"]
    collide.index_invariant(t["index"]["conv"], len(v["state"]), v["state"], v["conv"].astype(np.uint64) | (v["dst"].astype(np.uint64) << np.uint64(32)),
                            id_words(v["id"]), True, what=what + " conv")
    for name in ("ack", "sock"):
        p = t[name]
        collide.index_invariant(t["index"][name], len(p["state"]), p["state"], (p["src"].astype(np.uint64) << np.uint64(32)) | p["dst"].astype(np.uint64),
                                (p["sp"].astype(np.uint64) << np.uint64(16)) | p["dp"].astype(np.uint64), by_id=True, what=what + " " + name)
    # the pick index, by its results
    for draw in (0, 1, 0x9E3779B1):
        want = [W.NONE if c is None else c.row for c in (walk.pick(g, draw) for g in ids)]
        assert chain.pick_probe(ids, draw) == want, (what, "pick", draw)
    assert chain.bound == snap["bound"], (what, "sockets bound")
    assert sorted(chain.closed) == snap["closed"], (what, "sockets closed")
    assert t["ip_id"] == snap["ip_id"], (what, "ip id")
    return t


def check_sends(oracle, got, want, what):
    """Every packet that left: parsed and verified back, and its fields against the walk's send."""
    assert len(got) == len(want), (what, "sends", len(got), len(want))
    for j, (g, w) in enumerate(zip(got, want)):
        assert w is not None, (what, "the walk found no conn for send", j)
        assert g["conn"] == w["conn"], (what, "send", j, "conn", g["conn"], w["conn"])
        b = g["wire"]
        a = np.frombuffer(b + bytes(64), np.uint8)
        o = oracle.parse_decode_batch(KEY, a, [0], [len(b)], [len(b)], A.DLT_EN10MB, 0)
        cs, _s, nb = rc.verify_wire_host(a, np.zeros(1, np.uint64), np.array([len(b)], np.uint32), A.DLT_EN10MB)
        ok = A.CSUM_IP_CHECKED | A.CSUM_IP_OK | A.CSUM_TCP_CHECKED | A.CSUM_TCP_OK
        assert int(cs[0]) & ok == ok and o["status"][0] == A.RECV_VALID, (what, "send", j, "does not verify")
        flen = W.HEAD + len(w["payload"])
        body = a[54 + W.HEAD:54 + flen].tobytes()
        ip_id = int.from_bytes(b[18:20], "big")
        # the parse stores a received packet's TcpInfo the way its answer travels: src <-> dst
        have = dict(conn=g["conn"], src=int(o["dst"][0]), dst=int(o["src"][0]), sp=int(o["dp"][0]), dp=int(o["sp"][0]),
                    seq=(int(o["seq"][0]) - flen) & W.M32, ack=int(o["ack"][0]), flag=int(o["flag"][0]), ip_id=ip_id,
                    cmd=int(o["cmd"][0]), id8=o["id"][:8].tobytes(), conv=int(o["conv"][0]), key=int(o["conn_key"][0]), payload=body)
        assert have == w, (what, "send", j, {k: (have[k], w[k]) for k in w if have[k] != w[k]})


def streams_of(got, packets, what):
    """The delivered bytes of every conv row, in arrival order; a control packet is a segment of its own."""
    streams = {}
    for (first, idx), b in zip(got["segments"], got["segment_bytes"]):
        if got["kind"][first] != W.K_NONE or packets[first].cmd != W.DATA:
            assert len(idx) == 1, (what, "a control packet shares a segment")
            continue
        r = int(got["conv_row"][first])
        assert all(int(got["conv_row"][i]) == r for i in idx), (what, "a segment of two convs")
        streams[r] = streams.get(r, b"") + b
    return streams


def check_capture(res, got, packets, what):
    for k in ("parse_status", "status", "conn", "hit", "miss", "kind", "arg", "cconn", "conv_row"):
        dt = np.int64 if k in ("parse_status", "status", "miss") else np.uint64
        a, b = np.asarray(got[k]).astype(dt), np.array(res[k], dtype=dt)
        assert np.array_equal(a, b), (what, k, np.nonzero(a != b)[0][:8])
    assert not (got["unknown"] == A.RECV_VALID).any(), (what, "a packet is still unknown")
    c, g = res["counts"], got["counts"]
    for k in c:
        assert g[k] == c[k], (what, "count", k, g[k], c[k])
    assert g["n_miss"] == int((np.array(res["miss"]) == W.VALID).sum()) and g["n_unknown"] == 0
    for k in ("conn_new_rows", "conn_new_first", "closed_sock_rows", "conv_closed_rows", "conv_new_rows", "conv_new_first", "conv_reborn_rows",
              "conv_reborn_first"):
        assert list(got[k]) == list(res[k]), (what, k, list(got[k])[:8], list(res[k])[:8])
    m = got["messages"]
    want = res["messages"]
    assert len(m["cmd"]) == len(want), (what, "messages", len(m["cmd"]), len(want))
    for j, (cmd, body, id8, avoid, src) in enumerate(want):
        have = (int(m["cmd"][j]), int(m["body"][j]), m["id"][j].tobytes(), int(m["avoid_key"][j]), int(m["src"][j]))
        assert have == (cmd, body, id8, avoid, src), (what, "message", j, have)
    streams = streams_of(got, packets, what)
    assert streams == res["delivered"], (what, "delivered bytes", sorted(streams)[:8], sorted(res["delivered"])[:8])


_FRAMES = {}  # (shape, seed, event, part) -> the capture's bytes; the scripts are a fixed set, each built once


def frames_of(oracle, sc, e, lo=0, hi=None):
    key = (sc["shape"], sc["seed"], e, lo, hi)
    if key not in _FRAMES:
        _FRAMES[key] = build_capture(oracle, sc["events"][e][1][lo:hi])
    return _FRAMES[key]


def run(sc, chain, oracle, events=None, after_event=None):
    """The script through the walk and the chain, compared after every event.  -> (walk.seen, the chain's outputs and
    tables after every event, for a byte-for-byte comparison with another side)."""
    p = sc["params"]
    walk = W.Walk(p["cap_conn"], p["cap_conv"], p["cap_pool"], p["cap_pool"], PERSIST_MS)
    trace = []
    for e, ev in enumerate(sc["events"][:events]):
        what = f"{sc['shape']} event {e} {ev[0]}"
        with chain.on():
            got, t = step(sc, e, ev, walk, chain, oracle, what)
        trace.append((got, t))
        if after_event is not None:
            after_event(e, ev, chain, walk)
    return walk.seen, trace


def step(sc, e, ev, walk, chain, oracle, what):
    """One event through the walk and the chain, compared.  -> (the chain's outputs, its tables on the host)."""
    if ev[0] == "ACCEPT":
        assert chain.accept(ev[1], ev[2]) == walk.accept(ev[1], ev[2]), (what, "rows")
        got = None
    elif ev[0] == "CAPTURE":
        res = walk.capture(ev[1], ev[2])
        want_sends = walk.send_queued(ev[3])
        got = chain.capture(frames_of(oracle, sc, e), ev[2], ev[3])
        check_capture(res, got, ev[1], what)
        check_sends(oracle, got["sends"], want_sends, what)
    elif ev[0] == "SEND":
        want_sends = walk.send(ev[1], ev[2], ev[3])
        got = {"sends": chain.send(ev[1], ev[2], ev[3])}
        check_sends(oracle, got["sends"], want_sends, what)
    else:
        res = walk.tick(ev[1], ev[2])
        want_sends = walk.send_queued(ev[3], tick=True)
        got = chain.tick(ev[1], ev[2], ev[3])
        for k in ("ka_dead", "conn_closed", "conv_dead", "ack_dead", "sock_dead"):
            assert got[k] == res[k], (what, k, got[k][:8], res[k][:8])
        if "ka" in ev[2]:
            m = got["requests"]
            have = [(int(m["cmd"][j]), int(m["body"][j]), m["id"][j].tobytes(), int(m["avoid_key"][j]), int(m["src"][j]))
                    for j in range(len(m["cmd"]))]
            assert have == res["requests"], (what, "requests")
        check_sends(oracle, got["sends"], want_sends, what)
    return got, check_tables(walk, chain, sc["ids"], what)


# ---- two sides, or two runs, byte for byte ---------------------------------------------------------------------------
def same(a, b, what):
    """Two sides' outputs or tables are the same, byte for byte (the opaque indexes are held to their contract and to
    the lookups' results by check_tables, not to their bytes)."""
    if isinstance(a, dict):
        assert sorted(a) == sorted(b), (what, sorted(a), sorted(b))
        for k in a:
            if k != "index":
                same(a[k], b[k], what + (k,))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), (what, len(a), len(b))
        for j, (x, y) in enumerate(zip(a, b)):
            same(x, y, what + (j,))
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, "differs at", np.nonzero(np.asarray(a != b).reshape(-1))[0][:8])
    else:
        assert a == b and type(a) is type(b), (what, a, b)


def same_trace(a, b, what):
    assert len(a) == len(b)
    for e, ((got_a, tab_a), (got_b, tab_b)) in enumerate(zip(a, b)):
        same(got_a, got_b, (what, "event", e, "outputs"))
        same(tab_a, tab_b, (what, "event", e, "tables"))


def live_rows(t):
    """A chain's tables with the columns of the vacant rows blanked: what a dead row still holds is not table content
    (the walk's comparison never reads it either), and it may differ between two runs that agree on every LIVE row."""
    out = dict(t)
    for name in ("conn", "conv", "ack", "sock"):
        live = (t[name]["state"] & 1) != 0
        out[name] = {k: np.where(np.repeat(live, len(v) // len(live)), v, 0).astype(v.dtype) for k, v in t[name].items()}
    return out


PER_PACKET = ("parse_status", "status", "conn", "hit", "miss", "kind", "arg", "cconn", "conv_row", "unknown")


def run_split(sc, whole, parts, oracle):
    """Split invariance, with no model: the script on two chains of one side, `whole` taking every capture in one
    batch and `parts` cut into the 2 to 5 consecutive batches the generator marked as safe.  After every event all
    tables, the sockets, the per-packet outputs, the answers' bytes and every conv's delivered bytes are the same.
    -> the number of batches `parts` ran."""
    batches = 0
    for e, ev in enumerate(sc["events"]):
        what = (sc["shape"], "split", "event", e, ev[0])
        if ev[0] == "CAPTURE":
            pk, now, draws, cuts = ev[1], ev[2], ev[3], ev[4]
            with whole.on():
                a = whole.capture(frames_of(oracle, sc, e), now, draws)
            cols, streams, sends = {k: [] for k in PER_PACKET}, {}, []
            for lo, hi in zip([0] + list(cuts), list(cuts) + [len(pk)]):
                with parts.on():
                    b = parts.capture(frames_of(oracle, sc, e, lo, hi), now, draws[len(sends):])
                batches += 1
                for k in PER_PACKET:
                    cols[k].append(b[k])
                for r, x in streams_of(b, pk[lo:hi], what).items():
                    streams[r] = streams.get(r, b"") + x
                sends += b["sends"]
            for k in PER_PACKET:
                same(a[k], np.concatenate(cols[k]), what + (k,))
            same(streams_of(a, pk, what), streams, what + ("delivered bytes",))
            same(a["sends"], sends, what + ("answers",))
        else:
            outs = []
            for c in (whole, parts):
                with c.on():
                    outs.append(c.accept(ev[1], ev[2]) if ev[0] == "ACCEPT" else c.send(ev[1], ev[2], ev[3]) if ev[0] == "SEND"
                                else c.tick(ev[1], ev[2], ev[3]))
            same(outs[0], outs[1], what + ("outputs",))
        with whole.on():
            ta = whole.tables()
        with parts.on():
            tb = parts.tables()
        same(live_rows(ta), live_rows(tb), what + ("tables",))
        assert whole.bound == parts.bound and whole.closed == parts.closed, (what, "sockets")
    return batches
