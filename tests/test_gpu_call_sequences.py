"""GPU: sequences of calls on one context.  The library keeps state between calls in per-stream scratch
(the demux key table and its "clean" word, the compaction epoch, the two-pass and output-stationary
encode records, the send-seq tables, the delivery and control tile sums), laid out by the batch size
and reallocated only to grow.  Every test here makes a context of its own, so the scratch history is
the test's, varies the batch size up and down between calls, compares every call with its reference
and reads the device error flags after it."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from tests import conn_ref as R
from tests import control_ref as C
from tests import deliver_ref as D
from tests.enc_paths import held
from tests.test_demux_oracle import ALL, make_case

pytestmark = pytest.mark.gpu

KEY = b"hello135"
# batch sizes that share a key table size T = table_size(n): the power of two >= 2 n
BRACKETS = {4096: (1025, 1300, 1700, 2048), 16384: (4097, 4800, 6000, 8192)}
SWEEP_FIELDS = (ALL, A.DEMUX_CONN_KEY | A.DEMUX_CMD_BARRIER, ALL | A.DEMUX_GROUP_BARRIER)


def table_size(n: int) -> int:
    t = 64
    while t < 2 * n:
        t <<= 1
    return t


def dev(a, gpu, dt=None):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dt) if dt is not None else a).to(gpu)


def new_codec():
    from rsock_amd.codec import Codec

    return Codec(KEY, 0)


# ---- demux batches, built and referenced once, never changed ---------------------------------------
class DmCase:
    """One demux batch: the host columns, the device copies (made on first use, with `cap` entries of
    room) and the oracle's result per field selection.  kind "few": 10 keys, every packet VALID, a
    control packet in 500 (few segments: the call clears its slots and leaves the table flagged clean);
    "distinct": every packet a key of its own (more than T / 16 segments: nothing is cleared); "mix":
    400 keys, 2 % control packets, 10 % not VALID."""

    def __init__(self, n: int, kind: str, seed: int = 0, p_ctrl: float | None = None):
        self.n, self.kind = n, kind
        rng = np.random.default_rng(1000 * n + len(kind) + seed)
        if kind == "few":
            cols = make_case(rng, n, 10, 0.002 if p_ctrl is None else p_ctrl, 1.0)
        elif kind == "mix":
            cols = make_case(rng, n, 400, 0.02 if p_ctrl is None else p_ctrl, 0.9)
        else:
            status = np.where(rng.random(n) < 0.95, A.RECV_VALID, A.RECV_DROP).astype(np.int8)
            cmd = np.where(rng.random(n) < 0.01, 3, 0).astype(np.uint8)
            cols = (status, cmd, rng.integers(0, 256, 8 * n, dtype=np.uint8), np.arange(n, dtype=np.uint32),
                    (rng.permutation(n).astype(np.uint64) + 1) * 7919, rng.integers(0, 2, n).astype(np.uint32))
        self.cols = cols
        self._dev = {}
        self._exp = {}

    def on(self, gpu, cap: int | None = None):
        """(status, cmd, id, conv, conn_key, dst) on the device: views of n entries into tensors of
        `cap` (default n) entries."""
        cap = self.n if cap is None else cap
        if cap not in self._dev:
            import torch

            full = []
            for a, dt, w in zip(self.cols, (np.int8, np.uint8, np.uint8, np.int32, np.int64, np.int32), (1, 1, 8, 1, 1, 1)):
                src = dev(a, gpu, dt)
                t = torch.zeros(cap * w, dtype=src.dtype, device=gpu)
                t[:self.n * w] = src
                full.append(t[:self.n * w])
            self._dev[cap] = tuple(full)
        return self._dev[cap]

    def expected(self, oracle, fields: int):
        """-> (perm [n_valid], seg_off [n_seg + 1], seg_first [n_seg]) of oracle.demux_batch."""
        if fields not in self._exp:
            segs, nv = oracle.demux_batch(self.cols[0], self.cols[1], fields, *self.cols[2:])
            lens = np.array([len(p) for _, p in segs], np.int64)
            perm = np.array([i for _, p in segs for i in p], np.uint32)
            assert len(perm) == nv
            self._exp[fields] = (perm, np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32),
                                 np.array([f for f, _ in segs], np.uint32))
        return self._exp[fields]


_CASES: dict = {}


def case(n: int, kind: str, seed: int = 0, p_ctrl: float | None = None) -> DmCase:
    k = (n, kind, seed, p_ctrl)
    if k not in _CASES:
        _CASES[k] = DmCase(n, kind, seed, p_ctrl)
    return _CASES[k]


def demux(cx, gpu, c: DmCase, fields: int, out=None, stream=None, cap: int | None = None):
    from rsock_amd.codec import DemuxBuffers

    st, cmd, ids, conv, ckey, dst = c.on(gpu, cap)
    out = DemuxBuffers.alloc(c.n if cap is None else cap, gpu) if out is None else out
    cx.demux_batch(st, cmd, fields, out, id=ids, conv=conv, conn_key=ckey, dst=dst, stream=stream)
    return out


def check_demux(out, c: DmCase, oracle, fields: int, what=None):
    """`out` (after its call has finished) against the oracle, segment for segment."""
    perm, seg_off, first = c.expected(oracle, fields)
    h = lambda t, k: t[:k].cpu().numpy().view(np.uint32)  # noqa: E731
    assert int(out.n_valid.item()) == len(perm), what
    assert int(out.n_seg.item()) == len(first), what
    assert np.array_equal(h(out.seg_first, len(first)), first), what
    assert np.array_equal(h(out.seg_off, len(seg_off)), seg_off), what
    assert np.array_equal(h(out.perm, len(perm)), perm), what


# ---- a. the same table size, a smaller batch ---------------------------------------------------------
def test_demux_same_table_smaller_batch(gpu, oracle):
    """A call that leaves the key table flagged clean, then a smaller batch with the same table size.

    The flag word (k_dm_final: `*tflag = tsize` after a call with at most T / 16 segments; k_dm_fill
    skips the table when `*tflag == tsize`; the host hint compares with tsize too) names the table
    size only, so the table has to lie at the same scratch offset for every n with that T.  Before
    this test existed dm_layout put it behind ten arrays of 4 n bytes (every piece rounded up to 256 B):
      n = 8192 (T = 16384): flag 256, cidx / hslot / rank_at / pep 4 * 32768, cpos 33024 (4 n + 4),
        seg_slot 32768 -> kA at 256 + 5 * 32768 + 33024 = 197120, then vA, kB, vB of 32768 B each
        (kA .. vB = [197120, 328192)), ghist 4096, two counters of 256: the table at 332800;
      n = 4800 (T = 16384 still): 256 + 9 * 19200 + 19456 + 4096 + 512 = 197120, the table's 131072
        bytes exactly over the larger call's kA .. vB.
    Call 1 (n = 8192, 10 keys, every packet VALID DATA, no barrier) has 8182 followers (> kSmallF =
    1024: k_dm_leader_rank writes them to kA / vA, k_dm_segof_hist turns kA into segment ids, one
    radix pass writes kB / vB) and 10 segments <= T / 16, so it leaves the flag at T; the
    synchronisation lets the host hint land, so call 2 takes k_dm_fill, which trusts the flag.  Call 2
    (n = 4800, about 400 keys) then found at most 20 of its 16384 slots free (words 8182 .. 8191 of
    the four arrays) and the rest holding segment ids and packet indices: its probes walked the whole
    table, gave up with RSK_DEVERR_TABLE and named stale words as leaders.  With the table at an
    offset that depends on T alone, call 2 finds the table call 1 cleared.

    Two calls come first so that every word such a failed call 2 could read is known (no fresh device
    memory): 8192 distinct keys (every rank_at word a rank) and one key (kA .. vB words 0 .. 8190).
    The stale words are then below 16384 (slot numbers, packet indices, ranks), and the tensors have
    room for 32768 entries, so even a library with the bug writes inside them."""
    import torch

    cap = 32768
    cx = new_codec()
    try:
        one = case(8192, "few", seed=1, p_ctrl=0.0)
        one_key = DmCase(8192, "few", seed=2, p_ctrl=0.0)
        one_key.cols = (one.cols[0], one.cols[1], np.zeros(8 * 8192, np.uint8), np.zeros(8192, np.uint32),
                        np.full(8192, 77, np.uint64), np.zeros(8192, np.uint32))
        distinct = DmCase(8192, "distinct", seed=3)
        distinct.cols = (one.cols[0], one.cols[1]) + distinct.cols[2:]  # every packet VALID DATA
        small = case(4800, "mix", seed=4, p_ctrl=0.0)
        assert (one.cols[0] == A.RECV_VALID).all() and not one.cols[1].any()
        assert len(one.expected(oracle, ALL)[2]) == 10
        n_keys = len(small.expected(oracle, ALL)[2])
        assert 300 <= n_keys <= table_size(4800) // 16 and table_size(4800) == table_size(8192) == 16384
        for k, c in enumerate((distinct, one_key, one, small)):
            out = demux(cx, gpu, c, ALL, cap=cap)
            torch.cuda.synchronize()
            check_demux(out, c, oracle, ALL, k)
            assert cx.check_device_errors() == 0
    finally:
        cx.close()


# ---- b. every ordered pair of sizes inside a table size ---------------------------------------------
@pytest.mark.parametrize("sync", [True, False], ids=["sync", "nosync"])
@pytest.mark.parametrize("tsize", sorted(BRACKETS))
def test_demux_layout_sweep(gpu, oracle, tsize, sync):
    """n1, n2, n1 on one stream for every ordered pair of sizes with one table size, the first call
    leaving the table flagged clean (10 keys) or not (a key per packet), over three field selections.
    sync: the host waits after every call, so the hint is current and a clean table takes k_dm_fill;
    nosync: the three calls are issued back to back (the hint lags: the memset form, or k_dm_fill
    against a flag another size set) and compared at the end."""
    import torch

    sizes = BRACKETS[tsize]
    assert all(table_size(n) == tsize for n in sizes)
    cx = new_codec()
    try:
        for fields in SWEEP_FIELDS:
            for kind in ("few", "distinct"):
                for n1 in sizes:
                    first = case(n1, kind)
                    ns = len(first.expected(oracle, fields)[2])
                    assert ns <= tsize // 16 if kind == "few" else ns > tsize // 16, (n1, kind, fields, ns)
                    for n2 in sizes:
                        if n2 == n1:
                            continue
                        calls = (first, case(n2, "mix"), case(n1, "mix"))
                        outs = []
                        for c in calls:
                            outs.append(demux(cx, gpu, c, fields))
                            if sync:
                                torch.cuda.synchronize()
                        torch.cuda.synchronize()
                        for k, (c, out) in enumerate(zip(calls, outs)):
                            check_demux(out, c, oracle, fields, (fields, kind, n1, n2, k))
                        assert cx.check_device_errors() == 0
    finally:
        cx.close()


# ---- c. the send-seq group-by over the same scratch --------------------------------------------------
def _send_case(n, n_conn, seed):
    rng = np.random.default_rng(seed)
    conn = rng.integers(0, n_conn + 2, n).astype(np.uint32)  # some ids past n_conn
    status = np.where(rng.random(n) < 0.9, rng.integers(32, 1501, n), rng.choice([0, -1], n)).astype(np.int32)
    return conn, status


class SendState:
    """conn_seq / ip_id_next on the device and carried on the host through the oracle."""

    def __init__(self, gpu, n_conn, seed):
        rng = np.random.default_rng(seed)
        self.cs = rng.integers(0, 2**32, n_conn, dtype=np.uint64).astype(np.uint32)
        self.cs[0] = 0xFFFFF000  # wraps
        self.ip = 65000
        self.d_cs, self.d_ip = dev(self.cs, gpu, np.int32), dev(np.array([self.ip], np.uint16), gpu, np.int16)

    def step(self, oracle, conn, status):
        es, ei, self.cs, self.ip = oracle.tcp_send_seq_batch(conn, status, self.cs, self.ip)
        return es, ei

    def check(self, seq, ipid, es, ei, what):
        assert np.array_equal(seq.cpu().numpy().view(np.uint32), es), what
        assert np.array_equal(ipid.cpu().numpy().view(np.uint16), ei), what
        assert np.array_equal(self.d_cs.cpu().numpy().view(np.uint32), self.cs), what
        assert int(self.d_ip.cpu().numpy().view(np.uint16)[0]) == self.ip, what


def test_send_seq_groupby_across_sizes(gpu, oracle):
    """rsk_tcp_send_seq_batch held to its group-by path (which calls rsk_demux_batch on the stream's
    demux scratch) over n = 8192, 4800, 8192, 4097 with 7 connections -- few segments, so every call
    leaves the table flagged clean for the next, smaller or larger, one -- and a caller's own demux of
    another size with the same table size between them; conn_seq and ip_id_next carry over."""
    import torch

    cx = new_codec()
    try:
        cx.set_send_seq_groupby(1)
        state = SendState(gpu, 7, 5)
        between = (case(6000, "mix"), case(8192, "few"), case(4097, "distinct"), case(4800, "mix"))
        for k, n in enumerate((8192, 4800, 8192, 4097)):
            conn, status = _send_case(n, 7, 50 + k)
            seq = torch.empty(n, dtype=torch.int32, device=gpu)
            ipid = torch.empty(n, dtype=torch.int16, device=gpu)
            cx.tcp_send_seq_batch(dev(conn, gpu, np.int32), dev(status, gpu), state.d_cs, state.d_ip, seq, ipid)
            out = demux(cx, gpu, between[k], ALL)
            torch.cuda.synchronize()
            state.check(seq, ipid, *state.step(oracle, conn, status), k)
            check_demux(out, between[k], oracle, ALL, k)
            assert cx.check_device_errors() == 0
    finally:
        cx.close()


def test_send_seq_many_connections_shrinking_batch(gpu, oracle):
    """The path a server takes without any knob: 3000 connections (past the table path's 2047), a batch
    of 131072 packets and then one of 70000 -- both with a key table of 262144 slots, the first with
    3000 segments (<= T / 16: it leaves the table flagged clean)."""
    import torch

    assert table_size(131072) == table_size(70000) == 262144 and 3000 <= 262144 // 16
    cx = new_codec()
    try:
        state = SendState(gpu, 3000, 6)
        for k, n in enumerate((131072, 70000)):
            conn, status = _send_case(n, 3000, 60 + k)
            seq = torch.empty(n, dtype=torch.int32, device=gpu)
            ipid = torch.empty(n, dtype=torch.int16, device=gpu)
            cx.tcp_send_seq_batch(dev(conn, gpu, np.int32), dev(status, gpu), state.d_cs, state.d_ip, seq, ipid)
            torch.cuda.synchronize()
            state.check(seq, ipid, *state.step(oracle, conn, status), k)
            assert cx.check_device_errors() == 0
    finally:
        cx.close()


# ---- d. two streams, one context ---------------------------------------------------------------------
def test_demux_two_streams_one_hint(gpu, oracle):
    """Two streams of one context alternate demux calls of the sizes of one table size.  The scratch
    (table, flag word) is per stream; the host hint is one word per context, so each stream's choice
    between memset and k_dm_fill is made on the other stream's last verdict as often as on its own."""
    import torch

    cx = new_codec()
    try:
        sa, sb = torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)
        plan_a = [(8192, "few"), (4800, "mix"), (6000, "few"), (4097, "mix"), (8192, "mix"), (4800, "few"), (4097, "mix")]
        plan_b = [(4097, "distinct"), (8192, "few"), (4800, "mix"), (6000, "distinct"), (4097, "few"), (6000, "mix"),
                  (8192, "mix")]
        for fields in (ALL, A.DEMUX_CONN_KEY | A.DEMUX_CMD_BARRIER):
            for c in {case(*p) for p in plan_a + plan_b}:
                c.on(gpu)  # uploaded on the default stream, before either side stream runs
            torch.cuda.synchronize()
            done = []
            for k, (pa, pb) in enumerate(zip(plan_a, plan_b)):
                for s, p in ((sa, pa), (sb, pb)) if k % 2 == 0 else ((sb, pb), (sa, pa)):
                    with torch.cuda.stream(s):
                        done.append((case(*p), demux(cx, gpu, case(*p), fields, stream=s)))
                if k % 3 == 2:  # now and then the hint is current
                    torch.cuda.synchronize()
            torch.cuda.synchronize()
            for k, (c, out) in enumerate(done):
                check_demux(out, c, oracle, fields, (fields, k))
            assert cx.check_device_errors() == 0
    finally:
        cx.close()


# ---- e. captured graphs ------------------------------------------------------------------------------
def _overwrite(c_dev, src: DmCase, gpu):
    """The captured input tensors rewritten in place with another batch of the same size."""
    for t, s in zip(c_dev, src.on(gpu)):
        t.copy_(s)


@pytest.mark.parametrize("before", ["clean", "dirty"])
def test_demux_in_captured_graph(gpu, oracle, before):
    """rsk_demux_batch captured on a side stream and replayed three times with the inputs rewritten in
    place.  A captured call records k_dm_fill whatever the hint says: the kernel reads the flag word at
    every replay.  "clean": the eager call before the capture left the table clean -- an eager demux of
    another size with the same table size runs between the replays and leaves the flag either way;
    "dirty": the eager call had a key per packet, so the flag is 0, the hint says dirty (an uncaptured
    call would take the memset) and the first replay's k_dm_fill has the whole table to fill.  (The
    first build of this test found the memset in the graph: its first replay ended in an illegal memory
    access; the library no longer records it.)"""
    import torch

    from rsock_amd.codec import DemuxBuffers

    n, fields = 4800, ALL | A.DEMUX_CMD_BARRIER
    cx = new_codec()
    try:
        s = torch.cuda.Stream(gpu)
        eager = case(n, "few" if before == "clean" else "distinct")
        batches = (case(n, "mix"), case(n, "distinct"), case(n, "few"))
        others = (case(8192, "few"), case(4097, "distinct"), case(6000, "mix"))
        for c in (eager,) + batches + others:
            c.on(gpu)
        live = tuple(t.clone() for t in eager.on(gpu))  # the tensors the graph reads
        out = DemuxBuffers.alloc(n, gpu)
        torch.cuda.synchronize()

        def call(stream):
            st, cmd, ids, conv, ckey, dst = live
            cx.demux_batch(st, cmd, fields, out, id=ids, conv=conv, conn_key=ckey, dst=dst, stream=stream)

        with torch.cuda.stream(s):
            # the scratch is sized for the largest batch that will run on this stream (it must not be
            # reallocated under the graph, and a demux has no reserve call), then the capture's own
            # size: the flag word is initialised and says what `eager` left
            first = demux(cx, gpu, others[0], fields, stream=s)
            call(s)
        torch.cuda.synchronize()  # ... and the hint has landed
        check_demux(first, others[0], oracle, fields, "sizing")
        check_demux(out, eager, oracle, fields, "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            call(torch.cuda.current_stream())
        for r, (c, other) in enumerate(zip(batches, others)):
            _overwrite(live, c, gpu)
            for t in (out.perm, out.seg_off, out.seg_first, out.n_seg, out.n_valid):
                t.fill_(-1)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            torch.cuda.synchronize()
            check_demux(out, c, oracle, fields, r)
            if before == "clean":
                with torch.cuda.stream(s):
                    o2 = demux(cx, gpu, other, fields, stream=s)
                torch.cuda.synchronize()
                check_demux(o2, other, oracle, fields, ("between", r))
        assert cx.check_device_errors() == 0  # a captured context: waits for the device
        del g
    finally:
        cx.close()


@pytest.mark.parametrize("groupby", [0, 2])
def test_send_seq_in_captured_graph(gpu, oracle, groupby):
    """rsk_tcp_send_seq_batch captured and replayed three times, by the table path with either column
    scan: conn, status rewritten in place between the replays, conn_seq and ip_id_next advancing on the
    device from replay to replay.  (The group-by path is not captured here: it records a memset node of
    4 n bytes for seq, kin to the one test_demux_in_captured_graph found faulting.)"""
    import torch

    n, n_conn = 4800, 7
    cx = new_codec()
    try:
        cx.set_send_seq_groupby(groupby)
        s = torch.cuda.Stream(gpu)
        state = SendState(gpu, n_conn, 7)
        conn, status = _send_case(n, n_conn, 70)
        d_conn, d_status = dev(conn, gpu, np.int32), dev(status, gpu)
        seq = torch.empty(n, dtype=torch.int32, device=gpu)
        ipid = torch.empty(n, dtype=torch.int16, device=gpu)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            cx.tcp_send_seq_batch(d_conn, d_status, state.d_cs, state.d_ip, seq, ipid, stream=s)
        torch.cuda.synchronize()
        state.check(seq, ipid, *state.step(oracle, conn, status), "eager")
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cx.tcp_send_seq_batch(d_conn, d_status, state.d_cs, state.d_ip, seq, ipid,
                                  stream=torch.cuda.current_stream())
        for r in range(3):
            conn, status = _send_case(n, n_conn, 71 + r)
            d_conn.copy_(dev(conn, gpu, np.int32))
            d_status.copy_(dev(status, gpu))
            seq.fill_(-1)
            ipid.fill_(-1)
            torch.cuda.synchronize()
            with torch.cuda.stream(s):
                g.replay()
            torch.cuda.synchronize()
            state.check(seq, ipid, *state.step(oracle, conn, status), r)
        assert cx.check_device_errors() == 0
        del g
    finally:
        cx.close()


# ---- f. the other scratch kinds: one pipeline over shrinking and growing batches ---------------------
PIPE_SIZES = (40000, 16384, 33000, 16385)  # all >= kTwoPassMinPackets (16384): the two-pass forms run
PIPE_PATHS = ((2, 1), (2, 4), (2, -1))
PIPE_FIELDS = ALL  # 600 keys over the batch: long segments, the radix passes run


class PipeCase:
    """n packets for encode -> decode -> demux -> deliver -> control, with every stage's reference:
    byte-packed frames (mostly short payloads, one in eight of 1200 .. 1400 B), 5 % control packets
    whose bodies name keys of a pool half of which the connection table holds, one frame in 16
    corrupted before the decode."""

    def __init__(self, n: int, gpu, oracle, ref_cx):
        import torch

        self.n = n
        rng = np.random.default_rng(n)
        cmd = np.where(rng.random(n) < 0.05, rng.integers(1, 5, n), 0).astype(np.uint8)
        plen = np.where(rng.random(n) < 0.125, rng.integers(1200, 1401, n), rng.integers(1, 200, n))
        plen = np.where(cmd == 1, 4, np.where(cmd >= 2, 8, plen)).astype(np.uint16)
        pay_off = np.concatenate([[3], 3 + np.cumsum(plen[:-1].astype(np.int64) + rng.integers(0, 9, n - 1))]).astype(np.uint64)
        payload = rng.integers(0, 256, int(pay_off[-1]) + 1500, dtype=np.uint8)
        pool = rng.integers(1, 2**62, 64, dtype=np.uint64)
        for i in np.nonzero(cmd)[0].tolist():  # the control bodies: a conv (4 B) or a key of the pool (8 B)
            body = int(pool[rng.integers(0, 64)]).to_bytes(8, "little")[:int(plen[i])]
            payload[int(pay_off[i]): int(pay_off[i]) + len(body)] = np.frombuffer(body, np.uint8)
        conv = rng.integers(0, 4, n).astype(np.uint32)
        ckey = rng.integers(1, 2**40, 50, dtype=np.uint64)[rng.integers(0, 50, n)]
        flen = plen.astype(np.int64) + 31
        frame_off = (5 + np.concatenate([[0], np.cumsum(flen)[:-1]])).astype(np.uint64)
        self.frame_bytes = int(frame_off[-1] + flen[-1]) + 64
        self.enc_in = (dev(payload, gpu), dev(pay_off, gpu, np.int64), dev(plen, gpu, np.int16), dev(cmd, gpu),
                       dev(conv, gpu, np.int32), dev(ckey, gpu, np.int64))
        self.frame_off, self.frame_len = dev(frame_off, gpu, np.int64), dev(flen.astype(np.uint16), gpu, np.int16)
        self.corrupt = dev(frame_off[np.arange(7, n, 16)], gpu, np.int64)
        self.dst = dev(rng.integers(0, 3, n).astype(np.uint32), gpu, np.int32)
        # the encode's reference: the per-set kernel's bytes, from a context that runs nothing else
        self.frame = torch.zeros(self.frame_bytes, dtype=torch.uint8, device=gpu)
        self.status = torch.empty(n, dtype=torch.int32, device=gpu)
        with held(ref_cx, 1):
            self.encode(ref_cx)
        torch.cuda.synchronize()
        self.exp_frame, self.exp_status = self.frame.clone(), self.status.clone()
        assert bool((self.exp_status == self.frame_len.to(torch.int32)).all())
        # decode, demux, deliver, control: the oracle and the numpy restatements on the corrupted frames
        self.exp_frame[self.corrupt] ^= 1
        frames = self.exp_frame.cpu().numpy().copy()
        self.exp_frame[self.corrupt] ^= 1
        self.exp_dec = dec = oracle.decode_batch(KEY, frames, frame_off, flen.astype(np.uint16))
        assert 0.9 * n < dec["n_valid"] < n
        dst = self.dst.cpu().numpy().view(np.uint32)
        segs, nv = oracle.demux_batch(dec["status"], dec["cmd"], PIPE_FIELDS, dec["id"], dec["conv"], dec["conn_key"], dst)
        perm = np.full(n, D.STRAY, np.uint32)
        perm[:nv] = [i for _, p in segs for i in p]
        self.exp_demux = (perm[:nv].copy(), np.concatenate([[0], np.cumsum([len(p) for _, p in segs])]).astype(np.uint32),
                          np.array([f for f, _ in segs], np.uint32))
        arena, off, total = D.expected(D.Case(frames, frame_off, None, dec["pay_off"], dec["pay_len"], dec["status"],
                                              perm, nv), 1)
        self.exp_deliver = (dev(arena, gpu), off, total)
        cap = 257
        self.cols = R.random_columns(rng, cap)
        R.place(self.cols, rng.permutation(cap)[:32], pool[:32])
        self.ctl = dict(status=dec["status"], cmd=dec["cmd"], id=dec["id"], conn_key=dec["conn_key"], pay_off=dec["pay_off"],
                        pay_len=dec["pay_len"], arena=frames, base_off=frame_off, inner_off=None, tcp_sp=None, tcp_dp=None,
                        miss=None)
        self.ka = rng.choice(np.array([A.KA_NONE, 0, 1, 2], np.uint8), cap)
        self.exp_ctl = C.snapshot_ref(self.ctl, R.table_map(self.cols["state"], self.cols["conn_key"])[0], cap, False, self.ka)
        assert self.exp_ctl["n_msg"] > 0 and (self.exp_ctl["conn"] != C.NONE).any()

    def encode(self, cx):
        from rsock_amd import workload

        payload, pay_off, plen, cmd, conv, ckey = self.enc_in
        self.frame.zero_()
        self.status.fill_(-9)
        cx.output_batch(payload, pay_off, plen, cmd, conv, ckey, self.frame, self.frame_off, self.status,
                        id_uniform=workload.ID_UNIFORM)


def _pipeline_round(cx, gpu, p: PipeCase, tab, what):
    import torch

    from rsock_amd import codec as rc
    from tests.test_gpu_parity import assert_dec_equal

    n = p.n
    p.encode(cx)
    assert torch.equal(p.status, p.exp_status), what
    assert torch.equal(p.frame, p.exp_frame), what
    p.frame[p.corrupt] ^= 1
    dec = rc.DecodeBuffers.alloc(n, gpu)
    cx.onrecv_batch(p.frame, p.frame_off, p.frame_len, dec)
    dmx = rc.DemuxBuffers.alloc(n, gpu)
    cx.demux_batch(dec.status, dec.cmd, PIPE_FIELDS, dmx, id=dec.id, conv=dec.conv, conn_key=dec.conn_key, dst=p.dst)
    arena, off, total = p.exp_deliver
    dl = rc.DeliverBuffers.alloc(n, gpu, total + 256)
    dl.cap = total
    dl.arena.fill_(0xA5)
    cx.deliver_batch(p.frame, p.frame_off, dec.pay_off, dec.pay_len, dec.status, dl, order=dmx.perm, n_order=dmx.n_valid)
    ctl = rc.ControlBuffers.alloc(n, gpu, capacity=tab.capacity)
    tries = dev(p.ka, gpu)
    cx.control_batch(tab, dec.status, dec.cmd, dec.pay_off, dec.pay_len, p.frame, p.frame_off, ctl, id=dec.id,
                     conn_key=dec.conn_key, ka_tries=tries)
    torch.cuda.synchronize()
    # decode with compaction
    got = dec.to_host()
    assert_dec_equal(got, p.exp_dec)
    nv = int(got["n_valid"][0])
    assert nv == p.exp_dec["n_valid"], what
    assert np.array_equal(got["valid_idx"][:nv].view(np.uint32), p.exp_dec["valid_idx"][:nv]), what
    # demux
    perm, seg_off, first = p.exp_demux
    h = lambda t, k: t[:k].cpu().numpy().view(np.uint32)  # noqa: E731
    assert int(dmx.n_valid.item()) == len(perm) and int(dmx.n_seg.item()) == len(first), what
    assert np.array_equal(h(dmx.seg_first, len(first)), first) and np.array_equal(h(dmx.seg_off, len(seg_off)), seg_off), what
    assert np.array_equal(h(dmx.perm, len(perm)), perm), what
    # deliver
    assert int(dl.total.item()) == total, what
    assert np.array_equal(dl.out_off.cpu().numpy().view(np.uint64), off), what
    assert torch.equal(dl.arena[:total], arena) and bool((dl.arena[total:] == 0xA5).all()), what
    # control
    want = p.exp_ctl
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    assert np.array_equal(ctl.kind.cpu().numpy(), want["kind"]) and np.array_equal(u32(ctl.conn), want["conn"]), what
    assert np.array_equal(ctl.arg.cpu().numpy().view(np.uint64), want["arg"]), what
    assert int(u32(ctl.n_msg)[0]) == want["n_msg"] and int(u32(ctl.n_ctl)[0]) == want["n_ctl"], what
    assert np.array_equal(u32(ctl.rst_first), want["rst_first"]) and np.array_equal(tries.cpu().numpy(), want["ka_tries"]), what
    for name, a in ctl.messages().items():
        assert np.array_equal(a, want["msgs"][name]), (what, name)
    assert cx.check_device_errors() == 0


def test_pipeline_over_changing_sizes(gpu, oracle):
    """encode (held to the two-pass copy with 1 and 4 packets per wave and to the output-stationary
    copy) -> decode with compaction -> demux -> deliver -> control on one stream of one context, for
    n = 40000, 16384, 33000, 16385: each kind of scratch is reused by a smaller and then a larger batch
    (the output-stationary copy's ctl / bfirst words lie at 32 n, the tile sums and look-back words
    are counted by n, the compaction's epoch word runs on).  Every stage of every round is compared
    with its reference: the per-set kernel's bytes, the oracle's decode and demux, deliver_ref,
    control_ref."""
    from rsock_amd import codec as rc

    cx, ref_cx = new_codec(), new_codec()
    try:
        for k, n in enumerate(PIPE_SIZES):
            p = PipeCase(n, gpu, oracle, ref_cx)
            tab = C.table_on(rc, p.cols, 257, False, gpu, cx)
            for pk in PIPE_PATHS[k % 3:] + PIPE_PATHS[:k % 3]:  # another form first at every size
                with held(cx, *pk):
                    _pipeline_round(cx, gpu, p, tab, (n, pk))
    finally:
        cx.close()
        ref_cx.close()
