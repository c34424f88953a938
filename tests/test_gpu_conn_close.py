"""GPU: rsk_conn_close_batch (include/rsk_codec.h) against tests/conn_close_ref: the scenarios of
tests/test_conn_close_host.py on the device (capacities at the tile edges with every closing pattern in both
forms, the list form's edges, SWEEP, sequences on one pick index, emptied groups and probe chains, the reference's
recorded control walk, keepalive timer and doSend, argument checks), the column-form chain control -> conn_close
-> pick in a captured graph, two streams, and tables closed on one side and used on the other."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_close_ref as K
from tests import control_golden as G
from tests import control_ref as C
from tests import pick_ref as P

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", K.CAPACITIES)
def test_patterns(cx, gpu, capacity, by_id):
    assert K.scenario_patterns(rc, capacity, by_id, gpu, cx) > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [2, 257, 1025])
def test_list_edges(cx, gpu, capacity, by_id):
    K.scenario_list_edges(rc, capacity, by_id, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1, 257, 4097])
def test_sweep(cx, gpu, capacity, by_id):
    K.scenario_sweep(rc, capacity, by_id, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [2, 1025, 4097])
def test_sequences(cx, gpu, capacity, by_id):
    K.scenario_sequences(rc, capacity, by_id, gpu, cx)


@pytest.mark.parametrize("capacity", [64, 257])
def test_emptied_group_keeps_probe_chains(cx, gpu, capacity):
    K.scenario_probe_chains(rc, capacity, gpu, cx)


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", K.COLLIDE_LENGTHS)
def test_constructed_cluster(cx, gpu, capacity, by_id, wrap):
    """A full table that is one run of the index (and of the pick's group entries, tests/collide.py): every second row
    closed without and with REMOVE, then the rest; groups of one pick home emptied one by one."""
    assert K.scenario_collide_close(rc, capacity, by_id, wrap, gpu, cx) == capacity


@pytest.mark.parametrize("name", K.WALK_CASES)
def test_reference_pin_walk(cx, gpu, name):
    K.scenario_walk_golden(rc, name, gpu, cx)


@pytest.mark.parametrize("name", K.TIMER_CASES)
def test_reference_pin_timer(cx, gpu, name):
    K.scenario_timer_golden(rc, name, gpu, cx)


@pytest.mark.parametrize("name", K.SEND_CASES)
def test_reference_pin_send(cx, gpu, name):
    K.scenario_send_golden(rc, name, gpu, cx)


def test_device_argument_errors(cx, gpu):
    K.check_einval(rc, gpu, cx)


IN_COLS = (("status", np.int8), ("cmd", np.uint8), ("id", np.uint8), ("conn_key", np.int64), ("pay_off", np.int16),
           ("pay_len", np.int16), ("arena", np.uint8), ("base_off", np.int64), ("inner_off", np.int16))


class Chain:
    """control -> conn_close (column form, with pick) -> pick for the messages, over persistent columns as a caller
    keeps them between batches: a linear chain."""

    def __init__(self, h, b):
        dev, cap = h.device, h.cap
        self.h, self.n = h, len(b["status"])
        self.t = {k: C.tensor(b[k], dev, dt) for k, dt in IN_COLS}
        self.out = rc.ControlBuffers.alloc(self.n, dev, capacity=cap)
        self.out.dead_rows = self.out.n_dead = None
        e = lambda k: torch.empty(k, dtype=torch.int32, device=dev)  # noqa: E731
        self.o = {"marked_rows": e(cap), "n_marked": e(1), "closed_rows": e(cap), "n_closed": e(1), "pick_counts": e(2),
                  "conn": e(self.n), "n_none": e(1)}

    def load(self, b):
        for k, dt in IN_COLS:
            self.t[k].copy_(C.tensor(b[k], self.t[k].device, dt))
        for v in list(self.o.values()) + [getattr(self.out, f) for f in self.out.__dataclass_fields__]:
            if v is not None:
                v.view(torch.uint8).fill_(K.SENT)

    def run(self, codec, stream=None):
        t, o, out, tab = self.t, self.o, self.out, self.h.tab
        codec.control_batch(tab, t["status"], t["cmd"], t["pay_off"], t["pay_len"], t["arena"], t["base_off"], out,
                            id=t["id"], conn_key=t["conn_key"], inner_off=t["inner_off"], stream=stream)
        codec.conn_close_batch(tab, self.h.work, rst_first=out.rst_first, pick=True, marked_rows=o["marked_rows"],
                               n_marked=o["n_marked"], closed_rows=o["closed_rows"], n_closed=o["n_closed"],
                               pick_counts=o["pick_counts"], stream=stream)
        codec.conn_pick_batch(tab, o["conn"], id=out.msg_id if self.h.by_id else None, avoid_key=out.msg_avoid_key,
                              seed=0x5EED, n_none=o["n_none"], stream=stream)

    def result(self):
        got = {k: v.cpu().numpy().view(np.uint32).copy() for k, v in self.o.items()}
        got["rst_first"] = self.out.rst_first.cpu().numpy().view(np.uint32).copy()
        got["n_msg"] = self.out.n_msg.cpu().numpy().view(np.uint32).copy()
        got["state"] = self.h.tab.state.cpu().numpy().copy()
        return got


def walk_batch(name):
    c = G.case("walk", name)
    n = len(c["cmd"])
    cols, _cap, _row = G.walk_table(c)
    b = dict(status=c["status"].copy(), cmd=c["cmd"], id=np.tile(np.ascontiguousarray(c["id"], np.uint8), n),
             conn_key=c["pool"][c["ck"]])
    b.update(G.frames(c))
    return cols, b, int(c["shape"]) == G.SERVER


@pytest.mark.parametrize("name", ["server_4097", "client_2048"])
def test_chain_in_captured_graph(cx, gpu, name):
    """control -> conn_close -> pick captured on a side stream of a fresh context after a reserve; replayed on the
    first batch, on a second rst_first (half of the resets dropped) with the table as the first left it, and after
    a host revival of every row plus both rebuilds: outputs and state equal the eager chain's on a twin table and
    the restatement's, and both tables look up and pick as their state says."""
    cols, b1, by_id = walk_batch(name)
    b2 = dict(b1, status=b1["status"].copy())
    rst = np.nonzero((b1["status"] == A.RECV_VALID) & (b1["cmd"] == A.CMD_NETCONN_RST))[0]
    b2["status"][rst[::2]] = A.RECV_DROP
    eager = Chain(K.Harness(rc, cols, by_id, gpu, cx), b1)
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        cxg.reserve(eager.n, stream=s)
        graph = Chain(K.Harness(rc, cols, by_id, gpu, cx), b1)
        graph.load(b1)
        with torch.cuda.stream(s):
            graph.run(cxg)  # the eager call: loads the kernels and runs the chain once
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            graph.run(cxg, torch.cuda.current_stream())
        graph.h.host_edit(cols["state"])  # the table as it was before the warm-up call and the capture
        marked_total = 0
        for step, b in enumerate((b2, b1, b1)):
            if step == 2:  # the host revives every row and rebuilds both indexes
                for ch in (eager, graph):
                    ch.h.host_edit(cols["state"])
                    ch.h.killed.clear()
            before = eager.h.cols["state"]
            eager.load(b)
            graph.load(b)
            eager.run(cx)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            x, y = eager.result(), graph.result()
            assert x.keys() == y.keys()
            for k in x:
                assert np.array_equal(x[k], y[k]), (step, k)
            ref = K.close_ref(before, x["rst_first"] != K.NO_RST)
            k = len(ref["marked_rows"])
            marked_total += k
            assert x["n_marked"][0] == k and np.array_equal(x["marked_rows"][:k], ref["marked_rows"]) and x["n_closed"][0] == 0
            assert np.array_equal(x["state"], ref["state"])
            sent = x["conn"][: x["n_msg"][0]]
            sent = sent[sent != K.NONE].astype(np.int64)
            assert bool((x["rst_first"][sent] == K.NO_RST).all()) and bool(((ref["state"][sent] & K.UP) == K.UP).all())
            for ch in (eager, graph):
                ch.h.cols["state"] = ref["state"]
                ch.h.killed |= set(ref["marked_rows"].tolist())
                ch.h.check_lookups()
                ch.h.check_picks()
            if step == 0:
                assert 0 < k < len(rst)
            elif step == 1:
                assert k > 0  # the resets the second batch dropped
        assert marked_total > 20
        del g
    finally:
        cxg.close()


def test_two_streams(cx, gpu):
    """The list form with REMOVE and pick on two streams at once, each with its own table and work buffer."""
    hs, lists, outs = [], [], []
    for j, by_id in enumerate((False, True)):
        h = K.Harness(rc, K.grouped_table(65536, by_id, seed=20 + j), by_id, gpu, cx)
        rows = np.random.default_rng(j).integers(0, h.cap, h.cap // 3).astype(np.uint32)
        hs.append(h)
        lists.append((P.tensor(rows, gpu), P.tensor(np.array([len(rows)], np.uint32), gpu), rows))
        outs.append({k: K.filled(h.cap if k.endswith("rows") else 2, torch.int32, gpu)
                     for k in ("marked_rows", "n_marked", "closed_rows", "n_closed", "pick_counts")})
    streams = [torch.cuda.Stream(gpu) for _ in hs]
    torch.cuda.synchronize()
    for h, (lst, cnt, _r), o, s in zip(hs, lists, outs, streams):
        with torch.cuda.stream(s):
            cx.conn_close_batch(h.tab, h.work, close_rows=lst, n_close=cnt, remove=True, pick=True, **o)
    torch.cuda.synchronize()
    for h, (_l, _c, rows), o in zip(hs, lists, outs):
        ref = K.close_ref(h.cols["state"], K.list_marks(h.cap, rows, len(rows), len(rows)), remove=True)
        for lst, cnt in (("marked_rows", "n_marked"), ("closed_rows", "n_closed")):
            k = len(ref[lst])
            assert K.host(o[cnt], np.uint32)[0] == k > 100 and np.array_equal(K.host(o[lst], np.uint32)[:k], ref[lst])
        h.cols["state"] = ref["state"]
        h.killed |= set(ref["marked_rows"].tolist())
        h.removed |= set(ref["closed_rows"].tolist())
        h.compare_columns()
        h.check_lookups()
        h.check_picks()
    for s in streams:
        cx.release_stream(s)


@pytest.mark.parametrize("by_id", [False, True])
def test_closed_on_either_side(cx, gpu, by_id):
    """A table closed by the host twin and copied to the device looks up and picks there as its state says, and is
    closed further there; and the reverse."""
    cols = K.grouped_table(4097, by_id, seed=30)
    rng = np.random.default_rng(31)
    first = rng.integers(0, 4097, 1500).astype(np.uint32)
    second = K.as_column(4097, np.nonzero(rng.random(4097) < 0.3)[0])
    for sides in ((("cpu", None), (gpu, cx)), ((gpu, cx), ("cpu", None))):
        a = K.Harness(rc, cols, by_id, *sides[0])
        assert len(a.close(close_rows=first, remove=True)["closed_rows"]) > 100
        b = a.moved(*sides[1])
        b.check_picks()
        b.check_lookups()
        assert len(b.close(rst_first=second, sweep=True)["marked_rows"]) > 100
