"""GPU: rsk_conv_close_batch (include/rsk_codec.h) against tests/conv_close_ref: the scenarios of
tests/test_conv_close_host.py on the device (the reference's recorded flush -> close rounds, the timer form on
random lists, resolve -> create -> close (HOLD) -> create against the per-packet walk, the specified deviations,
HOLD against not HOLD, calls that close nothing, skew, poisoned columns, optional outputs, argument checks), the
two chains in a captured graph, two streams, and tables closed on one side and used on the other."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import codec as rc
from tests import conv_close_ref as K
from tests import conv_create_ref as C
from tests import conv_ref as R

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", K.FLUSH_CASES)
def test_reference_pin_flush_close(cx, gpu, name):
    assert K.scenario_flush_golden(rc, name, gpu, cx)["closed"] > 0


@pytest.mark.parametrize("length,shape,flags,wrap", K.INDEX_CLUSTERS)
def test_constructed_cluster_index(cx, gpu, length, shape, flags, wrap):
    """The conn index's cluster families for the conv table's key forms (tests/collide.py; the client's conv-only keys
    by search): a full table that is one run of the index, two interleaved homes, duplicates inside the run (the
    lowest row wins, n_dup), absent keys of the same and of the neighbouring homes."""
    assert K.scenario_cluster_index(rc, length, shape, flags[0], flags[1], wrap, gpu, cx) > length // 2


@pytest.mark.parametrize("capacity,flags,wrap", K.LIFE_CLUSTERS)
def test_constructed_cluster(cx, gpu, capacity, flags, wrap):
    """A create that fills the table (a run as long as the table has rows), the list-form close of every second row,
    a create in place into the index as the close left it, a close under HOLD (BY_DST), then the rest: on a conv table
    whose keys all probe from one entry of the index, across the index's end or not."""
    assert K.scenario_cluster(rc, capacity, flags[0], flags[1], wrap, gpu, cx) > capacity // 2


@pytest.mark.parametrize("by_dst,by_id", R.FLAG_COMBOS)
@pytest.mark.parametrize("capacity", K.CAPACITIES)
def test_timer_random(cx, gpu, capacity, by_dst, by_id):
    K.scenario_timer_random(rc, capacity, by_dst, by_id, gpu, cx)


@pytest.mark.parametrize("capacity", K.CAPACITIES)
@pytest.mark.parametrize("n", K.SIZES)
def test_receive_against_walk(cx, gpu, n, capacity):
    K.scenario_walk(rc, n, capacity, True, gpu, cx)


def test_receive_against_walk_without_ids(cx, gpu):
    out, _w = K.scenario_walk(rc, 4097, 1025, False, gpu, cx)
    assert out["cl"]["n_closed"] > 10 and out["cl"]["n_reopened"] > 10


@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_receive_against_walk_golden(cx, gpu, name, seed):
    K.scenario_walk_golden(rc, name, seed, gpu, cx)


def test_deviations(cx, gpu):
    K.scenario_deviations(rc, gpu, cx)


def test_hold_against_plain(cx, gpu):
    K.scenario_hold(rc, gpu, cx)


def test_nothing_to_close(cx, gpu):
    K.scenario_nothing(rc, gpu, cx)


@pytest.mark.parametrize("kind", ["one_conv", "every_row", "edges"])
def test_skew(cx, gpu, kind):
    K.scenario_skew(rc, kind, gpu, cx)


def test_reads(cx, gpu):
    K.scenario_reads(rc, gpu, cx)


def test_optional_outputs(cx, gpu):
    K.scenario_optional_outputs(rc, gpu, cx)


def test_device_argument_errors(cx, gpu):
    K.check_einval(rc, gpu, cx)


class Chain:
    """flush -> close, then resolve -> create -> close (HOLD) -> create, of one table over persistent columns, as
    a caller keeps them between batches."""

    def __init__(self, tab, n, device):
        e = lambda dt, k=n: torch.empty(k, dtype=dt, device=device)  # noqa: E731
        cap = tab.capacity
        self.tab, self.n = tab, n
        self.t = {"status": e(torch.int8), "cmd": e(torch.uint8), "conv": e(torch.int32), "dst": e(torch.int32),
                  "id": e(torch.uint8, 8 * n), "ctl_kind": e(torch.uint8), "ctl_arg": e(torch.int64)}
        self.o = {"conv_row": e(torch.int32), "unknown": e(torch.int8), "n_unknown": e(torch.int32, 1),
                  "rst_first": e(torch.int32, cap), "new_rows": e(torch.int32, min(n, cap)), "n_new": e(torch.int32, 1),
                  "n_full": e(torch.int32, 1), "new_rows2": e(torch.int32, min(n, cap)), "n_new2": e(torch.int32, 1),
                  "closed_rows": e(torch.int32, cap), "closed_at": e(torch.int32, cap), "n_closed": e(torch.int32, 1),
                  "n_reopened": e(torch.int32, 1), "n_rst_again": e(torch.int32, 1), "dead_rows": e(torch.int32, cap),
                  "n_dead": e(torch.int32, 1), "timer_rows": e(torch.int32, cap), "n_timer": e(torch.int32, 1)}
        self.work, self.close_work = tab.create_work(n), tab.close_work()

    def load(self, c):
        for k, v in self.t.items():
            v.copy_(R.tensor(c[k], v.device))
        for v in self.o.values():
            v.view(torch.uint8).fill_(R.SENT)

    def run(self, codec, stream=None):
        t, o, tab = self.t, self.o, self.tab
        # the timer's chain: the convs that the flush lists close with no host step
        codec.conv_flush(tab, dead_rows=o["dead_rows"], n_dead=o["n_dead"], stream=stream)
        codec.conv_close_batch(tab, close_rows=o["dead_rows"], n_close=o["n_dead"], work=self.close_work,
                               closed_rows=o["timer_rows"], n_closed=o["n_timer"], stream=stream)
        # the receive chain; the rows it holds stay LIVE until host_clear
        codec.conv_resolve_batch(tab, t["status"], t["conv"], o["conv_row"], cmd=t["cmd"], id=t["id"], dst=t["dst"],
                                 ctl_kind=t["ctl_kind"], ctl_arg=t["ctl_arg"], unknown=o["unknown"], rst_first=o["rst_first"],
                                 stream=stream)
        codec.conv_create_batch(tab, t["conv"], o["conv_row"], o["unknown"], self.n, self.work, id=t["id"], dst=t["dst"],
                                n_unknown=o["n_unknown"], new_rows=o["new_rows"], n_new=o["n_new"], stream=stream)
        codec.conv_close_batch(tab, rst_first=o["rst_first"], ctl_kind=t["ctl_kind"], conv_row=o["conv_row"],
                               unknown=o["unknown"], n_unknown=o["n_unknown"], hold=True, closed_rows=o["closed_rows"],
                               closed_at=o["closed_at"], n_closed=o["n_closed"], n_reopened=o["n_reopened"],
                               n_rst_again=o["n_rst_again"], stream=stream)
        codec.conv_create_batch(tab, t["conv"], o["conv_row"], o["unknown"], self.n, self.work, id=t["id"], dst=t["dst"],
                                n_unknown=o["n_unknown"], new_rows=o["new_rows2"], n_new=o["n_new2"], n_full=o["n_full"],
                                stream=stream)

    def result(self):
        got = {k: u32(v).copy() for k, v in self.o.items() if k != "unknown"}
        got["unknown"] = self.o["unknown"].cpu().numpy()
        for cnt, lst in (("n_new", "new_rows"), ("n_new2", "new_rows2"), ("n_closed", "closed_rows"), ("n_closed", "closed_at"),
                         ("n_dead", "dead_rows"), ("n_timer", "timer_rows")):
            got[lst] = got[lst][:got[cnt][0]]
        got.update({"tab." + k: v for k, v in C.table_columns(self.tab).items()})
        return got

    def host_clear(self, rows):
        """After the batch: the host clears LIVE for the rows the HOLD close listed; no rebuild."""
        self.tab.state[torch.from_numpy(rows.astype(np.int64)).to(self.tab.state.device)] &= 0xFE


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def chain_case(rng, n, cap):
    """A table and a batch over it with resets, reborn convs and new convs; a fifth of the rows not alive."""
    cols, c = K.recv_case(rng, n, cap, live=0.5, resets=0.2, noise=0.05)
    cols["alive"][:] = rng.random(cap) > 0.2
    return cols, c


def test_chains_in_captured_graph(cx, gpu):
    """resolve -> create -> close -> create and flush -> close captured on a side stream of a fresh context after
    a reserve; replayed on the first batch and on new column contents: every output and table column equals the
    eager chain's on a twin table, and the two tables resolve alike (lookups, not index bytes)."""
    rng = np.random.default_rng(1101)
    n, cap = 5000, 3000
    cols, c1 = chain_case(rng, n, cap)
    # a second batch over the same keys: the first batch's packets in another order
    perm = rng.permutation(n)
    c2 = {k: (None if v is None else (v.reshape(n, -1)[perm].reshape(v.shape))) for k, v in c1.items()}
    eager = Chain(R.make_table(rc, cols, gpu, True, True, cx), n, gpu)
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        cxg.reserve(n, stream=s)
        graph = Chain(R.make_table(rc, cols, gpu, True, True, cx), n, gpu)
        graph.load(c1)
        with torch.cuda.stream(s):
            graph.run(cxg)  # the eager call: loads the kernels and runs the chain once
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            graph.run(cxg, torch.cuda.current_stream())
        # the table as it was before the warm-up call
        graph.tab.load(**{k: v for k, v in cols.items() if v is not None})
        graph.tab.rebuild(cx)
        torch.cuda.synchronize()
        for step, c in enumerate((c1, c2)):
            eager.load(c)
            graph.load(c)
            eager.run(cx)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            a, b = eager.result(), graph.result()
            same(a, b)
            if step == 0:
                assert len(a["closed_rows"]) > 10 and a["n_reopened"][0] > 10 and len(a["timer_rows"]) > 10
            assert np.array_equal(a["timer_rows"], a["dead_rows"])
            for ch in (eager, graph):
                ch.host_clear(a["closed_rows"])
            after = C.table_columns(eager.tab)
            for ch in (eager, graph):
                K.check_lookups(rc, ch.tab, after, after["state"], True, True, gpu, cx)
        del g
    finally:
        cxg.close()


def test_two_streams(cx, gpu):
    """The chains on two streams at once, each with its own table and work buffers."""
    rng = np.random.default_rng(1103)
    n, cap = 9000, 1500
    chains, refs = [], []
    for _ in range(2):
        cols, c = chain_case(rng, n, cap)
        ch = Chain(R.make_table(rc, cols, gpu, True, True, cx), n, gpu)
        ch.load(c)
        chains.append(ch)
        one = Chain(R.make_table(rc, cols, gpu, True, True, cx), n, gpu)
        one.load(c)
        one.run(cx)
        torch.cuda.synchronize()
        refs.append(one.result())
    streams = [torch.cuda.Stream(gpu) for _ in chains]
    torch.cuda.synchronize()
    for ch, s in zip(chains, streams):
        with torch.cuda.stream(s):
            ch.run(cx)
    torch.cuda.synchronize()
    for ch, ref in zip(chains, refs):
        same(ch.result(), ref)
        assert len(ref["closed_rows"]) > 10 and len(ref["timer_rows"]) > 10
    for s in streams:
        cx.release_stream(s)


@pytest.mark.parametrize("by_id", [False, True])
def test_closed_on_either_side(cx, gpu, by_id):
    """A table closed on the host twin and copied to the device resolves the same there, and the reverse."""
    rng = np.random.default_rng(1105)
    cols, c = K.recv_case(rng, 6000, 3000, by_id)
    host = K.run_chain(rc, cols, c, by_id, "cpu")
    dev = K.run_chain(rc, cols, c, by_id, gpu, cx)
    assert host["cl"]["n_closed"] == dev["cl"]["n_closed"] > 20
    for k in ("conv_row", "unknown"):
        assert np.array_equal(host["cr2"][k], dev["cr2"][k]), k
    after = C.table_columns(host["tab"])
    C.compare_table(dev["tab"], after)
    look = after["state"].copy()
    look[host["cl"]["closed_rows_all"][:host["cl"]["n_closed"]].astype(np.int64)] &= 0xFE  # held: gone from the index
    for tab, side in ((host["tab"].to(gpu), cx), (dev["tab"].to("cpu"), None)):
        K.check_lookups(rc, tab, after, look, True, by_id, gpu if side else "cpu", side)
