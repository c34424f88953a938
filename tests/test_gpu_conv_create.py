"""GPU: rsk_conv_create_batch (include/rsk_codec.h) against tests/conv_create_ref: the scenarios of
tests/test_conv_create_host.py on the device (the reference's recorded SConn per packet out of one resolve ->
create, the index that survives the next batch, random equivalence with the host procedure, full tables, u_max
and repeated calls, skew, poisoned columns, optional outputs, argument checks, determinism), the chain in a
captured graph, two streams, and tables created on one side and used on the other."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import codec as rc
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


@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_reference_pin_server(cx, gpu, name):
    C.scenario_golden_server(rc, name, gpu, cx)


@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_survives_the_next_batch(cx, gpu, name):
    C.scenario_survives(rc, name, gpu, cx)


@pytest.mark.parametrize("capacity", C.CAPACITIES)
@pytest.mark.parametrize("n", C.SIZES)
def test_random_equivalence(cx, gpu, n, capacity):
    C.scenario_random(rc, n, capacity, True, True, gpu, cx)


@pytest.mark.parametrize("by_dst,by_id", R.FLAG_COMBOS)
@pytest.mark.parametrize("n,capacity", C.FLAG_POINTS)
def test_flag_combinations(cx, gpu, n, capacity, by_dst, by_id):
    C.scenario_random(rc, n, capacity, by_dst, by_id, gpu, cx)


@pytest.mark.parametrize("kind", ["fewer", "none", "cap1_vacant", "cap1_live"])
def test_table_full(cx, gpu, kind):
    C.scenario_full(rc, kind, gpu, cx)


@pytest.mark.parametrize("u_max", [1, 64, 65])
def test_u_max_repeated_calls(cx, gpu, u_max):
    C.scenario_u_max(rc, u_max, gpu, cx)


def test_u_max_until_full(cx, gpu):
    C.scenario_u_max_full(rc, gpu, cx)


@pytest.mark.parametrize("kind", ["one_key", "all_keys"])
def test_skew(cx, gpu, kind):
    C.scenario_skew(rc, kind, gpu, cx)


BAND_TABLES = {}


@pytest.mark.parametrize("pattern", R.BAND_PATTERNS)
@pytest.mark.parametrize("n", R.BAND_SIZES)
def test_counts_on_colliding_rows(cx, gpu, n, pattern):
    """The count pass of the create on 2048 distinct rows of one tile that share one run of its LDS table, on
    every row three times and on half a tile on one row: cur_in of the new convs is np.bincount."""
    assert C.scenario_band_create(rc, n, pattern, gpu, cx, cache=BAND_TABLES) > 600


def test_reads(cx, gpu):
    C.scenario_reads(rc, gpu, cx)


def test_optional_outputs(cx, gpu):
    C.scenario_optional_outputs(rc, gpu, cx)


def test_device_argument_errors(cx, gpu):
    C.check_einval(rc, gpu, cx)


def test_determinism(cx, gpu):
    C.scenario_determinism(rc, gpu, cx)


class Chain:
    """resolve -> create of one table over persistent columns, as a caller keeps them between batches."""

    def __init__(self, tab, n, device):
        e = lambda dt, k=n: torch.empty(k, dtype=dt, device=device)  # noqa: E731
        self.tab, self.n = tab, n
        self.t = {"status": e(torch.int8), "cmd": e(torch.uint8), "hit": e(torch.uint8), "conv": e(torch.int32),
                  "dst": e(torch.int32), "id": e(torch.uint8, 8 * n)}
        self.o = {"conv_row": e(torch.int32), "unknown": e(torch.int8), "n_unknown": e(torch.int32, 1),
                  "new_rows": e(torch.int32, min(n, tab.capacity)), "new_first": e(torch.int32, min(n, tab.capacity)),
                  "n_new": e(torch.int32, 1), "n_full": e(torch.int32, 1)}
        self.work = tab.create_work(n)

    def load(self, c):
        for k, v in self.t.items():
            v.copy_(R.tensor(c[k], v.device))
        for v in self.o.values():
            v.view(torch.uint8).fill_(R.SENT)

    def run(self, codec, stream=None):
        t, o = self.t, self.o
        codec.conv_resolve_batch(self.tab, t["status"], t["conv"], o["conv_row"], cmd=t["cmd"], hit=t["hit"], id=t["id"],
                                 dst=t["dst"], unknown=o["unknown"], stream=stream)
        codec.conv_create_batch(self.tab, t["conv"], o["conv_row"], o["unknown"], self.n, self.work, id=t["id"], dst=t["dst"],
                                n_unknown=o["n_unknown"], new_rows=o["new_rows"], new_first=o["new_first"], n_new=o["n_new"],
                                n_full=o["n_full"], stream=stream)

    def result(self):
        got = {k: u32(self.o[k])[0] for k in ("n_unknown", "n_new", "n_full")}
        got["conv_row"], got["unknown"] = u32(self.o["conv_row"]), self.o["unknown"].cpu().numpy()
        for k in ("new_rows", "new_first"):
            got[k] = u32(self.o[k])
        got.update({"tab." + k: v for k, v in C.table_columns(self.tab).items()})
        return got


def same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_resolve_create_in_captured_graph(cx, gpu):
    """resolve -> create captured on a side stream of a fresh context after a reserve; replayed on the first
    batch, on new column contents, and after a host-side close plus rebuild: every output and table column
    equals the eager chain's on a twin table."""
    rng = np.random.default_rng(91)
    n, cap = 5000, 3000
    cols, c1 = R.random_case(rng, n, cap, True, True, known=0.5, live=0.3, pool=150, ctl=False)
    _cols2, c2 = R.random_case(rng, n, cap, True, True, known=0.5, live=0.3, pool=150, ctl=False)
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
        born = []
        for step, c in enumerate((c1, c2, c1)):
            if step == 2:  # the host closes convs: clear LIVE, rebuild; the batch that made them makes them again
                closed = torch.from_numpy(born[0][:len(born[0]) // 2].astype(np.int64)).to(gpu)
                assert len(closed) > 10
                for ch in (eager, graph):
                    ch.tab.state[closed] = 0
                    ch.tab.rebuild(cx)
            eager.load(c)
            graph.load(c)
            eager.run(cx)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            a, b = eager.result(), graph.result()
            same(a, b)
            assert a["n_new"] > 10, step
            born.append(a["new_rows"][:a["n_new"]])
            if step == 0:
                want = R.resolve_ref(cols, True, True, c)
                ref = C.create_ref(dict(cols, cur_in=cols["cur_in"] + want["add"]), True, True, c, want["conv_row"],
                                   want["unknown"], n)
                assert np.array_equal(b["conv_row"], ref["conv_row"]) and b["n_new"] == ref["n_new"] and b["n_full"] == ref["n_full"]
                C.compare_table(graph.tab, ref["cols"])
        assert len(born[2]) == len(born[0]) // 2  # the closed convs, and nothing else, were born again
        del g
    finally:
        cxg.close()


def test_two_streams(cx, gpu):
    """The call on two streams at once, each with its own table and work buffer."""
    rng = np.random.default_rng(93)
    n, cap = 9000, 1200
    chains, refs = [], []
    for _ in range(2):
        cols, c = R.random_case(rng, n, cap, True, True, known=0.5, live=0.4, pool=300, ctl=False)
        ch = Chain(R.make_table(rc, cols, gpu, True, True, cx), n, gpu)
        ch.load(c)
        chains.append(ch)
        want = R.resolve_ref(cols, True, True, c)
        refs.append(C.create_ref(dict(cols, cur_in=cols["cur_in"] + want["add"]), True, True, c, want["conv_row"],
                                 want["unknown"], n))
    streams = [torch.cuda.Stream(gpu) for _ in chains]
    torch.cuda.synchronize()
    for _rep in range(2):
        for ch, s in zip(chains, streams):
            with torch.cuda.stream(s):
                ch.run(cx)
    torch.cuda.synchronize()
    for ch, ref in zip(chains, refs):
        got = ch.result()
        # the second run found every key of the first: only its cur_in counts came on top
        assert got["n_new"] == 0 and got["n_unknown"] == ref["n_unknown"] and np.array_equal(got["conv_row"], ref["conv_row"])
        for k in ("state", "conv", "dst", "id"):
            assert np.array_equal(got["tab." + k], ref["cols"][k]), k
    for s in streams:
        cx.release_stream(s)


@pytest.mark.parametrize("by_dst,by_id", [(False, False), (True, True)])
def test_created_on_either_side(cx, gpu, by_dst, by_id):
    """A table created on the host twin and copied to the device resolves the same there, and the reverse."""
    rng = np.random.default_rng(97)
    cols, c = R.random_case(rng, 6000, 3000, by_dst, by_id, known=0.5, live=0.5, pool=1500)
    _g, ref, host_tab, _b = C.resolve_create(rc, cols, c, by_dst, by_id, "cpu")
    _g, ref_d, dev_tab, _b = C.resolve_create(rc, cols, c, by_dst, by_id, gpu, cx)
    assert ref["n_new"] == ref_d["n_new"] > 100
    want = R.resolve_ref(ref["cols"], by_dst, by_id, c)
    assert want["n_unknown"] == ref["n_unknown"]
    for tab, side in ((host_tab.to(gpu), cx), (dev_tab.to("cpu"), None)):
        got = R.run_resolve(rc, tab, c, gpu if side else "cpu", side, msg_mode="none")
        assert np.array_equal(got["conv_row"], want["conv_row"]) and got["n_unknown"] == want["n_unknown"]
        C.check_lookups(rc, tab, ref["cols"], by_dst, by_id, gpu if side else "cpu", side)
