"""GPU: rsk_pool_add_batch, rsk_pool_offers, rsk_pool_settle_batch and rsk_pool_flush against their host twins and
the rules of tests/pool_ref.py: integer-exact outputs and tables, rsk_conn.h's contract on every index a call left
(tests/collide.index_invariant), sentinel-filled outputs (nothing behind a list's end is written).  The cases are
those of tests/test_pool_host.py; constructed collisions put all new tuples of a call into one index entry near the
end of the index (and of the add's dedup table), so the probes wrap; an add and a flush replay from a captured
graph on edited columns."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import codec as rc
from tests import collide
from tests import pool_ref as PR
from tests.pool_ref import CASES

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def libs(cx, gpu):
    return [PR.Lib(rc), PR.Lib(rc, gpu, cx)]


@pytest.mark.parametrize("n", PR.NS)
def test_sizes_device_equals_twin_and_rule(libs, n):
    """Every n with every capacity, fill and kind of batch: the cross tests/test_pool_host.py runs on the twin."""
    for cap in PR.CAPS:
        for fill in PR.FILLS:
            for kind in PR.KINDS:
                PR.property_case(libs, 31 * n + cap, n, cap, fill, kind)


@pytest.mark.parametrize("case", sorted(CASES))
def test_edges_device_equals_twin_and_rule(libs, case):
    kw, want = CASES[case]
    seen = PR.property_case(libs, 7, **kw)
    for k, v in want.items():
        assert seen[k] >= v, (case, k, seen)


@pytest.mark.parametrize("capacity", [67, 1025])
def test_all_new_tuples_in_one_entry_near_the_end(libs, capacity):
    """collide.tuples_at: every tuple of the case probes from entry S - 3 of every table, the pools' indexes and the
    add's dedup table alike, so every insert and every lookup walks one run that wraps."""
    seen = PR.property_case(libs, 11, 2 * capacity, capacity, "empty", "mixed", home=collide.WIDE - 3)
    assert seen["n_new"] == capacity and seen["n_full"] > 0 and seen["n_again"] > 0
    # the proof that the cluster is one: a pool filled by one add holds one run from S - 3
    lib = libs[1]
    uni = PR.universe(None, 40, home=collide.WIDE - 3)
    tab = lib.table(PR.empty(capacity, vals=False, rng=np.random.default_rng(3)))
    o = lib.add(tab, uni, 9, 40, False)
    assert o["n_new"] == 40 and o["row"].tolist() == o["new_rows"].tolist()
    collide.one_run(tab.column("index"), collide.conn_slots(capacity) - 3, 40)
    PR.index_check(tab, "one run")


def test_a_call_that_changes_nothing_writes_no_index_byte(libs):
    PR.nothing_changes_case(libs[1])


def test_invalid_arguments(cx, gpu):
    lib = PR.Lib(rc, gpu, cx)
    tab = lib.table(PR.empty(8))
    one = {f: np.ones(1, dt) for f, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
                                           ("seq", np.uint32), ("ack", np.uint32))}
    with pytest.raises(rc.RskError):
        lib.add(tab, one, 1, 0, True, work=tab.add_work(1))  # u_max 0
    with pytest.raises(rc.RskError):
        lib.add(tab, {k: v for k, v in one.items() if k != "seq"}, 1, 1, True)  # the pool has seq, the input not
    with pytest.raises(rc.RskError):
        lib.offers(tab, tab, 0)  # m_max 0
    with pytest.raises(rc.RskError):
        lib.offers(lib.table(PR.empty(8, vals=False)), tab, 4)  # an ack pool without seq / ack
    with pytest.raises(rc.RskError):
        cx.pool_flush(tab, 1, dead_rows=lib.fill(8))  # dead_rows without n_dead
    with pytest.raises(rc.RskError):
        cx.pool_settle_batch(tab, tab, tab.settle_work(tab)[1:], m_max=1)  # work not 16-B aligned


def test_add_and_flush_replay_from_a_captured_graph(gpu):
    """harvest -> flush on one pool, captured behind one eager run on a side stream of a fresh context after a
    reserve, replayed on edited rows: every replay equals the rule on the pool as the last one left it."""
    cxg = rc.Codec(KEY, 0)
    try:
        lib = PR.Lib(rc, gpu, cxg)
        rng = np.random.default_rng(5)
        n, cap = 2049, 1025
        uni = PR.universe(rng, 4 * cap)
        cols = PR.empty(cap, rng=np.random.default_rng(6))
        tab = lib.table(cols)
        stream = torch.cuda.Stream(gpu)
        cxg.reserve(n, stream=stream)
        t = {f: lib.t(np.zeros(n, dt)) for f, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
                                                      ("seq", np.uint32), ("ack", np.uint32), ("parse_status", np.int8))}
        work = tab.add_work(n)
        cnt, new_rows, dead = lib.fill(5), lib.fill(cap), lib.fill(cap)

        def run(s=None):
            cxg.pool_add_batch(tab, t["src"], t["dst"], t["sp"], t["dp"], 50, n, work, seq=t["seq"], ack=t["ack"],
                               parse_status=t["parse_status"], touch=True, new_rows=new_rows, n_new=cnt[0:1], n_again=cnt[1:2],
                               n_full=cnt[2:3], n_zero_port=cnt[3:4], stream=s)
            cxg.pool_flush(tab, 40, dead_rows=dead, n_dead=cnt[4:5], stream=s)

        graph = None
        for rnd in range(3):
            pick = rng.integers(0, len(uni["src"]), n)
            inp = {f: uni[f][pick].copy() for f in ("src", "dst", "sp", "dp")}
            inp["seq"], inp["ack"] = pick.astype(np.uint32), (pick * 3).astype(np.uint32)
            inp["sp"][::97] = 0
            status = np.where(rng.random(n) < 0.8, 2, 1).astype(np.int8)
            for f, v in dict(inp, parse_status=status).items():
                t[f].copy_(lib.t(v))
            # rows that the flush takes: the expiry of some LIVE rows set below now
            have = PR.Lib.columns(tab)
            old = np.nonzero(have["state"] & PR.LIVE)[0][::3]
            have["expiry"][old] = 40 - (old % 2)
            tab.load(expiry=have["expiry"])
            want, wo = PR.add_ref(dict(have, flag=np.zeros(cap, np.uint8)), inp, 50, n, True, status)
            want, wf = PR.flush_ref(want, 40)
            torch.cuda.synchronize()
            if graph is None:
                with torch.cuda.stream(stream):
                    run()
                torch.cuda.synchronize()
                keep = {k: getattr(tab, k).clone() for k, _ in PR.COLS}
                keep["index"] = tab.index.clone()
                got = PR._host(cnt, np.uint32).copy(), PR._host(new_rows, np.uint32).copy(), PR._host(dead, np.uint32).copy()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=stream):
                    run(torch.cuda.current_stream())
                for k, v in keep.items():
                    getattr(tab, k).copy_(v)
                torch.cuda.synchronize()
            else:
                graph.replay()
                torch.cuda.synchronize()
                got = PR._host(cnt, np.uint32).copy(), PR._host(new_rows, np.uint32).copy(), PR._host(dead, np.uint32).copy()
            c, nr, dr = got
            assert c.tolist() == [wo["n_new"], wo["n_again"], wo["n_full"], wo["n_zero_port"], wf["n_dead"]], (rnd, c)
            assert np.array_equal(nr[: wo["n_new"]], wo["new_rows"]) and np.array_equal(dr[: wf["n_dead"]], wf["dead_rows"])
            PR.same_columns(tab, want, f"round {rnd}")
            PR.index_check(tab, f"round {rnd}")
            assert rnd == 0 or wf["n_dead"] > 0
        del graph
    finally:
        cxg.close()
