"""GPU: rsk_conn_create_batch (include/rsk_codec.h) against tests/conn_create_ref: the scenarios of
tests/test_conn_create_host.py on the device (tile-edge capacities and batch sizes, the patterns, groups that grow
and are reborn, the repeat loop, the list form, the tcpstate pin, the equivalence with the host procedure,
sequences with closes, argument checks), the device bytewise against the host twin, tables created on one side and
continued on the other, the receive chain resolve -> create -> recv_ack -> control -> conn_close -> pick in one
captured graph, and two streams."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_close_ref as K
from tests import conn_create_ref as R
from tests import conn_ref as CR
from tests import pick_ref as P
from tests import tcpstate_golden as T

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", R.GPU_CAPACITIES)
def test_capacities(cx, gpu, capacity, by_id):
    R.scenario_sizes(rc, capacity, 700, by_id, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("n", R.SIZES)
def test_batch_sizes(cx, gpu, n, by_id):
    assert (R.scenario_sizes(rc, 1025, n, by_id, gpu, cx) > 0) == (n > 0)


@pytest.mark.parametrize("by_id", [False, True])
def test_large_table_once(cx, gpu, by_id):
    assert R.scenario_sizes(rc, 65536, 6000, by_id, gpu, cx) > 1000


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1, 2, 257, 1025])
def test_patterns(cx, gpu, capacity, by_id):
    R.scenario_patterns(rc, capacity, by_id, gpu, cx)


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity,live0,k", R.COLLIDE_CASES)
def test_constructed_cluster(cx, gpu, capacity, live0, k, by_id, wrap):
    """Hundreds of lanes of one launch insert into ONE run of the index, of the dedup table, of the offers table and
    of the pick's group entries (keys, 4-tuples and ids built to probe from one entry, tests/collide.py), across the
    tables' ends; the index keeps rsk_conn.h's contract after every call."""
    assert R.scenario_collide(rc, capacity, live0, k, by_id, wrap, gpu, cx) > capacity // 2


@pytest.mark.parametrize("capacity", [257, 1025])
def test_constructed_cluster_of_new_groups(cx, gpu, capacity):
    """70 new groups of one pick home born in one call: the claim of taken-off and emptied group entries."""
    assert R.scenario_collide_groups(rc, capacity, gpu, cx) == 70


@pytest.mark.parametrize("by_id", [False, True])
def test_groups_grow_and_are_reborn(cx, gpu, by_id):
    assert R.scenario_groups(rc, by_id, gpu, cx) > 100


@pytest.mark.parametrize("capacity", [2, 257])
def test_idbuf_churn_beyond_the_group_entries(cx, gpu, capacity):
    assert R.scenario_churn(rc, capacity, gpu, cx) > 0


@pytest.mark.parametrize("by_id", [False, True])
def test_repeat_loop_reaches_the_one_call_result(cx, gpu, by_id):
    R.scenario_repeat(rc, 4097, by_id, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1, 257, 1025])
def test_list_form(cx, gpu, capacity, by_id):
    R.scenario_list(rc, capacity, by_id, gpu, cx)


def test_rows_hold_the_recorded_init_state(cx, gpu):
    for name in T.names()[:3]:
        assert R.scenario_tcpstate(rc, name, gpu, cx) > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity,seed", [(257, 0), (4097, 2)])
def test_equivalence_with_the_host_procedure(cx, gpu, capacity, seed, by_id):
    assert R.scenario_equivalence(rc, capacity, by_id, gpu, cx, seed=seed) > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [2, 1025])
def test_sequences(cx, gpu, capacity, by_id):
    assert R.scenario_sequences(rc, capacity, by_id, gpu, cx) > 0


def test_device_argument_errors(cx, gpu):
    R.check_einval(rc, gpu, cx)


@pytest.mark.parametrize("by_id", [False, True])
def test_device_equals_host_twin_bytewise(cx, gpu, by_id):
    """One column-form and one list-form call on both sides: every output and every table column bytewise."""
    rng = np.random.default_rng(40 + by_id)
    cols = R.table(4097, by_id, seed=9)
    nc = R.new_conns(rng, cols, by_id, 300)
    b = R.batch_of(rng, cols, by_id, nc, 5000)
    of = R.offers_of(nc, rng.permutation(300)[:250])
    lst = R.offers_of(R.new_conns(np.random.default_rng(3), cols, by_id, 40), list_form=True)
    lst["conn_key"] += np.uint64(777)
    sides = [R.Harness(rc, cols, by_id, "cpu"), R.Harness(rc, cols, by_id, gpu, cx)]
    tmap, _ = CR.table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)
    conn, hit, miss, _ = CR.resolve_ref(tmap, np.full(5000, R.VALID, np.int8), b["conn_key"], id=b["id"] if by_id else None)
    outs = []
    for h in sides:
        o1 = h.raw_create(of, 250, 250, b, conn, hit, miss, u_max=5000)
        o2 = h.raw_create(lst, 40, 40, list_form=True)
        outs.append((o1, o2))
    for x, y in zip(outs[0], outs[1]):
        assert x.keys() == y.keys()
        for k in x:
            assert (x[k] is None and y[k] is None) or np.array_equal(x[k], y[k]), k
    assert outs[0][0]["n_new"][0] == 250 and outs[0][1]["n_new"][0] == 40
    for name, _dt, _k in rc._CONN_COLUMNS:
        a, d = getattr(sides[0].tab, name), getattr(sides[1].tab, name)
        assert (a is None and d is None) or bool((a == d.cpu()).all()), name
    assert np.array_equal(K.host(sides[0].t_est, np.uint64), K.host(sides[1].t_est, np.uint64))


@pytest.mark.parametrize("by_id", [False, True])
def test_created_on_either_side(cx, gpu, by_id):
    for sides in ((("cpu", None), (gpu, cx)), ((gpu, cx), ("cpu", None))):
        assert R.scenario_moved(rc, 4097, by_id, sides) > 40


# ---- the receive chain in one graph -----------------------------------------------------------------------------
CHAIN_COLS = (("status", np.int8), ("cmd", np.uint8), ("id", np.uint8), ("conn_key", np.uint64), ("src", np.uint32),
              ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16), ("seq", np.uint32), ("arena", np.uint8),
              ("base_off", np.uint64), ("pay_off", np.uint16), ("pay_len", np.uint16))
N_CHAIN, M_CHAIN = 3000, 64


def chain_batch(rng, cols, by_id, nc, resets):
    """DATA packets of known and new conns, and NETCONN_RST packets whose 8-byte bodies name `resets` LIVE rows."""
    n = N_CHAIN
    b = R.batch_of(rng, cols, by_id, nc, n, known=0.6)
    b["status"] = np.full(n, R.VALID, np.int8)
    b["cmd"] = np.full(n, A.CMD_DATA, np.uint8)
    at = rng.permutation(np.nonzero(b["which"] < 0)[0])[: len(resets)]
    body = np.zeros(n, np.uint64)
    w = CR.id_words(cols["id"] if by_id else None, len(cols["state"]))
    for i, r in zip(at.tolist(), resets.tolist()):
        b["cmd"][i] = A.CMD_NETCONN_RST
        body[i] = cols["conn_key"][r]
        if by_id:
            b["id"].reshape(-1, 8)[i] = np.array([w[r]], np.uint64).view(np.uint8)
    b.update(seq=rng.integers(0, 2**32, n).astype(np.uint32), arena=body.view(np.uint8), base_off=np.arange(n, dtype=np.uint64) * 8,
             pay_off=np.zeros(n, np.uint16), pay_len=np.full(n, 8, np.uint16))
    if not by_id:
        b["id"] = np.zeros(8 * n, np.uint8)
    return b


class Chain:
    """resolve -> create -> recv_ack -> control -> conn_close -> pick over persistent columns: a linear chain."""

    def __init__(self, h):
        dev, cap, n = h.device, h.cap, N_CHAIN
        self.h = h
        self.t = {k: torch.zeros(n * (8 if k in ("id", "arena") else 1), dtype=P.tensor(np.zeros(1, dt), "cpu").dtype, device=dev)
                  for k, dt in CHAIN_COLS}
        self.of = {k: torch.zeros(M_CHAIN, dtype=P.tensor(np.zeros(1, dt), "cpu").dtype, device=dev) for k, dt in R.OFFER_COLS}
        self.n_offer = torch.zeros(1, dtype=torch.int32, device=dev)
        e = lambda k, dt=torch.int32: torch.empty(k, dtype=dt, device=dev)  # noqa: E731
        self.o = {"conn": e(n), "hit": e(n, torch.uint8), "miss": e(n, torch.int8), "n_miss": e(1), "new_rows": e(M_CHAIN),
                  "new_first": e(M_CHAIN), "new_offer": e(M_CHAIN), "offer_row": e(M_CHAIN), "n_new": e(1), "n_full": e(1),
                  "n_refused": e(1), "pick_counts": e(2)}
        self.c = {"marked_rows": e(cap), "n_marked": e(1), "closed_rows": e(cap), "n_closed": e(1), "pick_counts": e(2)}
        self.pk = {"conn": e(n), "n_none": e(1)}
        self.ctl = rc.ControlBuffers.alloc(n, dev, capacity=cap)
        self.ctl.dead_rows = self.ctl.n_dead = None
        self.work = h.tab.create_work(n, M_CHAIN)

    def load(self, b, offers, n_offer):
        for k, dt in CHAIN_COLS:
            self.t[k].copy_(P.tensor(np.ascontiguousarray(b[k], dt), self.t[k].device))
        for k, dt in R.OFFER_COLS:
            self.of[k].zero_()
            self.of[k][: len(offers[k])] = P.tensor(np.ascontiguousarray(offers[k], dt), self.of[k].device)
        self.n_offer.fill_(n_offer)
        for d in (self.o, self.c, self.pk):
            for v in d.values():
                v.view(torch.uint8).fill_(K.SENT)

    def run(self, codec, stream=None):
        t, o, tab, by_id = self.t, self.o, self.h.tab, self.h.by_id
        idc = t["id"] if by_id else None
        codec.conn_resolve_batch(tab, t["status"], t["conn_key"], o["conn"], cmd=t["cmd"], id=idc, hit=o["hit"], miss=o["miss"],
                                 n_miss=o["n_miss"], stream=stream)
        offers = rc.ConnOffers(n_offer=self.n_offer, m_max=M_CHAIN, **self.of)
        codec.conn_create_batch(tab, offers, self.work, stream=stream, u_max=N_CHAIN, conn_key=t["conn_key"], id=idc,
                                src=t["src"], dst=t["dst"], sp=t["sp"], dp=t["dp"], pick=True, established_ms=self.h.t_est,
                                ka_tries=self.h.t_ka, now_ms=77, **o)
        codec.tcp_recv_ack_batch(o["conn"], o["hit"], t["seq"], tab.ack, stream=stream)
        codec.control_batch(tab, t["status"], t["cmd"], t["pay_off"], t["pay_len"], t["arena"], t["base_off"], self.ctl,
                            id=idc, conn_key=t["conn_key"], miss=o["miss"], stream=stream)
        codec.conn_close_batch(tab, self.h.work, rst_first=self.ctl.rst_first, pick=True, stream=stream, **self.c)
        codec.conn_pick_batch(tab, self.pk["conn"], id=self.ctl.msg_id if by_id else None, avoid_key=self.ctl.msg_avoid_key,
                              seed=0x5EED, n_none=self.pk["n_none"], stream=stream)

    def check(self, b, offers, n_offer):
        """The chain's outputs against the restatements, and the harness's image brought up to date."""
        h, by_id, n = self.h, self.h.by_id, N_CHAIN
        idb = b["id"] if by_id else None
        tmap, _ = CR.table_map(h.cols["state"], h.cols["conn_key"], h.cols["id"] if by_id else None)
        conn, hit, miss, _ = CR.resolve_ref(tmap, b["status"], b["conn_key"], cmd=b["cmd"], id=idb)
        ref = R.create_ref(h.cols, by_id, offers, n_offer, M_CHAIN, b, miss, conn, hit, n, now_ms=77, est=h.est, ka=h.ka)
        got = {k: K.host(v, np.int8 if k == "miss" else np.uint8 if k == "hit" else np.uint32) for k, v in self.o.items()}
        for k in ("n_new", "n_full", "n_refused", "n_miss"):
            assert got[k][0] == ref[k], (k, got[k][0], ref[k])
        for k in ("conn", "hit", "miss"):
            assert np.array_equal(got[k], ref[k]), k
        m = ref["n_new"]
        for k in ("new_rows", "new_first", "new_offer"):
            assert np.array_equal(got[k][:m], ref[k]) and bool((got[k][m:] == K.SENT32).all()), k
        cols = ref["cols"]
        delivered = ref["hit"] != 0
        np.maximum.at(cols["ack"], ref["conn"][delivered].astype(np.int64), b["seq"][delivered])  # FakeTcp::OnRecv
        tmap, _ = CR.table_map(cols["state"], cols["conn_key"], cols["id"] if by_id else None)
        w = CR.id_words(idb, n)
        rst_first = np.full(h.cap, K.NO_RST, np.uint32)
        body = b["arena"].view(np.uint64)
        for i in np.nonzero(b["cmd"] == A.CMD_NETCONN_RST)[0].tolist():
            r = tmap.get((int(w[i]), int(body[i])))
            if r is not None and rst_first[r] == K.NO_RST:
                rst_first[r] = i
        assert np.array_equal(K.host(self.ctl.rst_first, np.uint32), rst_first)
        n_msg = int(K.host(self.ctl.n_msg, np.uint32)[0])
        assert n_msg == ref["n_miss"]
        closed = K.close_ref(cols["state"], rst_first != K.NO_RST)
        k = len(closed["marked_rows"])
        assert K.host(self.c["n_marked"], np.uint32)[0] == k and K.host(self.c["n_closed"], np.uint32)[0] == 0
        assert np.array_equal(K.host(self.c["marked_rows"], np.uint32)[:k], closed["marked_rows"])
        cols["state"] = closed["state"]
        h.cols, h.est, h.ka = cols, ref["est"], ref["ka"]
        h.killed |= set(closed["marked_rows"].tolist())
        h.killed -= set(ref["new_rows"].tolist())
        h.removed -= set(ref["new_rows"].tolist())
        h.compare_columns()
        mid = K.host(self.ctl.msg_id, np.uint8)[: 8 * n_msg] if by_id else None
        avoid = K.host(self.ctl.msg_avoid_key, np.uint64)[:n_msg]
        want = P.rule_ref(cols, by_id, n_msg, id=mid, avoid_key=avoid, seed=0x5EED)
        assert np.array_equal(K.host(self.pk["conn"], np.uint32)[:n_msg], want[0])
        h.check_lookups()
        h.check_picks()
        return m, k


@pytest.mark.parametrize("by_id", [False, True])
def test_chain_in_captured_graph(cx, gpu, by_id):
    """The chain captured on a side stream of a fresh context after a reserve, replayed three times on edited batches
    and offers: conns born, none born (nothing missing that has an offer), conns born again into rows and groups the
    earlier replays left.  Every replay against the restatements."""
    rng = np.random.default_rng(60 + by_id)
    cols = R.table(4097, by_id, seed=11)
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        cxg.reserve(N_CHAIN, stream=s)
        h = R.Harness(rc, cols, by_id, gpu, cx)
        ch = Chain(h)
        steps = []
        for step in range(4):  # step 0 is the warm-up call before the capture
            nc = R.new_conns(rng, cols, by_id, 40 if step != 2 else 5)
            nc["conn_key"] += np.uint64(step * 104729)
            nc["src"] += np.uint32((step + 1) << 24)
            steps.append(nc)
        g = None
        born = killed = 0
        for step, nc in enumerate(steps):
            live = np.nonzero((h.cols["state"] & K.UP) == K.UP)[0]
            b = chain_batch(rng, h.cols, by_id, nc, rng.permutation(live)[:20])
            offers, n_offer = (R.offers_of(nc), len(nc["src"])) if step != 2 else (R.offers_of(steps[0]), 0)
            ch.load(b, offers, n_offer)
            if g is None:
                with torch.cuda.stream(s):
                    ch.run(cxg)  # eager: loads the kernels
                torch.cuda.synchronize()
                m, k = ch.check(b, offers, n_offer)
                g = torch.cuda.CUDAGraph()
                keep = {name: getattr(h.tab, name).clone() for name, _, _ in rc._CONN_COLUMNS if getattr(h.tab, name) is not None}
                keep.update(index=h.tab.index.clone(), pick=h.tab.pick.clone(), est=h.t_est.clone(), ka=h.t_ka.clone())
                with torch.cuda.graph(g, stream=s):
                    ch.run(cxg, torch.cuda.current_stream())
                for name, v in keep.items():  # the capture ran nothing, but leave the table exactly as checked
                    (h.t_est if name == "est" else h.t_ka if name == "ka" else getattr(h.tab, name)).copy_(v)
                torch.cuda.synchronize()
                continue
            g.replay()
            torch.cuda.synchronize()
            m, k = ch.check(b, offers, n_offer)
            assert (m == 0) == (step == 2) and k > 0
            born += m
            killed += k
        assert born > 40 and killed > 20
        del g
    finally:
        cxg.close()


def test_two_streams(cx, gpu):
    """Two tables, each with its own work buffer, on two streams at once."""
    hs, args, streams = [], [], [torch.cuda.Stream(gpu) for _ in range(2)]
    for j, by_id in enumerate((False, True)):
        rng = np.random.default_rng(80 + j)
        cols = R.table(65536, by_id, seed=12 + j)
        h = R.Harness(rc, cols, by_id, gpu, cx)
        nc = R.new_conns(rng, cols, by_id, 3000)
        of = R.offers_of(nc, list_form=True)
        hs.append(h)
        args.append((of, h.offers_on(of, 3000, 3000, True), h.create_work(0, 3000),
                     {k: K.filled(3003 if "_" in k and not k.startswith("n_") else 1, torch.int32, gpu)
                      for k in ("new_rows", "new_offer", "offer_row", "n_new", "n_full", "n_refused")}))
    torch.cuda.synchronize()
    for h, (_of, offers, work, o), s in zip(hs, args, streams):
        with torch.cuda.stream(s):
            cx.conn_create_batch(h.tab, offers, work, list_form=True, pick=True, established_ms=h.t_est, ka_tries=h.t_ka,
                                 now_ms=5, **o)
    torch.cuda.synchronize()
    for h, (of, _offers, _work, o) in zip(hs, args):
        ref = R.create_ref(h.cols, h.by_id, of, 3000, 3000, list_form=True, now_ms=5, est=h.est, ka=h.ka)
        assert K.host(o["n_new"], np.uint32)[0] == ref["n_new"] == 3000
        assert np.array_equal(K.host(o["new_rows"], np.uint32)[:3000], ref["new_rows"])
        h.cols, h.est, h.ka = ref["cols"], ref["est"], ref["ka"]
        h.compare_columns()
        h.check_lookups()
        h.check_picks()
    for s in streams:
        cx.release_stream(s)
