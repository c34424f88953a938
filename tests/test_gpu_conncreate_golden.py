"""GPU: rsk_parse_decode_batch's SYN rows -> the documented host procedure -> rsk_conn_resolve_batch ->
rsk_conn_create_batch -> rsk_tcp_recv_ack_batch -> rsk_conn_pick_batch, held to tests/golden/conncreate.npz: what the
REFERENCE's own RawTcp, TcpAckPool, ServerNetManager, SNetGroup, INetGroup and FakeTcp did with the same scripts.
tests/conncreate_golden.py is the checker (shared with tests/test_conncreate_golden.py, which runs it on the host
twin and shows with mutants that the fixture sees each rule).  BY_ID tables of 257 and 4097 rows, every script; the
documented deviation; the client's list form; one multi-batch script replayed from a captured graph."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_close_ref as K
from tests import conn_create_ref as R
from tests import conncreate_golden as G
from tests import pick_ref as P

pytestmark = pytest.mark.gpu

KEY = b"hello135"
CASES = [(name, cap) for name in G.names() for cap in G.capacities(G.script(name))]


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


@pytest.mark.parametrize("name,capacity", CASES)
def test_device_equals_the_reference(cx, gpu, oracle, name, capacity):
    s = G.script(name)
    seen = G.check(s, G.Twin(rc, capacity, gpu, cx, oracle))
    assert seen["packets"] == len(s["d_key"]) and seen["conns"] == len(s["c_key"])
    assert seen["snapshots"] == len(s["ev_kind"]) and seen["sends"] == len(s["s_draws"])


def test_the_deviation_is_the_documented_one(cx, gpu, oracle):
    """A refused key whose later packet carries another tuple that has an offer: refused in this call, its packets in
    miss, its offer left whole, born by the next call -- and the reference, which creates at that later packet,
    differs at that key's packets only."""
    s = G.script("deviation_other_tuple")
    exp = G.expected(s)
    assert len(exp["moved"]) == 1
    o = exp["moved"][0]
    differ = np.nonzero(exp["conn"] != s["r_conn"])[0]
    at = np.nonzero((s["d_group"] == s["c_group"][o]) & (s["d_key"] == s["c_key"][o]))[0]
    (_e0, lo, hi), (_e1, lo2, _hi2) = [(e, lo, hi) for e, (k, _t, lo, hi, _a) in enumerate(G.events(s)) if k == G.EV_DATA]
    assert differ.tolist() == [i for i in at.tolist() if s["c_packet"][o] <= i < hi]  # from the reference's create on
    assert lo <= s["c_packet"][o] < hi and exp["packet"][o] == at[at >= lo2][0]       # born by the next call
    seen = G.check(s, G.Twin(rc, 257, gpu, cx, oracle))
    assert seen["conns"] == len(s["c_key"]) and seen["refused"] >= 1


@pytest.mark.parametrize("k", [1, 64, 2049])
def test_client_dials_list_form(cx, gpu, oracle, k):
    c = G.client_case(k)
    offers = G.client_offers(c, oracle)
    h = R.Harness(rc, R.table(4097, False, seed=1, empty=True), False, gpu, cx)
    got = h.raw_create(offers, k, k, list_form=True)
    assert got["n_new"][0] == k and got["n_refused"][0] == 0 and got["n_full"][0] == 0
    G.check_client(c, offers, G.table_rows(h.tab), got["new_rows"][:k])
    assert np.array_equal(h.resolve(c["key"], None), got["new_rows"][:k])


# ---- a script's batches from one captured graph -------------------------------------------------------------------
class GraphTwin(G.Twin):
    """G.Twin whose resolve -> conn_create -> recv_ack runs over persistent columns of the script's largest batch
    (the rest of a smaller batch is not VALID): the first batch eagerly on a side stream of a fresh context after a
    reserve, every later one as a replay of the graph captured behind it."""

    COLS = (("status", np.int8), ("conn_key", np.uint64), ("id", np.uint8), ("src", np.uint32), ("dst", np.uint32),
            ("sp", np.uint16), ("dp", np.uint16), ("seq", np.uint32))

    def __init__(self, capacity, device, codec, oracle, n_max, m_max):
        super().__init__(rc, capacity, device, codec, oracle)
        self.n, self.m, dev = n_max, m_max, device
        self.stream = torch.cuda.Stream(device)
        codec.reserve(n_max, stream=self.stream)
        self.t = {k: torch.zeros(n_max * (8 if k == "id" else 1), dtype=P.tensor(np.zeros(1, dt), "cpu").dtype, device=dev)
                  for k, dt in self.COLS}
        self.of = {k: torch.zeros(m_max, dtype=P.tensor(np.zeros(1, dt), "cpu").dtype, device=dev) for k, dt in R.OFFER_COLS}
        self.n_offer = torch.zeros(1, dtype=torch.int32, device=dev)
        e = lambda k, dt=torch.int32: torch.empty(k, dtype=dt, device=dev)  # noqa: E731
        self.o = {"conn": e(n_max), "hit": e(n_max, torch.uint8), "miss": e(n_max, torch.int8), "n_miss": e(1), "new_rows": e(m_max),
                  "new_first": e(m_max), "new_offer": e(m_max), "offer_row": e(m_max), "n_new": e(1), "n_full": e(1),
                  "n_refused": e(1), "pick_counts": e(2)}
        self.work = self.h.tab.create_work(n_max, m_max)
        self.graph, self.replays = None, 0

    def run(self, stream=None):
        t, o, tab, cx = self.t, self.o, self.h.tab, self.codec
        cx.conn_resolve_batch(tab, t["status"], t["conn_key"], o["conn"], id=t["id"], hit=o["hit"], miss=o["miss"],
                              n_miss=o["n_miss"], stream=stream)
        offers = rc.ConnOffers(n_offer=self.n_offer, m_max=self.m, **self.of)
        cx.conn_create_batch(tab, offers, self.work, stream=stream, u_max=self.n, conn_key=t["conn_key"], id=t["id"], src=t["src"],
                             dst=t["dst"], sp=t["sp"], dp=t["dp"], pick=True, established_ms=self.h.t_est, ka_tries=self.h.t_ka,
                             now_ms=1, **o)
        cx.tcp_recv_ack_batch(o["conn"], o["hit"], t["seq"], tab.ack, stream=stream)

    def batch(self, b, offers, n_offer):
        n = len(b["conn_key"])
        assert n <= self.n and n_offer <= self.m
        cols = dict(b, status=np.full(n, A.RECV_VALID, np.int8))
        for k, dt in self.COLS:
            self.t[k].zero_()
            v = P.tensor(np.ascontiguousarray(cols[k], dt), self.device)
            self.t[k][: v.numel()] = v
        for k, dt in R.OFFER_COLS:
            self.of[k].zero_()
            self.of[k][: len(offers[k])] = P.tensor(np.ascontiguousarray(offers[k], dt), self.device)
        self.n_offer.fill_(n_offer)
        for v in self.o.values():
            v.view(torch.uint8).fill_(K.SENT)
        torch.cuda.synchronize()
        if self.graph is None:
            with torch.cuda.stream(self.stream):
                self.run()  # eager: loads the kernels
            torch.cuda.synchronize()
            h = self.h
            keep = {name: getattr(h.tab, name).clone() for name, _, _ in rc._CONN_COLUMNS if getattr(h.tab, name) is not None}
            keep.update(index=h.tab.index.clone(), pick=h.tab.pick.clone(), est=h.t_est.clone(), ka=h.t_ka.clone())
            got = self.outputs(n)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.run(torch.cuda.current_stream())
            for name, v in keep.items():  # the capture ran nothing, but leave the table exactly as the eager call did
                (h.t_est if name == "est" else h.t_ka if name == "ka" else getattr(h.tab, name)).copy_(v)
            torch.cuda.synchronize()
            return got
        self.graph.replay()
        torch.cuda.synchronize()
        self.replays += 1
        return self.outputs(n)

    def outputs(self, n):
        got = {k: K.host(v, np.int8 if k == "miss" else np.uint8 if k == "hit" else np.uint32) for k, v in self.o.items()}
        assert bool((got["conn"][n:] == A.CONN_NONE).all()) and not got["hit"][n:].any(), "a packet that is not VALID was resolved"
        for k in ("conn", "hit", "miss"):
            got[k] = got[k][:n]
        return got


def test_script_replayed_from_a_captured_graph(gpu, oracle):
    """half_offers: three batches between which handshakes and sockets arrive and refusals empty the pools."""
    s = G.script("half_offers")
    sizes = [hi - lo for k, _t, lo, hi, _a in G.events(s) if k == G.EV_DATA]
    assert len(sizes) >= 3
    cxg = rc.Codec(KEY, 0)
    try:
        dev = GraphTwin(257, gpu, cxg, oracle, max(sizes), 16)
        seen = G.check(s, dev)
        assert dev.replays == len(sizes) - 1 and seen["conns"] == len(s["c_key"]) > 0 and seen["refused"] > 0
        del dev.graph
    finally:
        cxg.close()
