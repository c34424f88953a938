"""GPU: the chain parse -> rsk_pool_add_batch -> rsk_pool_offers -> resolve -> rsk_conn_create_batch -> recv_ack ->
rsk_pool_settle_batch and rsk_pool_flush, held to tests/golden/conncreate.npz: what the REFERENCE's own TcpAckPool and
ServerNetManager held after every event of 20 scripts, and what its SNetGroup made of the packets
(tests/pool_golden.py; tests/test_pool_host.py runs the same checker on the host twins and shows with mutants that
the fixture sees each rule).  Every script at the smallest pool capacity that holds it and at 4097; the client's
dials through the pools into the create's list form; one multi-batch script with its whole DATA chain replayed from
one captured graph."""
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
from tests import pool_golden as PG
from tests import pool_ref as PR

pytestmark = pytest.mark.gpu

KEY = b"hello135"
CASES = [(name, cap) for name in G.names() for cap in sorted({PG.pool_capacity(G.script(name)), 4097})]


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


@pytest.mark.parametrize("name,capacity", CASES)
def test_device_equals_the_reference(cx, gpu, oracle, name, capacity):
    s = G.script(name)
    seen = PG.check(s, G.Twin(rc, int(s["capacity"]), gpu, cx, oracle), PR.LibPools(PR.Lib(rc, gpu, cx), capacity, capacity))
    assert seen["packets"] == len(s["d_key"]) and seen["conns"] == len(s["c_key"])
    assert seen["snapshots"] == len(s["ev_kind"])


@pytest.mark.parametrize("k", [1, 64, 2049])
def test_client_dials_through_the_pools(cx, gpu, oracle, k):
    """A client: the handshakes harvested without the server flag, the dialled tuples added to the socket pool,
    rsk_pool_offers with conn_key, and its columns -- as they lie on the device -- handed to the create's list form."""
    c = G.client_case(k)
    lib = PR.Lib(rc, gpu, cx)
    dev = G.Twin(rc, 257, gpu, cx, oracle)
    f = G.frames(c["syn_src"], c["syn_dst"], c["syn_sport"], c["syn_dport"], c["syn_seq"], c["syn_ack"], np.full(k, 0x12, np.uint8), 0)
    t = dev.parse(f, A.PARSE_HAS_ACK_POOL)
    assert bool((t["parse_status"] == G.PARSE_SYN).all())
    cap = 4097
    pools = PR.LibPools(lib, cap, cap)
    assert pools.harvest(t, 1000)["n_new"] == k
    tup = c["tuple"]
    dial = {"src": tup[:, 0].astype(np.uint32), "dst": tup[:, 1].astype(np.uint32), "sp": tup[:, 2].astype(np.uint16),
            "dp": tup[:, 3].astype(np.uint16)}
    assert pools.accept(dial, 1000)["n_new"] == k
    b = lib.offer_buffers(k, conn_key=True)
    cx.pool_offers(pools.ta, pools.ts, lib.conn_offers(b, k), offer_ack_row=b["offer_ack_row"], offer_sock_row=b["offer_sock_row"],
                   n_over=b["n_over"])
    h = R.Harness(rc, R.table(4097, False, seed=1, empty=True), False, gpu, cx)
    o = {name: K.filled(k + 3, torch.int32, gpu) for name in ("new_rows", "new_offer", "offer_row")}
    o.update({name: K.filled(1, torch.int32, gpu) for name in ("n_new", "n_full", "n_refused")})
    cx.conn_create_batch(h.tab, lib.conn_offers(b, k), h.create_work(0, k), list_form=True, pick=True, now_ms=1,
                         established_ms=h.t_est, ka_tries=h.t_ka, pick_counts=K.filled(2, torch.int32, gpu), **o)
    torch.cuda.synchronize()
    got = {name: K.host(v, np.uint32) for name, v in o.items()}
    assert got["n_new"][0] == k and got["n_refused"][0] == 0 and got["n_full"][0] == 0
    assert K.host(b["n_offer"], np.uint32)[0] == k and K.host(b["n_over"], np.uint32)[0] == 0
    offers = {name: K.host(b[name], dt)[:k] for name, dt in R.OFFER_COLS}
    offers["conn_key"] = K.host(b["conn_key"], np.uint64)[:k]
    # the offers stand in ack-pool row order; check_client takes them in the case's order: matched by tuple
    at = {tuple(x): j for j, x in enumerate(zip(offers["src"].tolist(), offers["dst"].tolist(), offers["sp"].tolist(), offers["dp"].tolist()))}
    p = np.array([at[tuple(x)] for x in tup.tolist()], np.int64)
    assert sorted(p.tolist()) == list(range(k))
    assert got["new_offer"][:k].tolist() == list(range(k))
    G.check_client(c, {name: v[p] for name, v in offers.items()}, G.table_rows(h.tab), got["new_rows"][:k][p])
    assert np.array_equal(h.resolve(c["key"], None), got["new_rows"][:k][p])
    # the settle behind it: every offer became a conn, both pools are empty again
    st = lib.settle(pools.ta, pools.ts, got["new_offer"][:k], k, K.host(b["offer_ack_row"], np.uint32)[:k],
                    K.host(b["offer_sock_row"], np.uint32)[:k], np.zeros(0, np.int8), {})
    assert st["n_closed"] == 0 and st["n_purged_ack"] == 0 and len(st["taken_sock_rows"]) == k
    ca, cs = pools.columns()
    assert not (ca["state"] & PR.LIVE).any() and not (cs["state"] & PR.LIVE).any()
    pools.check_indexes("client")


# ---- a script's DATA chains from one captured graph ---------------------------------------------------------------
class GraphPools(PR.LibPools):
    """LibPools whose DATA chain pool_offers -> resolve -> conn_create -> recv_ack -> pool_settle runs over persistent
    columns of the script's largest batch (the rest of a smaller batch is not VALID): the first batch eagerly on a
    side stream of a fresh context after a reserve, every later one as a replay of the graph captured behind it.  A
    linear chain: no parallel branches."""

    COLS = (("status", np.int8), ("conn_key", np.uint64), ("id", np.uint8), ("src", np.uint32), ("dst", np.uint32),
            ("sp", np.uint16), ("dp", np.uint16), ("seq", np.uint32))

    def __init__(self, lib, capacity, twin, n_max, m_max):
        super().__init__(lib, capacity, capacity)
        self.twin, self.n, self.m, dev = twin, n_max, m_max, lib.device
        self.stream = torch.cuda.Stream(dev)
        lib.codec.reserve(n_max, stream=self.stream)
        self.t = {k: torch.zeros(n_max * (8 if k == "id" else 1), dtype=P.tensor(np.zeros(1, dt), "cpu").dtype, device=dev)
                  for k, dt in self.COLS}
        self.ob = lib.offer_buffers(m_max)
        e = lambda k, dt=torch.int32: torch.empty(k, dtype=dt, device=dev)  # noqa: E731
        self.o = {"conn": e(n_max), "hit": e(n_max, torch.uint8), "miss": e(n_max, torch.int8), "n_miss": e(1), "new_rows": e(m_max),
                  "new_first": e(m_max), "new_offer": e(m_max), "offer_row": e(m_max), "n_new": e(1), "n_full": e(1),
                  "n_refused": e(1), "pick_counts": e(2)}
        self.so = {"taken": e(m_max), "closed": e(capacity), "cnt": e(2)}
        self.work = twin.h.tab.create_work(n_max, m_max)
        self.swork = self.ta.settle_work(self.ts)
        self.graph, self.replays = None, 0

    def run(self, stream=None):
        t, o, ob, so, h, cx = self.t, self.o, self.ob, self.so, self.twin.h, self.lib.codec
        offers = self.lib.conn_offers(ob, self.m)
        cx.pool_offers(self.ta, self.ts, offers, offer_ack_row=ob["offer_ack_row"], offer_sock_row=ob["offer_sock_row"],
                       n_over=ob["n_over"], stream=stream)
        cx.conn_resolve_batch(h.tab, t["status"], t["conn_key"], o["conn"], id=t["id"], hit=o["hit"], miss=o["miss"],
                              n_miss=o["n_miss"], stream=stream)
        cx.conn_create_batch(h.tab, offers, self.work, stream=stream, u_max=self.n, conn_key=t["conn_key"], id=t["id"],
                             src=t["src"], dst=t["dst"], sp=t["sp"], dp=t["dp"], pick=True, established_ms=h.t_est,
                             ka_tries=h.t_ka, now_ms=1, **o)
        cx.tcp_recv_ack_batch(o["conn"], o["hit"], t["seq"], h.tab.ack, stream=stream)
        cx.pool_settle_batch(self.ta, self.ts, self.swork, new_offer=o["new_offer"], n_new=o["n_new"],
                             offer_ack_row=ob["offer_ack_row"], offer_sock_row=ob["offer_sock_row"], m_max=self.m, miss=o["miss"],
                             src=t["src"], dst=t["dst"], sp=t["sp"], dp=t["dp"], new_max=self.m, taken_sock_rows=so["taken"],
                             closed_sock_rows=so["closed"], n_closed=so["cnt"][0:1], n_purged_ack=so["cnt"][1:2], stream=stream)

    def tables(self):
        h = self.twin.h
        keep = {("conn", name): getattr(h.tab, name) for name, _, _ in rc._CONN_COLUMNS if getattr(h.tab, name) is not None}
        keep.update({("conn", "index"): h.tab.index, ("conn", "pick"): h.tab.pick, ("conn", "est"): h.t_est, ("conn", "ka"): h.t_ka})
        for which, tab in (("ack", self.ta), ("sock", self.ts)):
            keep.update({(which, name): getattr(tab, name) for name, _ in PR.COLS if getattr(tab, name) is not None})
            keep[(which, "index")] = tab.index
        return keep

    def chain(self, dev, pools, b, m_max):
        assert dev is self.twin and pools is self
        n = len(b["conn_key"])
        assert n <= self.n
        cols = dict(b, status=np.full(n, A.RECV_VALID, np.int8))
        for k, dt in self.COLS:
            self.t[k].zero_()
            v = P.tensor(np.ascontiguousarray(cols[k], dt), self.lib.device)
            self.t[k][: v.numel()] = v
        for v in list(self.o.values()) + list(self.so.values()) + list(self.ob.values()):
            v.view(torch.uint8).fill_(K.SENT)
        torch.cuda.synchronize()
        if self.graph is None:
            with torch.cuda.stream(self.stream):
                self.run()  # eager: loads the kernels
            torch.cuda.synchronize()
            keep = {k: v.clone() for k, v in self.tables().items()}
            out = self.outputs(n)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=self.stream):
                self.run(torch.cuda.current_stream())
            for k, v in self.tables().items():  # the capture ran nothing, but leave the tables exactly as the eager run did
                v.copy_(keep[k])
            torch.cuda.synchronize()
            return out
        self.graph.replay()
        torch.cuda.synchronize()
        self.replays += 1
        return self.outputs(n)

    def outputs(self, n):
        got = {k: K.host(v, np.int8 if k == "miss" else np.uint8 if k == "hit" else np.uint32) for k, v in self.o.items()}
        assert bool((got["conn"][n:] == A.CONN_NONE).all()) and not got["hit"][n:].any(), "a packet that is not VALID was resolved"
        for k in ("conn", "hit", "miss"):
            got[k] = got[k][:n]
        ob = self.ob
        k = int(K.host(ob["n_offer"], np.uint32)[0])
        assert k <= self.m
        off = {"n_offer": k, "n_over": int(K.host(ob["n_over"], np.uint32)[0])}
        for name, dt in R.OFFER_COLS + (("offer_ack_row", np.uint32), ("offer_sock_row", np.uint32)):
            a = K.host(ob[name], dt)
            assert bool((a[k:].view(np.uint8) == K.SENT).all()), (name, "written behind the list's end")
            off[name] = a[:k].copy()
        offers = {name: (off[name] if k else np.zeros(1, dt)) for name, dt in R.OFFER_COLS}
        cnt = K.host(self.so["cnt"], np.uint32)
        taken, closed = K.host(self.so["taken"], np.uint32), K.host(self.so["closed"], np.uint32)
        nn = int(got["n_new"][0])
        assert bool((taken[nn:].view(np.uint8) == K.SENT).all()) and bool((closed[int(cnt[0]):].view(np.uint8) == K.SENT).all())
        st = {"taken_sock_rows": taken[:nn].copy(), "closed_sock_rows": closed[: int(cnt[0])].copy(), "n_closed": int(cnt[0]),
              "n_purged_ack": int(cnt[1])}
        return off, offers, got, st


def test_script_replayed_from_a_captured_graph(gpu, oracle):
    """half_offers: three batches between which handshakes and sockets arrive and refusals empty the pools."""
    s = G.script("half_offers")
    sizes = [hi - lo for k, _t, lo, hi, _a in G.events(s) if k == G.EV_DATA]
    assert len(sizes) >= 3
    cxg = rc.Codec(KEY, 0)
    try:
        twin = G.Twin(rc, 257, gpu, cxg, oracle)
        pools = GraphPools(PR.Lib(rc, gpu, cxg), 67, twin, max(sizes), 16)
        seen = PG.check(s, twin, pools)
        assert pools.replays == len(sizes) - 1 and seen["conns"] == len(s["c_key"]) > 0
        assert seen["offers"] > 0 and seen["purged"] > 0
        del pools.graph
    finally:
        cxg.close()
