"""TEST INFRASTRUCTURE: the scripts of tests/golden/conncreate.npz (tests/conncreate_golden.py: the reference's own
RawTcp / TcpAckPool / ServerNetManager / SNetGroup run) replayed with the pools kept by the rsk_pool_* calls where
conncreate_golden.HostModel, the documented host procedure, stood:

  SYN      parse -> pool add (ack pool, TOUCH, the parse's rows and parse_status as they are)
  ACCEPT   pool add, list form (socket pool)
  DATA     pool offers -> resolve -> conn_create -> recv_ack -> pool settle
  FLUSH_*  pool flush

After every event both pools' LIVE rows, sorted by (src, sp, dst, dp), are compared integer-exact with the record
(pa_rows / pa_exp / pn_rows / pn_exp: tuples, stored seq / ack, expiries) and the running sum of the settle's
n_closed and the socket pool's n_dead with `closed`.  A deviation script's still-pending offer is treated exactly
as conncreate_golden.check treats it, and everything that check asserts about conns, conn / hit / miss and the
rows' contents is asserted here too, so the chain as a whole is held to the record.

`pools`: pool_ref.LibPools (the library: host twins or a device) or pool_ref.RefPools (the model, or a mutant)."""
from __future__ import annotations

import numpy as np

from rsock_amd import _abi as A
from tests import conn_create_ref as R
from tests import conncreate_golden as G
from tests import pool_ref as PR

CAPACITIES = (67, 1025, 4097)


def largest_pool(s: dict) -> int:
    return int(max(np.diff(s["pa_off"]).max(initial=0), np.diff(s["pn_off"]).max(initial=0)))


def pool_capacity(s: dict) -> int:
    """The smallest of CAPACITIES that holds the script's largest recorded pool."""
    need = largest_pool(s)
    return next(c for c in CAPACITIES if c >= need)


def chain(dev, pools, b, m_max):
    """A DATA event: pool offers -> resolve -> conn_create -> recv_ack (dev.batch) -> pool settle, one call at a time.
    -> (the offers call's outputs, the offer columns the create took, the create's outputs, the settle's).  A `pools`
    with a chain method of its own (a captured graph) runs that instead."""
    off = pools.offers(m_max)
    offers = {k: (off[k] if off["n_offer"] else np.zeros(1, off[k].dtype)) for k in ("src", "dst", "sp", "dp", "ack", "flag")}
    got = dev.batch(b, offers, off["n_offer"])
    return off, offers, got, pools.settle(off, got, b)


def check(s: dict, dev, pools) -> dict:
    """Replay script s: conns on `dev` (conncreate_golden.Twin / Model), pools in `pools`.  -> counts of what was
    compared.  An AssertionError names the first difference."""
    exp = G.expected(s)
    assert bool(exp["moved"]) == bool(s["deviation"]), "only a deviation script may deviate, and it must"
    ids = np.ascontiguousarray(s["ids"], np.uint8).reshape(-1, 8)
    row_of, born, closed = {}, 0, 0
    order = np.argsort(exp["packet"], kind="stable")
    seen = {"packets": 0, "conns": 0, "snapshots": 0, "offers": 0, "purged": 0}
    for e, (kind, ts, lo, hi, _arg) in enumerate(G.events(s)):
        if kind == G.EV_SYN:
            t = dev.parse(G.syn_frames(s, lo, hi), G.PARSE_FLAGS)
            assert bool((t["parse_status"] == G.PARSE_SYN).all()), "a SYN capture the parse does not report as one"
            o = pools.harvest(t, ts + G.PERSIST_MS)
            assert o["n_full"] == 0
        elif kind == G.EV_ACCEPT:
            tup = np.asarray(s["acc_tuple"][lo:hi]).reshape(-1, 4)
            inp = {"src": tup[:, 0].astype(np.uint32), "dst": tup[:, 1].astype(np.uint32), "sp": tup[:, 2].astype(np.uint16),
                   "dp": tup[:, 3].astype(np.uint16)}
            o = pools.accept(inp, ts + G.PERSIST_MS)
            assert o["n_full"] == 0
        elif kind in (G.EV_FLUSH_ACK, G.EV_FLUSH_NET):
            o = pools.flush(kind - G.EV_FLUSH_ACK, ts)
            if kind == G.EV_FLUSH_NET:
                closed += o["n_dead"]
        elif kind == G.EV_DATA:
            t = dev.parse(G.data_frames(s, lo, hi), G.PARSE_FLAGS)
            assert bool((t["parse_status"] == G.PARSE_DELIVER).all())
            b = {k: t[k] for k in ("src", "dst", "sp", "dp", "seq")}
            b["conn_key"] = s["d_key"][lo:hi]
            b["id"] = np.ascontiguousarray(ids[s["d_group"][lo:hi]]).reshape(-1)
            off, offers, got, st = getattr(pools, "chain", chain)(dev, pools, b, max(largest_pool(s), 1))
            assert off["n_over"] == 0
            n_offer = off["n_offer"]
            closed += st["n_closed"]
            seen["offers"] += n_offer
            seen["purged"] += st["n_purged_ack"] + st["n_closed"]
            assert st["taken_sock_rows"].tolist() == off["offer_sock_row"][got["new_offer"][: int(got["n_new"][0])]].tolist()
            # what conncreate_golden.check asserts about the conns born here, in creation order
            mine = [o for o in order[born:].tolist() if lo <= exp["packet"][o] < hi]
            assert int(got["n_new"][0]) == len(mine), ("n_new", int(got["n_new"][0]), len(mine))
            assert int(got["n_full"][0]) == 0
            assert got["new_first"][: len(mine)].tolist() == [int(exp["packet"][o]) - lo for o in mine], "new_first"
            rows = dev.rows()
            for j, o in enumerate(mine):
                r = int(got["new_rows"][j])
                row_of[o] = r
                info = s["c_info"][o]
                want = (int(s["c_key"][o]), ids[s["c_group"][o]].tobytes(), *info[[0, 1, 2, 3, 6, 4]].tolist(), R.BORN)
                have = (int(rows["conn_key"][r]), rows["id"].reshape(-1, 8)[r].tobytes(), int(rows["src"][r]), int(rows["dst"][r]),
                        int(rows["sp"][r]), int(rows["dp"][r]), int(rows["flag"][r]), int(rows["seq"][r]), int(rows["state"][r]))
                assert have == want, ("row", o, have, want)
                assert (int(offers["ack"][got["new_offer"][j]]) + 2) & 0xFFFFFFFF == int(info[5]), ("ack after Init", o)
            born += len(mine)
            seen["conns"] += len(mine)
            ec = exp["conn"][lo:hi]
            want_conn = np.array([row_of[c] if c >= 0 else G.NONE for c in ec.tolist()], np.uint32)
            assert np.array_equal(got["conn"], want_conn), ("conn", np.nonzero(got["conn"] != want_conn)[0][:8])
            assert np.array_equal(got["hit"], (ec >= 0).astype(np.uint8)), "hit"
            assert np.array_equal(got["miss"], np.where(ec >= 0, A.RECV_DROP, A.RECV_VALID).astype(np.int8)), "miss"
            same = exp["conn"][lo:hi] == s["r_conn"][lo:hi]
            assert np.array_equal((s["r_ret"][lo:hi] == G.ERR_NO_CONN)[same], (ec < 0)[same])
            assert bool((s["r_ret"][lo:hi][ec >= 0] == G.PAYLOAD).all())
            refused = {(int(g), int(k)) for g, k, c in zip(s["d_group"][lo:hi], s["d_key"][lo:hi], ec) if c < 0}
            assert int(got["n_refused"][0]) == len(refused), ("n_refused", int(got["n_refused"][0]), len(refused))
            last = {}
            for i, c in enumerate(ec.tolist()):
                if c >= 0:
                    last[c] = lo + i
            unmoved = [c for c in last if c not in exp["moved"]]
            assert [int(rows["ack"][row_of[c]]) for c in unmoved] == [int(s["r_ack"][last[c]]) for c in unmoved], "ack"
            seen["packets"] += hi - lo
        # a SEND event: the pick is conncreate_golden.check's business; the pools do not move
        # both pools after the event; a moved conn's offer is still whole here, consumed there
        ca, cs = pools.columns()
        (a, ae), (n, ne) = PR.snapshot(ca), PR.snapshot(cs)
        ra, rae = s["pa_rows"][s["pa_off"][e]:s["pa_off"][e + 1]], s["pa_exp"][s["pa_off"][e]:s["pa_off"][e + 1]]
        rn, rne = s["pn_rows"][s["pn_off"][e]:s["pn_off"][e + 1]], s["pn_exp"][s["pn_off"][e]:s["pn_off"][e + 1]]
        for e0, e1, o in exp["pending"]:
            if e0 <= e <= e1:
                tup = s["c_info"][o][:4]
                keep_a = ~(a[:, :4] == tup).all(axis=1)
                keep_n = ~(n == tup).all(axis=1)
                assert int((~keep_a).sum()) == 1 and int((~keep_n).sum()) == 1, "the moved conn's offer is not held"
                a, ae, n, ne = a[keep_a], ae[keep_a], n[keep_n], ne[keep_n]
        assert np.array_equal(a, ra) and np.array_equal(ae, rae), ("ack pool after event", e, a.tolist()[:4], ra.tolist()[:4],
                                                                     ae.tolist()[:4], rae.tolist()[:4])
        assert np.array_equal(n, rn) and np.array_equal(ne, rne), ("socket pool after event", e, n.tolist()[:4], rn.tolist()[:4])
        assert closed == int(s["closed"][e]), ("sockets closed after event", e, closed, int(s["closed"][e]))
        seen["snapshots"] += 1
    assert born == len(s["c_key"])
    pools.check_indexes("after the script")
    return seen
