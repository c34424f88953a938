#!/usr/bin/env python3
"""Times the four tuple-pool calls (rsk_pool_add_batch, rsk_pool_offers, rsk_pool_settle_batch, rsk_pool_flush) on one
GPU and writes profiles/pool_paths.json.

Shapes: C3 (4 Mi packets, 28232 conns) with every conn's handshake and socket pending and again with none pending; C4
(1 Mi packets, 272 K conns) with all pending; a flush over 2^20 rows with a fifth expired and with none.  In the
"pending" batches one packet per conn is a SYN row of the parse (parse_status == RSK_PARSE_SYN) and every other a
DATA row; the settle takes every offer (n_new = offers) and finds nothing missing.

Beside each shape two baselines of the same run:
  parent route   what the host did around rsk_conn_create_batch before the pool: the D2H copy of the parse's
                 parse_status and TcpInfo columns (22 B per packet), the documented host procedure (INTEGRATION.md:
                 harvest, accept, the join into offer columns, the pops behind the batch -- timed twice: in numpy /
                 Python dicts as tests/conncreate_golden.HostModel has it, and as the C++ host twins rsk_pool_*_host
                 on host pools, which is the figure the ratios use), the H2D copy of the offers; host clock around
                 device synchronisation, every part reported apart
  conn_resolve   rsk_conn_resolve_batch of the same batch on a table of the shape's conns: the project's yardstick

Timing: device events on a side stream, `--reps` calls per window, the median of `--rounds` windows; a call that
consumes its input has the pools restored before every call outside the timed span.  One box, one run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rsock_amd import _abi as A  # noqa: E402
from rsock_amd import codec as rc  # noqa: E402

SHAPES = {"c3": (4 << 20, 28232), "c4": (1 << 20, 272 * 1024)}


def dev(a, device):
    a = np.ascontiguousarray(a)
    v = a.view(np.uint8 if a.dtype == np.uint8 else f"i{a.dtype.itemsize}")
    return torch.from_numpy(v.copy()).to(device)


def conn_tuples(k):
    c = np.arange(k, dtype=np.uint64)
    return {"src": (0x0A000000 + c).astype(np.uint32), "dst": np.full(k, 0xC0A80001, np.uint32),
            "sp": (1024 + c % 60000).astype(np.uint16), "dp": (443 + c // 60000).astype(np.uint16)}


class Timer:
    def __init__(self, stream, rounds, reps):
        self.s, self.rounds, self.reps, self.out = stream, rounds, reps, {}

    def device(self, name, f, prep=None, rows=None):
        f() if prep is None else (prep(), f())  # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(self.rounds):
            if prep is None:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(self.s)
                for _ in range(self.reps):
                    f()
                e1.record(self.s)
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / self.reps)
            else:
                evs = []
                for _ in range(self.reps):
                    prep()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(self.s)
                    f()
                    e1.record(self.s)
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                ms.append(sum(a.elapsed_time(b) for a, b in evs) / self.reps)
        self.out[name] = dict(ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), **(rows or {}))
        return self.out[name]["ms"]

    def host(self, name, f, rows=None):
        f()
        ms = []
        for _ in range(self.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            parts = f()
            torch.cuda.synchronize()
            ms.append(((time.perf_counter() - t0) * 1e3, parts))
        ms.sort(key=lambda x: x[0])
        mid = ms[len(ms) // 2]
        self.out[name] = dict(ms=round(mid[0], 4), min_ms=round(ms[0][0], 4), max_ms=round(ms[-1][0], 4),
                              parts_ms={k: round(v, 4) for k, v in mid[1].items()}, **(rows or {}))
        return self.out[name]["ms"]


def pool_pair(cap, device):
    return rc.PoolTable.alloc(cap, device, vals=True), rc.PoolTable.alloc(cap, device, vals=False)


def snapshot(tab):
    return tab.state.clone(), tab.index.clone()


def restorer(pairs, stream):
    def run():
        with torch.cuda.stream(stream):
            for tab, (st, ix) in pairs:
                tab.state.copy_(st)
                tab.index.copy_(ix)
    return run


def shape(cx, device, s, name, n, k, tm: Timer, pending: bool):
    """One shape's paths; -> its dict."""
    sfx = "" if pending else "_none"
    tup = conn_tuples(k)
    rng = np.random.default_rng(n + k)
    conn_of = np.concatenate([np.arange(k), rng.integers(0, k, n - k)]).astype(np.int64)  # every conn's first packet leads
    pk = {f: dev(tup[f][conn_of], device) for f in ("src", "dst", "sp", "dp")}
    seq = dev(rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), device)
    ack = dev(rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32), device)
    flag = torch.full((n,), 0x10, dtype=torch.uint8, device=device)
    status = np.full(n, A.PARSE_DELIVER, np.int8)
    if pending:
        status[:k] = A.PARSE_SYN
    status_d = dev(status, device)
    cap = 1
    while cap < 2 * k:
        cap <<= 1
    cap = min(cap, A.CONN_MAX_ROWS)
    ta, ts = pool_pair(cap, device)
    with torch.cuda.stream(s):
        ta.rebuild(cx, stream=s)
        ts.rebuild(cx, stream=s)
    torch.cuda.synchronize()
    empty = [(ta, snapshot(ta)), (ts, snapshot(ts))]
    i32 = lambda m: torch.zeros(max(m, 1), dtype=torch.int32, device=device)  # noqa: E731
    cnt = i32(12)
    u_max = min(n, 1 << 24)
    work = ta.add_work(u_max)
    add = lambda: cx.pool_add_batch(ta, pk["src"], pk["dst"], pk["sp"], pk["dp"], 1000, u_max, work, seq=seq, ack=ack,  # noqa: E731
                                    parse_status=status_d, touch=True, n_new=cnt[0:1], n_again=cnt[1:2], n_full=cnt[2:3],
                                    n_zero_port=cnt[3:4], stream=s)
    tm.device(f"{name}_pool_add{sfx}", add, restorer(empty[:1], s), {"packets": n, "syn_rows": k if pending else 0, "capacity": cap})
    torch.cuda.synchronize()
    assert cnt[:4].tolist() == [k if pending else 0, 0, 0, 0], cnt.tolist()
    # the accepted sockets, list form (not part of the packet chain: the accept path's own call)
    acc = {f: dev(tup[f], device) for f in ("src", "dst", "sp", "dp")}
    awork = ts.add_work(k)
    accept = lambda: cx.pool_add_batch(ts, acc["src"], acc["dst"], acc["sp"], acc["dp"], 1000, k, awork, n_new=cnt[4:5], stream=s)  # noqa: E731
    if pending:
        tm.device(f"{name}_pool_accept", accept, restorer(empty[1:], s), {"tuples": k, "capacity": cap})
        assert int(cnt[4]) == k
    # the pools as the DATA chain finds them
    restorer(empty, s)()
    if pending:
        add()
        accept()
    torch.cuda.synchronize()
    full = [(ta, snapshot(ta)), (ts, snapshot(ts))]
    m_max = max(k, 1)
    ob = {"src": i32(m_max), "dst": i32(m_max), "sp": torch.zeros(m_max, dtype=torch.int16, device=device),
          "dp": torch.zeros(m_max, dtype=torch.int16, device=device), "ack": i32(m_max),
          "flag": torch.zeros(m_max, dtype=torch.uint8, device=device), "n_offer": cnt[5:6]}
    ar, sr = i32(m_max), i32(m_max)
    offers = rc.ConnOffers(ob["src"], ob["dst"], ob["sp"], ob["dp"], ob["ack"], ob["flag"], ob["n_offer"], m_max=m_max)
    off = lambda: cx.pool_offers(ta, ts, offers, offer_ack_row=ar, offer_sock_row=sr, n_over=cnt[6:7], stream=s)  # noqa: E731
    tm.device(f"{name}_pool_offers{sfx}", off, None, {"rows": cap, "offers": k if pending else 0})
    torch.cuda.synchronize()
    assert cnt[5:7].tolist() == [k if pending else 0, 0], cnt.tolist()
    # the settle: every offer became a conn, nothing is missing
    new_offer = torch.arange(m_max, dtype=torch.int32, device=device)
    n_new = cnt[7:8]
    n_new.fill_(k if pending else 0)
    miss = torch.full((n,), A.RECV_DROP, dtype=torch.int8, device=device)
    swork = ta.settle_work(ts)
    taken, closed = i32(m_max), i32(cap)
    settle = lambda: cx.pool_settle_batch(ta, ts, swork, new_offer=new_offer, n_new=n_new, offer_ack_row=ar, offer_sock_row=sr,  # noqa: E731
                                          m_max=m_max, miss=miss, src=pk["src"], dst=pk["dst"], sp=pk["sp"], dp=pk["dp"],
                                          new_max=m_max, taken_sock_rows=taken, closed_sock_rows=closed, n_closed=cnt[8:9],
                                          n_purged_ack=cnt[9:10], stream=s)
    tm.device(f"{name}_pool_settle{sfx}", settle, restorer(full, s) if pending else None, {"packets": n, "taken": k if pending else 0})
    torch.cuda.synchronize()
    assert cnt[8:10].tolist() == [0, 0] and int((ta.state & 1).sum()) == 0 and int((ts.state & 1).sum()) == 0
    # the timer: nothing expired (every entry's expiry is 1000), then everything
    restorer(full, s)()
    dead = i32(cap)
    tm.device(f"{name}_pool_flush_keep{sfx}", lambda: cx.pool_flush(ta, 999, dead_rows=dead, n_dead=cnt[10:11], stream=s), None,
              {"rows": cap, "dead": 0})
    assert int(cnt[10]) == 0
    if pending:
        tm.device(f"{name}_pool_flush_all", lambda: cx.pool_flush(ta, 1000, dead_rows=dead, n_dead=cnt[10:11], stream=s),
                  restorer(full[:1], s), {"rows": cap, "dead": k})
        assert int(cnt[10]) == k
    # ---- the parent commit's route for the same work
    cols = dict(pk, seq=seq, ack=ack, flag=flag, parse_status=status_d)
    # the host procedure a second time, as the C++ host twins on host pools (std::map-free, sequential)
    ta_c, ts_c = rc.PoolTable.alloc(cap, "cpu", vals=True), rc.PoolTable.alloc(cap, "cpu", vals=False)
    ta_c.rebuild()
    ts_c.rebuild()
    c_empty = [(t, t.state.clone(), t.index.clone()) for t in (ta_c, ts_c)]
    c_work_a, c_work_s, c_swork = ta_c.add_work(u_max), ts_c.add_work(max(k, 1)), ta_c.settle_work(ts_c)
    co = {f: np.zeros(m_max, dt) for f, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
                                               ("ack", np.uint32), ("flag", np.uint8))}
    c_ar, c_sr, c_new, c_cnt = np.zeros(m_max, np.uint32), np.zeros(m_max, np.uint32), np.arange(m_max, dtype=np.uint32), np.zeros(8, np.uint32)

    def twins(h):
        rc.pool_add_host(ta_c, h["src"], h["dst"], h["sp"], h["dp"], 1000, u_max, c_work_a, seq=h["seq"], ack=h["ack"],
                         parse_status=h["parse_status"], touch=True, n_new=c_cnt[0:1])
        if pending:
            rc.pool_add_host(ts_c, tup["src"], tup["dst"], tup["sp"], tup["dp"], 1000, k, c_work_s, n_new=c_cnt[1:2])
        rc.pool_offers_host(ta_c, ts_c, rc.ConnOffers(co["src"], co["dst"], co["sp"], co["dp"], co["ack"], co["flag"], c_cnt[2:3],
                                                      m_max=m_max), offer_ack_row=c_ar, offer_sock_row=c_sr)
        # every offer became a conn and nothing was refused: the procedure does not walk miss
        rc.pool_settle_host(ta_c, ts_c, c_swork, new_offer=c_new, n_new=c_cnt[2:3], offer_ack_row=c_ar, offer_sock_row=c_sr,
                            m_max=m_max, new_max=m_max, n_closed=c_cnt[3:4])
        assert c_cnt[:3].tolist() == [k if pending else 0] * 3, c_cnt.tolist()

    def parent():
        t0 = time.perf_counter()
        h = {f: v.cpu().numpy() for f, v in cols.items()}  # D2H (synchronises)
        h = {f: (v if f == "parse_status" else v.view(f"u{v.dtype.itemsize}")) for f, v in h.items()}
        t1 = time.perf_counter()
        pool_a, pool_n = {}, {}
        syn = np.nonzero(h["parse_status"] == A.PARSE_SYN)[0]
        syn = syn[(h["sp"][syn] != 0) & (h["dp"][syn] != 0)]
        for key, sq, ak in zip(zip(h["src"][syn].tolist(), h["sp"][syn].tolist(), h["dst"][syn].tolist(), h["dp"][syn].tolist()),
                               h["seq"][syn].tolist(), h["ack"][syn].tolist()):
            rec = pool_a.get(key)
            if rec is None:
                rec = pool_a[key] = [sq, ak, 0]
            rec[2] = 1000
        if pending:
            for key in zip(tup["src"].tolist(), tup["sp"].tolist(), tup["dst"].tolist(), tup["dp"].tolist()):
                pool_n.setdefault(key, 1000)
        keys = [key for key in pool_a if key in pool_n]
        o = {"src": np.array([x[0] for x in keys], np.uint32), "sp": np.array([x[1] for x in keys], np.uint16),
             "dst": np.array([x[2] for x in keys], np.uint32), "dp": np.array([x[3] for x in keys], np.uint16),
             "ack": np.array([pool_a[x][1] for x in keys], np.uint32), "flag": np.full(len(keys), 0x10, np.uint8)}
        for key in keys:  # behind the batch: every offer became a conn
            pool_a.pop(key, None)
            pool_n.pop(key, None)
        t2 = time.perf_counter()
        on = [dev(v, device) for v in o.values()]  # H2D
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        assert len(keys) == (k if pending else 0) and len(on) == 6
        for t, st, ix in c_empty:  # outside the timed parts
            t.state.copy_(st)
            t.index.copy_(ix)
        t4 = time.perf_counter()
        twins(h)
        t5 = time.perf_counter()
        return {"d2h": (t1 - t0) * 1e3, "host_procedure_python": (t2 - t1) * 1e3, "host_procedure_twins": (t5 - t4) * 1e3,
                "h2d_offers": (t3 - t2) * 1e3}

    tm.host(f"{name}_parent_route{sfx}", parent, {"packets": n, "d2h_bytes": 22 * n, "offers": k if pending else 0})
    # ---- the yardstick: the resolve of the same batch
    tab = rc.ConnTable.alloc(cap, device, by_id=False)
    st = np.zeros(cap, np.uint8)
    st[:k] = A.CONN_LIVE | A.CONN_ALIVE
    tab.load(state=st, conn_key=(np.arange(cap, dtype=np.uint64) + 1) * np.uint64(0x9E3779B97F4A7C15))
    tab.rebuild(cx, stream=s)
    ck = dev(((conn_of.astype(np.uint64) + 1) * np.uint64(0x9E3779B97F4A7C15)), device)
    rstat = torch.full((n,), A.RECV_VALID, dtype=torch.int8, device=device)
    conn, hit, rmiss = i32(n), torch.zeros(n, dtype=torch.uint8, device=device), torch.zeros(n, dtype=torch.int8, device=device)
    tm.device(f"{name}_conn_resolve", lambda: cx.conn_resolve_batch(tab, rstat, ck, conn, hit=hit, miss=rmiss, n_miss=cnt[11:12], stream=s),
              None, {"packets": n, "conns": k})
    assert int(cnt[11]) == 0


def flush_1m(cx, device, s, tm: Timer):
    cap = 1 << 20
    tab = rc.PoolTable.alloc(cap, device, vals=True)
    tup = conn_tuples(cap)
    exp = np.where(np.arange(cap) % 5 == 0, 500, 2000).astype(np.uint64)
    tab.load(state=np.full(cap, A.POOL_LIVE, np.uint8), expiry=exp, **tup)
    tab.rebuild(cx, stream=s)
    torch.cuda.synchronize()
    full = [(tab, snapshot(tab))]
    dead = torch.zeros(cap, dtype=torch.int32, device=device)
    nd = torch.zeros(1, dtype=torch.int32, device=device)
    tm.device("pool_flush_1m_none", lambda: cx.pool_flush(tab, 499, dead_rows=dead, n_dead=nd, stream=s), None, {"rows": cap, "dead": 0})
    assert int(nd) == 0
    tm.device("pool_flush_1m_fifth", lambda: cx.pool_flush(tab, 500, dead_rows=dead, n_dead=nd, stream=s), restorer(full, s),
              {"rows": cap, "dead": (cap + 4) // 5})
    assert int(nd) == (cap + 4) // 5
    restorer(full, s)()
    tm.device("pool_index_build_1m", lambda: tab.rebuild(cx, stream=s), None, {"rows": cap})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scale", type=int, default=1, help="divide every shape by this (a rehearsal)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pool_paths.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pool_paths.py needs a GPU"
    device = torch.device("cuda:0")
    cx = rc.Codec(b"hello135", 0)
    s = torch.cuda.Stream(device)
    cx.reserve(max(n for n, _ in SHAPES.values()), stream=s)
    tm = Timer(s, args.rounds, args.reps)
    with torch.cuda.stream(s):
        for name, (n, k) in SHAPES.items():
            n, k = max(n // args.scale, 4096), max(k // args.scale, 64)
            shape(cx, device, s, name, n, k, tm, True)
            if name == "c3":
                shape(cx, device, s, name, n, k, tm, False)
        if args.scale == 1:
            flush_1m(cx, device, s, tm)
    p = tm.out
    res = {"what": "rsk_pool_add_batch / rsk_pool_offers / rsk_pool_settle_batch / rsk_pool_flush (tools/pool_paths.py): medians of "
                   f"{args.rounds} windows of {args.reps} calls, device events on a side stream; parent_route: host clock, its parts apart; "
                   "one box, one run",
           "device": torch.cuda.get_device_name(0), "scale": args.scale, "paths": p}
    chain = lambda sfx: sum(p[f"c3_pool_{c}{sfx}"]["ms"] for c in ("add", "offers", "settle"))  # noqa: E731

    def route(name):  # the parent's route with the host procedure as the C++ twins run it (the Python figure stands beside it)
        q = p[name]["parts_ms"]
        p[name]["route_twins_ms"] = round(q["d2h"] + q["host_procedure_twins"] + q["h2d_offers"], 4)
        p[name]["route_python_ms"] = round(q["d2h"] + q["host_procedure_python"] + q["h2d_offers"], 4)
        return p[name]["route_twins_ms"]
    res["c3_chain_all_pending_ms"] = round(chain(""), 4)
    res["c3_chain_none_pending_ms"] = round(chain("_none"), 4)
    res["c3_chain_all_pending_over_parent_route"] = round(chain("") / route("c3_parent_route"), 4)
    res["c3_chain_none_pending_over_parent_route_none"] = round(chain("_none") / route("c3_parent_route_none"), 4)
    res["c3_chain_all_pending_over_conn_resolve"] = round(chain("") / p["c3_conn_resolve"]["ms"], 3)
    res["c3_chain_none_pending_over_conn_resolve"] = round(chain("_none") / p["c3_conn_resolve"]["ms"], 3)
    c4 = sum(p[f"c4_pool_{c}"]["ms"] for c in ("add", "offers", "settle"))
    res["c4_chain_all_pending_ms"] = round(c4, 4)
    res["c4_chain_all_pending_over_parent_route"] = round(c4 / route("c4_parent_route"), 4)
    res["c4_chain_all_pending_over_conn_resolve"] = round(c4 / p["c4_conn_resolve"]["ms"], 3)
    res["conn_create_empty_chain_c3_ms"] = 0.053  # README: the create's own empty chain on C3
    res["c3_chain_none_pending_over_conn_create_empty_chain"] = round(chain("_none") / 0.053, 2)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in res.items() if k != "paths"}, indent=1))
    for k, v in p.items():
        print(f"{k:40s} {v['ms']:10.4f} ms")
    cx.close()


if __name__ == "__main__":
    main()
