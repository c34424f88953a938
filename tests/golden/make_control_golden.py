#!/usr/bin/env python3
"""Generates tests/golden/control.npz from the REFERENCE's own control path, keepalive timer, send pick and
conv flush (oracle/_ref/librsk_ref_control.so: IAppGroup / INetGroup / ConnReset / NetConnKeepAlive / IGroup /
IConn compiled from the reference by `make -C oracle ref`; oracle/ref_control_harness.cpp).  Run in the build
container:

    make -C oracle ref && python tests/golden/make_control_golden.py

Each case stores its inputs and what the reference did with them (tests/control_golden.py: reference_*).
Data only.  Prints per case: packets / steps, control packets, sends, removals and draws consumed.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import control_golden as G  # noqa: E402
from tests.oracle_lib import RefControl  # noqa: E402

T0 = 1 << 40
DELAY = 15000


def tcp_keys(rng, n):
    """n distinct KeyForTcp values (KeyGenerator.cpp:16-25)."""
    out = set()
    while len(out) < n:
        out.add(0x10000000 | (int(rng.integers(10001, 10006)) << 16) | int(rng.integers(1024, 65536)))
    return np.array(sorted(out, key=lambda k: int(rng.integers(0, 2**31))), np.uint64)


def digit_keys(rng, n):
    """n distinct IntKeys of 1 to 12 digits, 9 / 10 / 99 / 100 among them: string order != numeric order."""
    out = [9, 10, 99, 100, 5, 1000, 12, 123456789012, 2, 19][:n]
    seen = set(out)
    while len(out) < n:
        k = int(rng.integers(1, 10 ** int(rng.integers(1, 13))))
        if k not in seen:
            seen.add(k)
            out.append(k)
    return np.array(out, np.uint64)


def group_id(rng):
    return rng.integers(1, 256, 8).astype(np.uint8)


# ---- the control walk -------------------------------------------------------------------------------------------
def walk_case(rng, shape, n_conn, n, script=None, sends=True):
    keys = tcp_keys(rng, n_conn)
    n_unk = max(3, n_conn // 4)
    pool = np.concatenate([keys, tcp_keys(rng, n_conn + n_unk)[:n_unk] ^ np.uint64(1 << 40)])
    safe = np.arange(0, n_conn, 2)            # conns no reset names: DATA goes to these
    risky = np.arange(1, n_conn, 2) if n_conn > 1 else np.arange(1)
    unk = np.arange(n_conn, len(pool))
    hot = risky[:max(1, len(risky) // 4)]     # named again and again
    status = rng.choice(np.array([1] * 14 + [0, -1], np.int8), n)
    menu = [0] * 9 + [1, 2, 2, 3, 3, 3, 3, 4, 4, 4] if sends else [0] * 9 + [1, 2, 2, 2, 4, 4, 4, 4]
    cmd = rng.choice(np.array(menu, np.uint8), n)
    odd = rng.random(n) < 0.03
    cmd[odd] = rng.choice(np.array([5, 9, 255], np.uint8), int(odd.sum()))
    for e in (0, 2047, 2048, 2049, 4095, 4096, n - 1):  # control packets at the tile edges
        if 0 <= e < n:
            status[e] = 1
            cmd[e] = [3, 2, 4][e % 3] if sends else [2, 4][e % 2]
    bk, ck = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    u = rng.random(n)
    pick = lambda a: a[rng.integers(0, len(a), n)]  # noqa: E731
    any_known = np.where(rng.random(n) < 0.5, pick(np.arange(n_conn)), pick(hot))
    bk[:] = np.where(u < 0.7, np.where(cmd == 2, np.where(rng.random(n) < 0.6, pick(hot), pick(risky)), any_known), pick(unk))
    ck[:] = np.where((rng.random(n) < 0.85) | (not sends), pick(safe), pick(unk))
    force8 = np.zeros(n, np.uint8)  # scripted packets carry a full body whatever length their turn would deal
    if script is not None:  # (offset, cmd, pool index) placed over the middle of the batch
        at0 = n // 3
        for off, cm, k in script:
            status[at0 + off], cmd[at0 + off], bk[at0 + off], force8[at0 + off] = 1, cm, k, 1
    req = rng.permutation(n_conn)[:(n_conn + 1) // 2]
    c = {"shape": np.int32(shape), "id": group_id(rng), "keys": keys, "pool": pool, "req_conn": req.astype(np.int16),
         "req_tries": rng.integers(0, 3, len(req)).astype(np.uint8), "status": status, "cmd": cmd, "bk": bk, "ck": ck, "force8": force8,
         "seed": np.uint64(rng.integers(1, 2**62)), "n_draws": np.uint32(int((status == 1).sum()) + n_conn + 8)}
    return c


def snapshot_script(k, other, gap):
    """RST K; KA_REQ K; KA_RESP K; RST K; then requests of another key (answers are sent: doSend may draw the dead
    K); then KA_REQ K, KA_RESP K and RST K once more."""
    s = [(0, 2, k), (1 * gap, 3, k), (2 * gap, 4, k), (3 * gap, 2, k)]
    s += [(3 * gap + 1 + j, 3, other) for j in range(gap - 1)]
    s += [(5 * gap, 3, k), (6 * gap, 4, k), (7 * gap, 2, k)]
    return s


def walk_cases(ref):
    rng = np.random.default_rng(0xC0A1)
    out = []
    for n, n_conn in ((1, 10), (2047, 37), (2048, 300), (2049, 64), (4097, 120)):
        for shape in (G.SERVER, G.CLIENT):
            gap = 1 if n < 100 else 9
            sc = snapshot_script(1, 3, gap) if n > 100 else None
            out.append((f"{'server' if shape == G.SERVER else 'client'}_{n}", walk_case(rng, shape, n_conn, n, script=sc)))
    # the snapshot question on small batches: one that sends nothing, one whose answers draw the dead conn
    c = walk_case(rng, G.CLIENT, 10, 400, sends=False)
    c["ck"][:] = np.arange(400) % 5 * 2  # DATA of known keys only: no miss, nothing is sent
    out.append(("client_rst_nothing_sent", c))
    for shape, name in ((G.CLIENT, "client_rst_then_sends"), (G.SERVER, "server_rst_then_sends")):
        while True:  # draws (a seed) with which the dead conn outlives the first round of packets and not the second
            c = walk_case(rng, shape, 12, 300, script=snapshot_script(1, 2, 6))
            look = G.reference_walk(ref, c)["look"]
            pk = np.nonzero((c["bk"] == 1) & (c["force8"] == 1))[0]
            if look[pk[[0, 1, 3]]].tolist() == [1, 1, 1] and look[pk[4]] == -1:
                break
        out.append((name, c))
    return out


# ---- the keepalive timer ------------------------------------------------------------------------------------------
def timer_case(rng, shape, n_conn, n_extra=3):
    keys = tcp_keys(rng, n_conn + n_extra)
    keys, extra = keys[:n_conn], keys[n_conn:]
    flags = np.full(n_conn, G.F_ALIVE, np.uint8)
    flags[rng.random(n_conn) < 0.1] |= G.F_NEW
    est = (T0 - rng.integers(0, 2 * DELAY, n_conn)).astype(np.uint64)
    diffs = [0, 1, 14999, 15000, 2**31 - 1, 2**31, 2**32 + 14999, 2**32 + 15000, -500, -1]
    if n_conn >= 2 * len(diffs):
        at = rng.permutation(n_conn)[:2 * len(diffs)]
        est[at] = np.array([T0 - d for d in diffs] * 2, np.uint64)
        flags[at] = G.F_ALIVE
    elif n_conn == 1:
        est[0] = T0 - DELAY
        flags[0] = G.F_ALIVE
    carrier = None
    if n_conn > 1:  # mConns.begin(): every draw is 0, so this conn carries every request; it never asks itself
        carrier = min(range(n_conn), key=lambda k: str(int(keys[k])))
        flags[carrier], est[carrier] = G.F_ALIVE, 1 << 62
    has = rng.permutation(n_conn)[:max(1, n_conn // 3)]
    has = has[has != carrier] if carrier is not None else has
    req_key = np.concatenate([has, n_conn + np.arange(n_extra)]).astype(np.int16)
    req_tries = rng.integers(0, 3, len(req_key)).astype(np.uint8)
    op, arg = [], []

    def step(o, a=0):
        op.append(o)
        arg.append(a)

    def flush(k):
        step(G.OP_FLUSH, T0 + 1000 * k)
        step(G.OP_GROUP_FLUSH, T0 + 1000 * k)

    idx = np.arange(n_conn)
    flush(0)
    flush(1)
    for k in idx[idx % 3 == 0].tolist() + [n_conn]:  # responses: with an entry, without, and for a key with no conn
        if k != carrier:
            step(G.OP_RESP, k)
    flush(2)
    for k in idx[idx % 7 == 1].tolist():  # conns removed, many with an entry
        if k != carrier:
            step(G.OP_REMOVE, k)
    for k in idx[(idx % 2 == 0) & ((flags & G.F_NEW) != 0)].tolist():
        step(G.OP_CLEAR_NEW, k)
    flush(3)
    step(G.OP_ONLINE, 0)
    flush(4)
    step(G.OP_ONLINE, 1)
    flush(5)
    flush(6)
    flushes = 7
    return {"shape": np.int32(shape), "id": group_id(rng), "keys": keys, "extra": extra, "flags": flags, "est": est,
            "req_key": req_key, "req_tries": req_tries, "online": np.int32(1), "op": np.array(op, np.uint8),
            "arg": np.array(arg, np.uint64), "draws": np.zeros(flushes * n_conn + 8, np.uint32)}


def timer_cases():
    rng = np.random.default_rng(0x71E2)
    out = [(f"{'server' if s == G.SERVER else 'client'}_{n}", timer_case(rng, s, n))
           for n, s in ((1, G.CLIENT), (1023, G.SERVER), (1024, G.CLIENT), (1025, G.CLIENT), (2049, G.SERVER))]
    # offline from the start, with stale entries (some of keys that have no conn); online again after two flushes
    c = timer_case(rng, G.CLIENT, 12)
    c["online"] = np.int32(0)
    f = lambda t: [(G.OP_FLUSH, t), (G.OP_GROUP_FLUSH, t)]  # noqa: E731
    steps = f(T0) + [(G.OP_REMOVE, int(c["req_key"][0]))] + f(T0 + 1000) + [(G.OP_ONLINE, 1)] + f(T0 + 2000) + f(T0 + 3000)
    c["op"], c["arg"] = np.array([s[0] for s in steps], np.uint8), np.array([s[1] for s in steps], np.uint64)
    out.append(("client_offline_stale", c))
    # one conn dead from the start and drawn by the first request's doSend: removed in the middle of the flush
    c = timer_case(rng, G.CLIENT, 10)
    order = sorted(range(10), key=lambda k: str(int(c["keys"][k])))
    dead = order[4]
    c["flags"][dead] = 0
    c["flags"][order[0]] = G.F_ALIVE
    c["est"][dead] = T0 - DELAY - 5
    steps = f(T0) + f(T0 + 1000) + f(T0 + 2000) + f(T0 + 3000)
    c["op"], c["arg"] = np.array([s[0] for s in steps], np.uint8), np.array([s[1] for s in steps], np.uint64)
    c["draws"] = np.zeros(64, np.uint32)
    c["draws"][0] = 4
    out.append(("client_dead_conn", c))
    return out


# ---- doSend -----------------------------------------------------------------------------------------------------
def send_case(rng, shape, n_conn, n, dead=0, avoid="none"):
    keys = digit_keys(rng, n_conn)
    extra = np.array([10**13 + 7, 3 * 10**13 + 1], np.uint64)  # longer than any key of the group
    assert not np.isin(extra, keys).any()
    flags = np.full(n_conn, G.F_ALIVE, np.uint8)
    if dead:
        flags[rng.permutation(n_conn)[:dead]] = 0
    av = np.full(n, -1, np.int32)
    if avoid == "outside":
        av[rng.random(n) < 0.4] = n_conn
    elif avoid == "one":
        av[:] = 4
    elif avoid == "inside":
        m = rng.random(n) < 0.4
        av[m] = rng.integers(0, n_conn + 1, int(m.sum()))
    return {"shape": np.int32(shape), "id": group_id(rng), "keys": keys, "extra": extra, "flags": flags, "avoid": av,
            "seed": np.uint64(rng.integers(1, 2**62)), "n_draws": np.uint32(2 * n + n_conn + 64)}


def send_cases():
    rng = np.random.default_rng(0x5E2D)
    out = []
    for n_conn, n in ((1, 1), (2, 63), (10, 64), (10, 65), (64, 2047), (1024, 2048), (1024, 4097), (1025, 2049), (1025, 4097)):
        shape = G.SERVER if (n_conn, n) in ((10, 65), (64, 2047)) else G.CLIENT
        out.append((f"alive_{n_conn}_{n}", send_case(rng, shape, n_conn, n)))
    for n_conn, n in ((10, 65), (64, 2049), (1024, 2048)):
        out.append((f"avoid_outside_{n_conn}_{n}", send_case(rng, G.CLIENT, n_conn, n, avoid="outside")))
    out.append(("avoid_one_10_65536", send_case(rng, G.CLIENT, 10, 65536, avoid="one")))
    out.append(("dead3_10_4097", send_case(rng, G.CLIENT, 10, 4097, dead=3, avoid="inside")))
    out.append(("dead3_server_10_2049", send_case(rng, G.SERVER, 10, 2049, dead=3, avoid="inside")))
    out.append(("all_dead_3_5", send_case(rng, G.CLIENT, 3, 5, dead=3)))
    return out


# ---- the conv flush -----------------------------------------------------------------------------------------------
def flush_case(rng, shape, nc, rounds=5):
    convs = (rng.permutation(4 * nc + 7)[:nc] + 1).astype(np.uint32)
    kind = np.arange(nc) % 8 if nc > 1 else np.array([5])
    in_off, out_off, in_leaf, out_leaf, out_ret = [0], [0], [], [], []
    for r in range(rounds):
        for leaf in (range(nc) if r % 2 == 0 else range(nc - 1, -1, -1)):  # in order: the fixture stays small
            k = int(kind[leaf])
            here = {0: True, 1: r < 2, 2: r < 2, 3: False, 4: r < 4, 5: True, 6: True, 7: True}[k]  # still in the group
            if not here:
                continue
            quiet = (k == 5 and r == 3)
            n_in = 0 if k in (2, 3) or quiet else (3 if k == 7 else 1)
            in_leaf += [leaf] * n_in
            if k in (1, 3) or quiet:
                rets = []
            elif k == 4 and r == 2:
                rets = [0, -1]           # sends that fail: they must not count
            elif k == 6:
                rets = [0, 32, -1][: 2 + r % 2] if r % 2 else [-1, 1400]
            elif k == 7:
                rets = [32, 32]
            else:
                rets = [32]
            out_leaf += [leaf] * len(rets)
            out_ret += rets
        in_off.append(len(in_leaf))
        out_off.append(len(out_leaf))
    return {"shape": np.int32(shape), "id": group_id(rng), "net_key": tcp_keys(rng, 1), "convs": convs,
            "in_off": np.array(in_off, np.uint32), "in_leaf": np.array(in_leaf, np.uint16), "out_off": np.array(out_off, np.uint32),
            "out_leaf": np.array(out_leaf, np.uint16), "out_ret": np.array(out_ret, np.int16),
            "now": (T0 + 1000 * np.arange(rounds)).astype(np.uint64)}


def flush_cases():
    rng = np.random.default_rng(0xF1A5)
    return [(f"{'server' if s == G.SERVER else 'client'}_{n}", flush_case(rng, s, n))
            for n, s in ((1, G.CLIENT), (1023, G.SERVER), (1024, G.CLIENT), (1025, G.SERVER), (2049, G.CLIENT))]


def main():
    ref = RefControl()
    out = {}
    for family, cases, run in (("walk", walk_cases(ref), G.reference_walk), ("timer", timer_cases(), G.reference_timer),
                               ("send", send_cases(), G.reference_send), ("flush", flush_cases(), G.reference_flush)):
        out[family + "_names"] = np.array([name for name, _ in cases])
        for ci, (name, c) in enumerate(cases):
            res = run(ref, c)
            c.update(res)
            out.update({f"{family[0]}{ci}_{k}": v for k, v in G.pack(c).items()})
            if family == "walk":
                v = c["status"] == 1
                print(f"walk {name}: packets={len(v)} valid={int(v.sum())} control={int((v & (c['cmd'] != 0)).sum())} "
                      f"sends={len(res['msg_src'])} notified={len(res['nt_pkt'])} removals={len(res['rm_conn'])} "
                      f"draws={int(res['draws_used'])}")
            elif family == "timer":
                print(f"timer {name}: conns={len(c['keys'])} steps={len(c['op'])} flushes={int((c['op'] == 0).sum())} "
                      f"sends={len(res['snd_key'])} timeouts={len(res['nt_conn'])} removals={len(res['rm_conn'])} "
                      f"draws={int(res['draws_used'])}")
            elif family == "send":
                print(f"send {name}: conns={len(c['keys'])} sends={len(c['avoid'])} no_conn={int((res['sender'] < 0).sum())} "
                      f"removals={len(res['rm_conn'])} draws={int(res['draws_used'])}")
            else:
                print(f"flush {name}: convs={len(c['convs'])} packets={len(c['in_leaf'])} sends={len(c['out_leaf'])} "
                      f"closed={len(res['cl_leaf'])} alive_last={int((res['alive'][-1] == 1).sum())}")
    # confirmed here before the fixture is written: the reference's own picks of the 65,536-send case are uniform
    c = G.case("send", "avoid_one_10_65536", out)
    G.check_uniform(c["sender"], [k for k in range(10) if k != 4])
    path = os.path.join(HERE, "control.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
