"""A server session of many batches on the host twins against the packet walk (tests/session.py, tests/session_ref.py):
every shape x 2 seeds with the floors of what each script must exercise, the walk's deviation guards on one constructed
script each, and the chain mutants -- the documented procedure with one step broken -- each caught by a named shape."""
from __future__ import annotations

import numpy as np
import pytest

from tests import collide
from tests import session as S
from tests import session_ref as W

SEEDS = (1, 2)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_host_twins_equal_the_walk(oracle, shape, seed):
    sc = S.script(seed, shape)
    assert 12 <= len(sc["events"]) <= 16
    sizes = tuple(len(ev[1]) for ev in sc["events"] if ev[0] == "CAPTURE")
    assert sizes == S.SHAPES[shape]["sizes"], "no packet of any capture is left out"
    proofs = set()

    def prove_cluster(e, ev, chain, walk):
        """clustered: every index is ONE run from HOME that wraps -- read back from the indexes the twins keep, after
        the first ACCEPT (socket pool) and after every CAPTURE (conns, convs, what the ack pool still holds)."""
        if shape != "clustered" or ev[0] not in ("ACCEPT", "CAPTURE"):
            return
        t = chain.tables()
        sizes = {"sock": len(walk.sock_pool), "ack": len(walk.ack_pool), "conn": len(walk.conn_at), "conv": len(walk.conv_at)}
        for name in ("sock",) if ev[0] == "ACCEPT" else ("ack", "conn", "conv", "sock"):
            if sizes[name] >= 20:
                collide.one_run(t["index"][name], S.HOME, sizes[name])
                proofs.add((name, sizes[name] > 100))

    seen, trace = S.run(sc, S.ServerChain("host", sc["params"], oracle), oracle, after_event=prove_cluster)
    assert len(trace) == len(sc["events"])
    floors = S.SHAPES[shape]["floors"]
    assert sorted(floors) == sorted(S.COUNTS) == sorted(seen), "every count has a floor in every shape"
    for k, floor in floors.items():
        assert seen[k] >= floor, (shape, seed, k, seen[k], floor)
    if shape == "clustered":
        assert proofs >= {("sock", True), ("conn", True), ("conv", True), ("ack", False)}, proofs


def test_scripts_hold_the_supported_sequences():
    """What the batch chain supports and the walk agrees on must be IN the traffic: DATA behind a CONV_RST of its conv
    in one capture, a handshake and the DATA packet that uses it in one capture (the handshake first), a conn born in
    one capture answering a KEEP_ALIVE_REQ in the next, a row vacated by a close and taken by a create later."""
    sc = S.script(1, "churn")
    p = sc["params"]
    walk = W.Walk(p["cap_conn"], p["cap_conv"], p["cap_pool"], p["cap_pool"], S.PERSIST_MS)
    born_last, answered_young, same_capture = set(), 0, 0
    for ev in sc["events"]:
        if ev[0] == "ACCEPT":
            walk.accept(ev[1], ev[2])
        elif ev[0] == "SEND":
            walk.send(ev[1], ev[2], ev[3])
        elif ev[0] == "TICK":
            walk.tick(ev[1], ev[2])
            walk.send_queued(ev[3], tick=True)
        else:
            syn_at = {}
            for i, x in enumerate(ev[1]):
                if x.flags & W.TH_SYN:
                    syn_at.setdefault((x.ip_src, x.sport, x.ip_dst, x.dport), i)
            res = walk.capture(ev[1], ev[2])
            walk.send_queued(ev[3])
            answered_young += sum(1 for i, x in enumerate(ev[1]) if res["kind"][i] == W.K_KA_REQ and res["cconn"][i] in born_last)
            born_last = set(res["conn_new_rows"])
            for r in res["conn_new_rows"]:
                c = walk.conn_at[r]
                same_capture += c.tup in syn_at
    assert walk.seen["convs_reborn"] > 0 and walk.seen["rows_reused"] > 0
    assert answered_young > 0 and same_capture > 0


# ---- the guards: one constructed script per documented deviation ---------------------------------------------------
ID8 = b"group-01"
SRV, CLI = 0x0100000A, 0x1400010A


def tup(port):
    return (SRV, 443, CLI, port)


def syn(t):
    return W.Packet(t[0], t[2], t[1], t[3], 1000, 2000, 0x12)


def frame(t, cmd, key, payload=b"x", conv=5, seq=100):
    return W.Packet(t[2], t[0], t[3], t[1], seq, 1, 0x18, cmd, ID8, conv, key, payload)


def k8(key):
    return int(key).to_bytes(8, "little")


def walk_with_conn(key=77, port=2000, cap_conn=8):
    w = W.Walk(cap_conn, 8, 8, 8, 1000)
    w.accept([tup(port)], 0)
    w.capture([syn(tup(port)), frame(tup(port), W.DATA, key)], 0)
    w.send_queued([])
    assert key in w.conns[ID8]
    return w


def other_tuple(w):
    w.accept([tup(2002)], 0)
    w.capture([syn(tup(2002)), frame(tup(2001), W.DATA, 88), frame(tup(2002), W.DATA, 88)], 1)


def data_ahead_of_handshake(w):
    w.capture([frame(tup(2001), W.DATA, 88), syn(tup(2001))], 1)


def names_a_reset_conn(w):
    w.capture([frame(tup(2000), W.NETCONN_RST, 77, k8(77)), frame(tup(2000), W.KA_REQ, 77, k8(77))], 1)


def data_on_a_reset_conn(w):
    w.capture([frame(tup(2000), W.NETCONN_RST, 77, k8(77)), frame(tup(2000), W.DATA, 77)], 1)


def names_a_created_conn(w):
    w.accept([tup(2001)], 0)
    w.capture([syn(tup(2001)), frame(tup(2001), W.DATA, 88), frame(tup(2001), W.KA_REQ, 88, k8(88))], 1)


def named_before_created(w):
    w.accept([tup(2001)], 0)
    w.capture([frame(tup(2000), W.KA_REQ, 77, k8(88)), syn(tup(2001)), frame(tup(2001), W.DATA, 88)], 1)


def conv_rst_of_a_conv_born_here(w):
    w.capture([frame(tup(2000), W.DATA, 77, conv=9), frame(tup(2000), W.CONV_RST, 77, (9).to_bytes(4, "little"))], 1)


def reset_twice_with_data_between(w):
    rst = frame(tup(2000), W.CONV_RST, 77, (5).to_bytes(4, "little"))
    w.capture([rst, frame(tup(2000), W.DATA, 77, conv=5), rst], 1)


def request_on_a_new_conn(w):
    w.send([0], [0], [b"p"])  # conn 77 has sent: it is not new any more
    w.accept([tup(2001)], 15000)
    w.capture([syn(tup(2001)), frame(tup(2001), W.DATA, 88)], 15000)
    w.send_queued([])
    res = w.tick(16000, ("ka",))
    assert [m[1] for m in res["requests"]] == [77]
    w.send_queued([1], tick=True)  # the draw picks the conn born at 15000, which has never sent


def only_conn_is_the_one_to_avoid(w):
    w.pick(ID8, 0, avoid=77)


def table_runs_full(w):
    w.accept([tup(2001)], 0)
    w.capture([syn(tup(2001)), frame(tup(2001), W.DATA, 88)], 1)


DEVIATIONS = {
    "other_tuple": (other_tuple, "a refused key"),
    "data_ahead_of_handshake": (data_ahead_of_handshake, "ahead of its own handshake"),
    "names_a_reset_conn": (names_a_reset_conn, "reset or created"),
    "data_on_a_reset_conn": (data_on_a_reset_conn, "batch reset"),
    "names_a_created_conn": (names_a_created_conn, "reset or created"),
    "named_before_created": (named_before_created, "a later packet of the batch creates"),
    "conv_rst_of_a_conv_born_here": (conv_rst_of_a_conv_born_here, "born in the same batch"),
    "reset_twice_with_data_between": (reset_twice_with_data_between, "reset twice"),
    "request_on_a_new_conn": (request_on_a_new_conn, "still new"),
    "only_conn_is_the_one_to_avoid": (only_conn_is_the_one_to_avoid, "the one to avoid"),
    "table_runs_full": (table_runs_full, "runs full"),
}


@pytest.mark.parametrize("name", sorted(DEVIATIONS))
def test_walk_raises_on_a_deviation(name):
    fn, words = DEVIATIONS[name]
    w = walk_with_conn(cap_conn=1 if name == "table_runs_full" else 8)
    with pytest.raises(W.SessionDeviation, match=words):
        fn(w)


def test_walk_accepts_the_neighbours_of_the_deviations():
    """The same packets in the order the batch chain supports raise nothing: the guards fire on the deviation alone."""
    w = walk_with_conn()
    w.accept([tup(2001)], 0)
    rst = frame(tup(2000), W.CONV_RST, 77, (5).to_bytes(4, "little"))
    res = w.capture([syn(tup(2001)), frame(tup(2001), W.DATA, 88), frame(tup(2001), W.DATA, 88, seq=50), frame(tup(2000), W.KA_REQ, 77, k8(77)),
                     frame(tup(2000), W.DATA, 77), rst, frame(tup(2000), W.DATA, 77)], 1)
    assert res["counts"]["n_new"] == 1 and res["counts"]["v_reborn"] == 1 and res["counts"]["v_closed"] == 1
    assert res["conn"][1] == res["conn"][2] != W.NONE and [m[0] for m in res["messages"]] == [W.KA_RESP]
    w.send_queued([0])
    res = w.capture([rst, rst], 2)  # a second reset with no DATA between finds nothing
    assert res["counts"]["v_closed"] == 1 and res["counts"]["n_rst_again"] == 1 and res["conv_row"][1] == W.NONE


# ---- the chain mutants: the documented procedure with one step broken ----------------------------------------------
# mutant -> (the shape that must catch it, the comparison that must see it: a pattern of the assertion's text).  A
# mutant that survives its shape, or dies of anything else, means the scripts or the checks are too weak.
CAUGHT_BY = {
    # the acks of the conns born in a batch lack their own packets
    "no_second_recv_ack": ("steady", r"CAPTURE', 'conn', 'row', \d+, 'ack'"),
    # the pick index goes stale: an answer travels on a conn the batch killed
    "close_without_pick": ("churn", r"'send', \d+, 'conn'|'pick'"),
    # a reset conv's row stays LIVE
    "hold_not_cleared": ("churn", r"'conv', 'the LIVE rows'"),
    # RSK_CONN_NEW stays set behind the conn's first send
    "new_never_cleared": ("steady", r"SEND', 'conn', 'row', \d+, 'state', 7, 3"),
    # the add's n_new is not the create's when a handshake precedes its DATA by a batch: pool rows stay, sockets are not bound
    "settle_with_add_n_new": ("churn", r"'sockets bound'|'(ack|sock)', 'the LIVE rows'"),
    # the packets of the conns born in the batch reach no conv
    "conv_resolve_with_old_hit": ("steady", r"CAPTURE', 'conv_row'"),
    # the second create hands a vacated row to another key inside the batch
    "conv_close_without_hold": ("skew", r"CAPTURE', 'conv_row'"),
    # accepted sockets nobody asked for are never closed
    "no_sock_flush": ("churn", r"TICK', 'sock_dead'"),
}


def test_every_mutant_is_listed():
    assert sorted(CAUGHT_BY) == sorted(S.MUTANTS)


@pytest.mark.parametrize("mutant", sorted(S.MUTANTS))
def test_chain_mutant_is_caught(oracle, mutant):
    shape, sees = CAUGHT_BY[mutant]
    sc = S.script(1, shape)
    with pytest.raises(AssertionError, match=sees):
        S.run(sc, S.ServerChain("host", sc["params"], oracle, mutant=mutant), oracle)


# ---- split invariance on the host twins (the GPU test runs the same on the device) ---------------------------------
@pytest.mark.parametrize("shape", ["churn", "shrinking"])
def test_split_invariance_on_the_host_twins(oracle, shape):
    sc = S.script(1, shape)
    cuts = [ev[4] for ev in sc["events"] if ev[0] == "CAPTURE"]
    assert all(1 <= len(c) <= 4 for c, n in zip(cuts, S.SHAPES[shape]["sizes"]) if n >= 63), "a capture without a safe cut"
    n = S.run_split(sc, S.ServerChain("host", sc["params"], oracle), S.ServerChain("host", sc["params"], oracle), oracle)
    assert n == sum(len(c) + 1 for c in cuts)


def test_fixed_buffers_on_the_host_twins(oracle):
    """What the graph side of the device runs -- every capture as the packets of the largest one, the rest with wire
    length 0, over buffers that never move -- on the host twins against the walk: the padding changes nothing."""
    sc = S.script(1, "churn")
    caps = [e for e, ev in enumerate(sc["events"]) if ev[0] == "CAPTURE"]
    chain = S.ServerChain("host", sc["params"], oracle, fixed=max(len(sc["events"][e][1]) for e in caps),
                          arena_max=max(len(S.frames_of(oracle, sc, e)[0]) for e in caps))
    S.run(sc, chain, oracle)
    assert len(chain.kept) > 40
