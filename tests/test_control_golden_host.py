"""CPU: the control walk, the keepalive timer, doSend's pick and the conv flush pinned to the REFERENCE's own
classes (tests/golden/control.npz, recorded by tests/golden/make_control_golden.py from
oracle/_ref/librsk_ref_control.so).  The host twins (rsk_control_host, rsk_keepalive_flush_host,
rsk_conn_pick_host, rsk_conv_resolve / send / flush_host) and the Python models of tests/control_ref,
tests/pick_ref and tests/conv_ref run the scenarios of tests/control_golden.py; tests/test_gpu_control_golden.py
runs the same scenarios on the device.  Where oracle/_ref is built, the harness is run again on the stored
inputs and must reproduce the stored results."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import control_golden as G
from tests import control_ref as C
from tests import pick_ref as P
from tests.oracle_lib import RefControl, ref_control_available

needs_ref = pytest.mark.skipif(not ref_control_available(), reason="oracle/_ref not built (no reference sources)")


@pytest.fixture(scope="module")
def ref():
    return RefControl()


# ---- the fixture still is what the reference does ---------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("family,run,results", [
    ("walk", G.reference_walk, G.WALK_RESULTS), ("timer", G.reference_timer, G.TIMER_RESULTS),
    ("send", G.reference_send, G.SEND_RESULTS), ("flush", G.reference_flush, G.FLUSH_RESULTS)])
def test_reference_reproduces_fixture(ref, family, run, results):
    for name in G.names(family):
        c = G.case(family, name)
        got = run(ref, {k: v for k, v in c.items() if k not in results})
        assert set(got) == set(results)
        for k in results:
            assert np.array_equal(np.asarray(got[k]), c[k]), (family, name, k)


def test_fixture_covers_what_it_is_for():
    """The shapes the cases were chosen for are in the recorded results."""
    sizes = {len(G.case("walk", n)["cmd"]) for n in G.names("walk")}
    assert sizes >= {1, 2047, 2048, 2049, 4097}
    c = G.case("walk", "client_4097")
    ctl = (c["status"] == 1) & (c["cmd"] >= 1) & (c["cmd"] <= 4)
    lens = G.walk_pay_len(c)
    seen = {(int(m), int(ln)) for m, ln in zip(c["cmd"][ctl], lens[ctl])}
    assert seen >= {(m, ln) for m in (1, 2, 3, 4) for ln in (0, 3, 4, 7, 8, 9, 12)}
    assert bool(ctl[[2047, 2048, 2049, 4095, 4096]].all()) and int((c["cmd"] > 4).sum()) > 0
    assert int((c["ret"] == G.ERR_NO_CONN).sum()) > 0 and len(c["rm_conn"]) > 0
    assert {len(G.case("timer", n)["keys"]) for n in G.names("timer")} >= {1, 1023, 1024, 1025, 2049}
    assert {len(G.case("flush", n)["convs"]) for n in G.names("flush")} >= {1, 1023, 1024, 1025, 2049}
    assert {len(G.case("send", n)["keys"]) for n in G.names("send")} >= {1, 2, 10, 64, 1024, 1025}
    assert {len(G.case("send", n)["avoid"]) for n in G.names("send")} >= {1, 63, 64, 65, 2047, 2048, 2049, 4097, 65536}
    c = G.case("timer", "server_2049")
    d = (int(c["arg"][0]) - c["est"].astype(object))
    assert set(d.tolist()) >= {0, 1, 14999, 15000, 2**31 - 1, 2**31, 2**32 + 14999, 2**32 + 15000, -1}


# ---- the control walk -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.names("walk"))
def test_host_walk(name):
    G.scenario_walk(rc, name, "cpu")


def test_snapshot_question():
    """What the reference does to later packets after a NETCONN_RST hit: NotifyErr only marks the conn dead
    (INetConn.cpp:49-52); it stays in mConnMap and is found -- a KEEP_ALIVE_REQ is answered with a RESP, a
    second reset notifies again -- until a doSend draws it and removes it (INetGroup.cpp:129-130)."""
    s = G.scenario_walk(rc, "client_rst_nothing_sent", "cpu")
    assert s["n_msg"] == 0 and s["n_removed"] == 0 and s["n_gone"] == 0
    assert s["n_late"] > 20 and s["n_late_found"] == s["n_late"]  # nothing sent: the snapshot IS the reference
    for name in ("client_rst_then_sends", "server_rst_then_sends"):
        s = G.scenario_walk(rc, name, "cpu")
        assert s["n_removed"] > 0 and s["n_gone"] > 0 and 0 < s["n_late_found"] < s["n_late"]
    c = G.case("walk", "client_rst_then_sends")
    k = 1  # the scripted conn: reset, asked, answered, reset again, removed by an answer's doSend, asked again
    pk = np.nonzero((c["bk"] == k) & (c["force8"] == 1))[0]
    first_rst, req1, _resp1, rst2 = pk[:4]
    assert c["look"][[first_rst, req1, rst2]].tolist() == [k, k, k]
    assert c["msg_cmd"][c["msg_src"] == req1].tolist() == [A.CMD_KEEP_ALIVE_RESP]
    assert int(((c["nt_conn"] == k) & (c["nt_pkt"] == rst2)).sum()) == 1  # the second reset notifies again


@pytest.mark.parametrize("name", G.names("walk"))
def test_sequential_model_on_the_fixture(name):
    """control_ref.sequential_ref with the removals the reference recorded: every lookup of the reference's
    walk.  Removing at the reset instead (what the model did before it was held against the reference) is not
    the reference's walk."""
    from tests import conn_ref as CR

    c = G.case("walk", name)
    by_id = int(c["shape"]) == G.SERVER
    n = len(c["cmd"])
    cols, _cap, row = G.walk_table(c)
    tmap, _ = CR.table_map(cols["state"], cols["conn_key"], cols["id"])
    b = dict(status=c["status"], cmd=c["cmd"], id=np.tile(np.ascontiguousarray(c["id"], np.uint8), n),
             conn_key=c["pool"][c["ck"]], tcp_sp=None, tcp_dp=None, miss=None)
    b.update(G.frames(c))
    idw = G.id_word(c) if by_id else 0
    removed = {(idw, int(c["keys"][k])): int(p) for k, p in zip(c["rm_conn"], c["rm_pkt"])}
    _k, _a, seq = C.sequential_ref(b, tmap, by_id, removed_at=removed)
    look = c["look"].astype(np.int64)
    want = np.where(look >= 0, row[np.maximum(look, 0)], G.NONE).astype(np.uint32)
    keyed = look > -2
    assert np.array_equal(seq[keyed], want[keyed]) and bool((seq[~keyed] == G.NONE).all())
    if name == "client_rst_nothing_sent":
        assert not removed
        _k, _a, old = C.sequential_ref(b, tmap, by_id, removed_at=C.AT_RESET)
        assert not np.array_equal(old[keyed], want[keyed])


# ---- the timer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.names("timer"))
def test_host_timer(name):
    s = G.scenario_timer(rc, name, "cpu")
    assert s["flushes"] >= 4 and s["sent"] > 0


def test_flush_model_on_the_fixture():
    """control_ref.flush_ref, the dict walk of OnFlush, against the reference's own mReqMap per flush."""
    for name in G.names("timer"):
        c = G.case("timer", name)
        nk, ne = len(c["keys"]), len(c["extra"])
        state = np.zeros(nk + ne, np.uint8)
        fl = c["flags"]
        state[:nk] = A.CONN_LIVE | np.where(fl & G.F_ALIVE, A.CONN_ALIVE, 0) | np.where(fl & G.F_NEW, A.CONN_NEW, 0)
        est = np.concatenate([c["est"], np.zeros(ne, np.uint64)])
        req = {int(k): int(t) for k, t in zip(c["req_key"], c["req_tries"])}
        online = bool(c["online"])
        for s, (op, arg) in enumerate(zip(c["op"].tolist(), c["arg"].tolist())):
            if op == G.OP_FLUSH:
                sent, dead = C.flush_ref(req, state, est, int(arg), A.KA_REQUEST_DELAY_MS, A.KA_MAX_RETRY, online)
                assert sorted(sent) == sorted(c["snd_key"][c["snd_step"] == s].tolist()), (name, s)
                assert sorted(dead) == sorted(c["nt_conn"][c["nt_step"] == s].tolist()), (name, s)
                at = c["snap_step"] == s
                assert req == dict(zip(c["snap_key"][at].tolist(), c["snap_tries"][at].tolist())), (name, s)
                state[c["snd_conn"][(c["snd_step"] == s) & (c["snd_conn"] >= 0)]] &= np.uint8(~A.CONN_NEW & 0xFF)
            elif op == G.OP_RESP:
                req.pop(int(arg), None)
            elif op == G.OP_REMOVE:
                state[arg] = 0
            elif op == G.OP_CLEAR_NEW:
                state[arg] &= np.uint8(~A.CONN_NEW & 0xFF)
            elif op == G.OP_ONLINE:
                online = bool(arg)
                req.clear()
            state[c["rm_conn"][c["rm_step"] == s]] = 0


# ---- doSend ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.names("send"))
def test_host_send(name):
    s = G.scenario_send(rc, name, "cpu")
    if name.startswith("alive_") and not name.startswith("alive_1_"):
        assert s["exact"] and s["differ"] > 0


def test_dosend_walk_model_on_the_fixture():
    """pick_ref.dosend_walk over the group in mConns order: the reference's senders, draws and removals."""
    for name in G.names("send"):
        c = G.case("send", name)
        if len(c["avoid"]) > 5000:
            continue
        avoid, _ = G.send_inputs(c)
        conns = [[int(k), int(c["keys"][k]), bool(c["flags"][k] & G.F_ALIVE)] for k in c["order"]]
        d = G.case_draws(c).tolist()
        used = [0]

        def draws():
            while True:
                used[0] += 1
                yield d[used[0] - 1]

        it = draws()
        got = [P.dosend_walk(conns, it, key_of_conn_to_reset=int(a)) for a in avoid]
        want = np.where(c["sender"] >= 0, c["sender"], G.ERR_NO_CONN)
        assert got == want.tolist() and used[0] == int(c["draws_used"]), name


def test_uniform_65536():
    """The 65,536-send case: the reference's own picks and the host twin's, each allowed conn within 5 sigma."""
    c = G.case("send", "avoid_one_10_65536")
    allowed = [k for k in range(10) if k != 4]
    G.check_uniform(c["sender"], allowed)
    s = G.scenario_send(rc, "avoid_one_10_65536", "cpu")
    G.check_uniform(s["conn"], s["row"][allowed])


# ---- the conv flush -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", G.names("flush"))
def test_host_flush(name):
    s = G.scenario_flush(rc, name, "cpu")
    assert s["closed"] > 0
