"""CPU: rsk_conn_create_host with the host procedure INTEGRATION.md documents around it, and
tests/conn_create_ref.create_ref, held to tests/golden/conncreate.npz: what the REFERENCE's own RawTcp, TcpAckPool,
ServerNetManager, SNetGroup, INetGroup and FakeTcp did with the same scripts (tests/conncreate_golden.py).  The
mutant models show that the fixture sees each rule: each one bends one rule and must be caught, at the script and
by the comparison named here.  The client's dial sequence holds the list form.  Where the reference is built, a
fresh run of it must reproduce the fixture."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_create_ref as R
from tests import conncreate_golden as G

SMALL = [n for n in G.names() if len(G.script(n)["d_key"]) < 100]


def test_fixture_coverage():
    names = G.names()
    sizes = {int(hi - lo) for n in names for k, _t, lo, hi, _a in G.events(G.script(n)) if k == G.EV_DATA}
    assert {1, 63, 64, 65, 2047, 2048, 2049, 4097} <= sizes
    assert {int(G.script(n)["n_groups"]) for n in names} == {1, 3, 65}
    assert G.names(deviation=True) == ["deviation_other_tuple"]
    for n in names:
        s = G.script(n)
        assert len(s["c_key"]) < int(s["capacity"]) <= 4097
    # the conn's flag is TcpInfo's member default, whatever the handshake and the DATA packet carried
    flags = np.concatenate([G.script(n)["c_info"][:, 6] for n in names])
    assert len(flags) > 7000 and bool((flags == G.TH_ACK).all())
    assert bool((np.concatenate([G.script(n)["syn_flags"] for n in names]) & G.TH_SYN).all())
    # a socket without a handshake costs the reference 500 ms: at most 8 in the fixture
    waits = 0
    for n in names:
        s = G.script(n)
        closed = np.concatenate([[0], s["closed"]]).astype(np.int64)
        waits += sum(int(closed[e + 1] - closed[e]) for e, (k, *_r) in enumerate(G.events(s)) if k == G.EV_DATA)
    assert 3 <= waits <= 8, waits


@pytest.mark.parametrize("name", G.names())
def test_host_twin_equals_the_reference(name, oracle):
    s = G.script(name)
    for cap in G.capacities(s):
        seen = G.check(s, G.Twin(rc, cap, "cpu", None, oracle))
        assert seen["packets"] == len(s["d_key"]) and seen["conns"] == len(s["c_key"])
        assert seen["snapshots"] == len(s["ev_kind"]) and seen["sends"] == len(s["s_draws"])


@pytest.mark.parametrize("walk", [False, True])
@pytest.mark.parametrize("name", G.names())
def test_restatement_equals_the_reference(name, walk, oracle):
    """create_ref, and the packet walk the mutants bend, unbent."""
    s = G.script(name)
    if walk and len(s["d_key"]) >= 100:
        s_cap = [int(s["capacity"])]
    else:
        s_cap = G.capacities(s)
    for cap in s_cap:
        assert G.check(s, G.Model(cap, oracle, walk=walk))["conns"] == len(s["c_key"])


# mutant -> (script, what the checker's first complaint names)
CAUGHT = {
    "flag_from_syn": ("refused_syn", "row"),                       # finding 1: the conn's flag is not the handshake's
    "last_syn_wins": ("repeated_syn", "ack pool after event"),     # finding 3
    "no_purge": ("half_offers", "ack pool after event"),           # finding 2: a refusal empties the tuple's entries
    "unreversed": ("orientation", "ack pool after event"),         # finding 4: the pooled record is Reverse()d
    "ack_from_seq": ("edges", "row"),                              # finding 4: which of the record's two numbers
    "retry_refused": ("deviation_other_tuple", "n_new"),           # the reference's own walk: the documented deviation
    "second_key_takes": ("two_keys", "n_new"),
    "swapped_addresses": ("sends", "row"),
}


@pytest.mark.parametrize("mutant", G.MUTANTS)
def test_each_mutant_is_caught_for_its_own_reason(mutant, oracle):
    name, reason = CAUGHT[mutant]
    s = G.script(name)
    with pytest.raises(AssertionError) as err:
        G.check(s, G.Model(int(s["capacity"]), oracle, mutant=mutant), mutant=mutant)
    first = err.value.args[0]
    assert (first[0] if isinstance(first, tuple) else first) == reason, err.value
    # and nowhere is a mutant the fixture's equal by accident of a script that cannot tell
    caught = 0
    for other in SMALL:
        o = G.script(other)
        try:
            G.check(o, G.Model(int(o["capacity"]), oracle, mutant=mutant), mutant=mutant)
        except AssertionError:
            caught += 1
    assert caught >= 1


# ---- the client's list form ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 2049])
def test_client_dials_list_form(k, oracle):
    """RSK_CONN_CREATE_LIST against the statement sequence of ClientNetManager::createINetConn run around the
    reference's objects; every dialled key then resolves to its row, as ConnOfIntKey found the conn.  Duplicate
    keys end in the reference's assert (INetGroup::AddNetConn) and stay unpinned."""
    c = G.client_case(k)
    offers = G.client_offers(c, oracle)
    cols = R.table(4097, False, seed=1, empty=True)
    h = R.Harness(rc, cols, False, "cpu")
    got = h.raw_create(offers, k, k, list_form=True)
    assert got["n_new"][0] == k and got["n_refused"][0] == 0 and got["n_full"][0] == 0
    rows = G.table_rows(h.tab)
    G.check_client(c, offers, rows, got["new_rows"][:k])
    conn = rc.conn_resolve_host(h.tab, np.full(k, A.RECV_VALID, np.int8), c["key"])[0]
    assert np.array_equal(conn, got["new_rows"][:k])
    ref = R.create_ref(cols, False, offers, k, k, list_form=True)
    assert np.array_equal(ref["new_rows"], got["new_rows"][:k])


# ---- the fixture against a fresh run of the reference ------------------------------------------------------------
def test_fixture_equals_a_fresh_reference_run():
    from tests.oracle_lib import ref_conncreate_available

    if not ref_conncreate_available():
        pytest.skip("oracle/_ref/librsk_ref_conncreate.so not built (needs /root/reference)")
    import resource

    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    room = (hard if hard != resource.RLIM_INFINITY else 1 << 20) - 64  # the harness raises the soft limit to the hard one
    ran = 0
    for name in G.names():
        s = G.script(name)
        if len(s["acc_tuple"]) > room:  # one descriptor per accepted socket
            continue
        rec = G.run_reference(s)
        for k in G.RECORDED:
            assert np.array_equal(rec[k], s[k]), (name, k)
        ran += 1
    assert ran >= len(SMALL)
