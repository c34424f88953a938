"""CPU: the host twins of the tuple pool (rsk_pool_add_host, rsk_pool_offers_host, rsk_pool_settle_host,
rsk_pool_flush_host) and the rules of tests/pool_ref.py, both held to tests/golden/conncreate.npz -- what the
REFERENCE's own TcpAckPool and ServerNetManager held after every event of 20 scripts (tests/pool_golden.py) -- and to
each other on randomised cases.  The mutants of pool_ref show that the fixture sees each rule."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import codec as rc
from tests import collide
from tests import conncreate_golden as G
from tests import pool_golden as PG
from tests import pool_ref as PR


def _twin(s, oracle):
    return G.Twin(rc, int(s["capacity"]), "cpu", None, oracle)


@pytest.mark.parametrize("name", G.names())
def test_host_twins_equal_the_reference(name, oracle):
    s = G.script(name)
    for cap in sorted({PG.pool_capacity(s), 4097}):
        seen = PG.check(s, _twin(s, oracle), PR.LibPools(PR.Lib(rc), cap, cap))
        assert seen["packets"] == len(s["d_key"]) and seen["conns"] == len(s["c_key"])
        assert seen["snapshots"] == len(s["ev_kind"])


@pytest.mark.parametrize("name", G.names())
def test_rules_equal_the_reference(name, oracle):
    s = G.script(name)
    cap = PG.pool_capacity(s)
    assert PG.check(s, _twin(s, oracle), PR.RefPools(cap, cap))["snapshots"] == len(s["ev_kind"])


def test_capacities_and_coverage():
    caps = {n: PG.pool_capacity(G.script(n)) for n in G.names()}
    assert set(caps.values()) == set(PG.CAPACITIES)
    assert PG.largest_pool(G.script("size_4097_g65_all_different")) == 4000 == max(PG.largest_pool(G.script(n)) for n in G.names())
    s = G.script("size_4097_g65_all_different")
    assert int(np.diff(s["pn_off"]).max()) == 3800


# mutant -> (script, what the checker's first complaint names)
CAUGHT = {
    "last_syn_wins": ("repeated_syn", "ack pool after event"),
    "zero_ports_kept": ("refused_syn", "ack pool after event"),
    "ack_from_seq": ("edges", "row"),
    "flag_from_syn": ("refused_syn", "row"),
    "no_purge": ("half_offers", "ack pool after event"),
    "purge_whole_offers": ("deviation_other_tuple", "the moved conn's offer is not held"),
    "expiry_strict": ("expiry", "ack pool after event"),
}
UNSEEN = ("socket_touch_moves_expiry",)


@pytest.mark.parametrize("mutant", PR.MUTANTS)
def test_each_mutant_is_caught(mutant, oracle):
    """Every mutant of pool_ref fails on the script named in CAUGHT, for the reason named there.

    socket_touch_moves_expiry is the one the fixture cannot see: no script accepts a tuple a second time while its
    first socket is still pooled (half_offers accepts one tuple twice, but the first socket has been taken by then),
    so ServerNetManager::add2Pool's emplace never meets an entry in the record.  The rule is read from the source
    (server/ServerNetManager.cpp:116: emplace on a std::map leaves an existing entry as it is); here the mutant is
    shown to pass every one of the 20 scripts, and to differ from the host twin on a constructed second accept."""
    if mutant in UNSEEN:
        for name in G.names():
            s = G.script(name)
            cap = PG.pool_capacity(s)
            PG.check(s, _twin(s, oracle), PR.RefPools(cap, cap, mutant))
        lib = PR.Lib(rc)
        tab = lib.table(PR.empty(8, vals=False))
        one = {"src": np.array([7], np.uint32), "dst": np.array([9], np.uint32), "sp": np.array([1], np.uint16),
               "dp": np.array([2], np.uint16)}
        lib.add(tab, one, 100, 1, False)
        o = lib.add(tab, one, 200, 1, False)
        assert o["n_again"] == 1 and tab.column("expiry")[0] == 100
        c, _ = PR.add_ref(PR.empty(8, vals=False), one, 100, 1, False)
        assert PR.add_ref(c, one, 200, 1, False)[0]["expiry"][0] == 100
        assert PR.add_ref(c, one, 200, 1, False, mutant=mutant)[0]["expiry"][0] == 200
        return
    name, reason = CAUGHT[mutant]
    s = G.script(name)
    cap = PG.pool_capacity(s)
    with pytest.raises(AssertionError) as err:
        PG.check(s, _twin(s, oracle), PR.RefPools(cap, cap, mutant))
    first = err.value.args[0]
    assert (first[0] if isinstance(first, tuple) else first) == reason, err.value


# ---- twin against rule ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", PR.NS)
def test_sizes_twin_equals_rule(n):
    """Every n with every capacity, fill and kind of batch."""
    lib = [PR.Lib(rc)]
    for cap in PR.CAPS:
        for fill in PR.FILLS:
            for kind in PR.KINDS:
                PR.property_case(lib, 31 * n + cap, n, cap, fill, kind)


@pytest.mark.parametrize("case", sorted(PR.CASES))
def test_edges_twin_equals_rule(case):
    kw, want = PR.CASES[case]
    seen = PR.property_case([PR.Lib(rc)], 7, **kw)
    for k, v in want.items():
        assert seen[k] >= v, (case, k, seen)
    if case == "n_new_of_zero":
        assert seen["taken"] == 0


@pytest.mark.parametrize("capacity", [67, 1025])
def test_all_new_tuples_in_one_entry_near_the_end(capacity):
    seen = PR.property_case([PR.Lib(rc)], 11, 2 * capacity, capacity, "empty", "mixed", home=collide.WIDE - 3)
    assert seen["n_new"] == capacity and seen["n_full"] > 0 and seen["n_again"] > 0


def test_a_call_that_changes_nothing_writes_no_index_byte():
    PR.nothing_changes_case(PR.Lib(rc))


def test_index_built_on_one_side_is_the_other_sides():
    """rsk_pool_index_build_host's index under rsk_conn.h's contract, with duplicates counted."""
    import torch

    lib = PR.Lib(rc)
    rng = np.random.default_rng(1)
    uni = PR.universe(rng, 40)
    c = PR.filled(rng, 67, np.arange(40), uni, 0, True)
    for f in ("src", "dst", "sp", "dp"):
        c[f][50] = c[f][3]
    c["state"][50] |= np.uint8(PR.LIVE)
    tab = lib.table(c, rebuild=False)
    n_dup = torch.zeros(1, dtype=torch.int32)
    tab.rebuild(n_dup=n_dup)
    assert int(n_dup[0]) == 1
    PR.index_check(tab, "host build")


def test_invalid_arguments():
    lib = PR.Lib(rc)
    tab = lib.table(PR.empty(8))
    one = {f: np.ones(1, dt) for f, dt in (("src", np.uint32), ("dst", np.uint32), ("sp", np.uint16), ("dp", np.uint16),
                                           ("seq", np.uint32), ("ack", np.uint32))}
    with pytest.raises(rc.RskError):
        lib.add(tab, one, 1, 0, True, work=tab.add_work(1))  # u_max 0
    with pytest.raises(rc.RskError):
        lib.add(tab, one, 1, (1 << 24) + 1, True, work=tab.add_work(1))  # u_max above the create's limit
    with pytest.raises(rc.RskError):
        lib.add(tab, {k: v for k, v in one.items() if k != "seq"}, 1, 1, True)  # the pool has seq, the input not
    with pytest.raises(rc.RskError):
        lib.offers(tab, tab, 0)  # m_max 0
    with pytest.raises(rc.RskError):
        lib.offers(tab, tab, (1 << 21) + 1)  # m_max above the create's limit
    with pytest.raises(rc.RskError):
        lib.offers(lib.table(PR.empty(8, vals=False)), tab, 4)  # an ack pool without seq / ack
    with pytest.raises(rc.RskError):
        rc.pool_flush_host(tab, 1, dead_rows=lib.fill(8))  # dead_rows without n_dead
    with pytest.raises(rc.RskError):
        rc.pool_settle_host(tab, tab, tab.settle_work(tab)[1:], m_max=1)  # work not 16-B aligned
    assert rc.lib().rsk_pool_add_bytes(0, 8) == 0 and rc.lib().rsk_pool_settle_bytes(0, 8) == 0
    assert rc.lib().rsk_pool_settle_bytes(8, (1 << 20) + 1) == 0
    with pytest.raises(rc.RskError):
        rc.PoolTable.alloc(0, "cpu")
