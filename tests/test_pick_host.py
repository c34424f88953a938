"""CPU: the host twins of the send pick (rsk_conn_pick_build_host, rsk_conn_pick_host; include/rsk_codec.h)
against tests/pick_ref's rule_ref, rule_ref against the step-by-step walk of INetGroup::doSend, a stale and a
never-built pick index, the struct layouts and every RSK_EINVAL.  tests/test_gpu_pick.py runs the same
scenarios on the device."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_ref as CR
from tests import pick_ref as R

TABLES: dict = {}


# ---- rule_ref against the walk of doSend (no library code) ------------------------------------------------------
def _mconns(cols, rows):
    return [[int(r), int(cols["conn_key"][r]), bool((cols["state"][r] & R.UP) == R.UP)] for r in rows]


def test_rule_equals_dosend_when_all_alive():
    """Every conn alive, no avoid key: the walk consumes one draw per packet and takes rand() % size of mConns;
    rule_ref over a table whose rows stand in mConns order gives the same picks from the same draws."""
    rng = np.random.default_rng(1)
    for m in (1, 2, 10, 65):
        cols = CR.random_columns(rng, m)
        cols["state"][:] = R.UP
        n = 500
        draw = rng.integers(0, 2**31, n, dtype=np.uint64).astype(np.uint32)  # rand() is non-negative
        draw[:4] = [0, m - 1, m, 2**31 - 1]
        it = iter(draw.tolist())
        walk = [R.dosend_walk(_mconns(cols, range(m)), it) for _ in range(n)]
        assert next(it, None) is None  # one draw per packet
        conn, n_none, _ = R.rule_ref(cols, False, n, draw=draw)
        assert n_none == 0 and np.array_equal(conn, np.array(walk, np.uint32))


def test_dosend_pick_is_a_candidate_in_every_other_case():
    """Dead conns, avoid keys, nread <= 0: the walk's pick is a member of rule_ref's candidate set less the
    avoided conn; no candidate at all is ERR_NO_CONN there and NONE here; the avoid-only case spins there."""
    rng = np.random.default_rng(2)
    spins = 0
    for trial in range(300):
        m = int(rng.integers(1, 12))
        cols = CR.random_columns(rng, m)
        cols["state"][:] = np.where(rng.random(m) < 0.6, R.UP, A.CONN_LIVE).astype(np.uint8)
        cols["conn_key"][:] = np.arange(1, m + 1, dtype=np.uint64)
        cand = set(R.candidates(cols["state"], None, False)[0].tolist())
        avoid = int(rng.integers(0, m + 2))  # 0 = none, m + 1 = no conn's key
        nread = int(rng.integers(-1, 3))
        draws = (int(x) for x in rng.integers(0, 2**31, 100000))
        conn, n_none, _ = R.rule_ref(cols, False, 1, len=np.array([nread], np.int32),
                                     avoid_key=np.array([avoid], np.uint64), draw=np.array([next(draws)], np.uint32))
        allowed = cand - ({avoid - 1} if avoid else set())
        try:
            got = R.dosend_walk(_mconns(cols, range(m)), draws, nread, avoid)
        except R.Spin:
            spins += 1
            assert cand and not allowed and nread > 0 and conn[0] == R.NONE and n_none == 1
            continue
        if nread <= 0:
            assert got == nread and conn[0] == R.NONE and n_none == 0
        elif not cand:
            assert got == R.ERR_NO_CONN and conn[0] == R.NONE and n_none == 1
        else:
            assert got in allowed and int(conn[0]) in allowed and n_none == 0
    assert spins > 0


# ---- the host twins against rule_ref ------------------------------------------------------------------------------
@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", R.CAPACITIES)
@pytest.mark.parametrize("n", R.SIZES)
def test_host_sizes(n, capacity, by_id):
    R.scenario_sizes(rc, n, capacity, by_id, "cpu", tables=TABLES)


def test_host_threads():
    cols, pool, derived = R.sized_table(257, True)
    b = R.random_batch(np.random.default_rng(4), cols, pool, True, 9001)
    R.check(rc, cols, True, 9001, "cpu", derived=derived, nthreads=4, **b)


@pytest.mark.parametrize("zero_real", [False, True])
def test_host_group_shapes(zero_real):
    R.scenario_groups(rc, zero_real, "cpu")


@pytest.mark.parametrize("m", R.BIG_GROUPS)
def test_host_big_group(m):
    R.scenario_big_group(rc, m, "cpu")


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("groups", [65, 1025])
def test_host_colliding_groups(groups, wrap):
    """Groups whose entries in the pick index all probe from one entry (tests/collide.py)."""
    assert R.scenario_colliding_groups(rc, groups, "cpu", wrap=wrap) > 4 * groups


@pytest.mark.parametrize("by_id", [False, True])
def test_host_avoid_keys(by_id):
    R.scenario_avoid(rc, by_id, "cpu")


def test_host_seed_stream_and_coverage():
    R.scenario_seed(rc, "cpu")


def test_host_len_gate_and_reads():
    R.scenario_reads(rc, "cpu")


@pytest.mark.parametrize("by_id", [False, True])
def test_host_stale_state(by_id):
    R.scenario_stale_state(rc, by_id, "cpu")


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("capacity", [1, 2, 257])
@pytest.mark.parametrize("by_id", [False, True])
def test_host_garbage_index(by_id, capacity, seed):
    R.scenario_garbage_index(rc, by_id, capacity, seed)


def test_host_counts_and_unaligned_ids():
    """counts = (groups with a candidate, candidates); the host twins take IdBuf columns at any alignment."""
    cols, ids = R.grouped_table(True)
    tab = R.make_table(rc, cols, True, "cpu")
    counts = np.zeros(2, np.uint32)
    rc.conn_pick_build_host(tab, counts=counts)
    assert counts.tolist() == [len(R.GROUP_SIZES), sum(R.GROUP_SIZES)]
    cap = tab.capacity
    n = 700
    w = np.array([ids[k] for k in ids], np.uint64)[np.arange(n) % len(ids)]
    buf = np.zeros(8 * n + 3, np.uint8)
    buf[3:] = R.id_bytes(w)
    tid = np.zeros(8 * cap + 1, np.uint8)
    tid[1:] = cols["id"]
    t = tab.abi()
    t.id = tid.ctypes.data + 1
    pick = np.zeros(tab.pick.numel() + 4, np.uint32)
    pick = pick[(-(pick.ctypes.data // 4) % 4):][: tab.pick.numel()]  # 16-B aligned
    assert rc.lib().rsk_conn_pick_build_host(ctypes.byref(t), pick.ctypes.data, None, 1) == A.OK
    conn = np.zeros(n, np.uint32)
    pin = A.ConnPickIn(None, buf.ctypes.data + 3, None, None, 99)
    pout = A.ConnPickOut(conn.ctypes.data, None, None)
    assert rc.lib().rsk_conn_pick_host(ctypes.byref(t), pick.ctypes.data, n, ctypes.byref(pin), ctypes.byref(pout), 2) == A.OK
    assert np.array_equal(conn, R.rule_ref(cols, True, n, id=R.id_bytes(w), seed=99)[0])


def test_host_argument_errors_and_empty_batch():
    R.check_einval(rc, "cpu")


def test_pick_struct_layouts_match_header(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = {"rsk_conn_pick_in": A.ConnPickIn, "rsk_conn_pick_out": A.ConnPickOut, "rsk_conn_table": A.ConnTable}
    consts = {"RSK_CONN_BY_ID": A.CONN_BY_ID, "RSK_CONN_LIVE": A.CONN_LIVE, "RSK_CONN_ALIVE": A.CONN_ALIVE,
              "RSK_CONN_NEW": A.CONN_NEW, "RSK_CONN_NONE": A.CONN_NONE, "RSK_CONN_MAX_ROWS": A.CONN_MAX_ROWS}
    body = "".join(f'printf("{t} %zu\\n", sizeof({t}));' +
                   "".join(f'printf("{t}.{f} %zu\\n", offsetof({t}, {f}));' for f, _ in c._fields_) for t, c in m.items())
    body += "".join(f'printf("#{k} %llu\\n", (unsigned long long)({k}));' for k in consts)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsk_codec.h"\nint main(void){' + body + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    seen = 0
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if not ln.strip():
            continue
        k, v = ln.split()
        seen += 1
        if k.startswith("#"):
            assert consts[k[1:]] == int(v), k
        elif "." in k:
            t, f = k.split(".")
            assert getattr(m[t], f).offset == int(v), k
        else:
            assert ctypes.sizeof(m[k]) == int(v), k
    assert seen == len(consts) + sum(1 + len(c._fields_) for c in m.values())


def test_index_size_and_table_copy():
    """rsk_conn_pick_bytes is a multiple of 16 for every flag value; ConnTable.to() carries the pick index."""
    for cap, by_id in itertools.product((1, 2, 3, 5, 257, 65536), (False, True)):
        assert rc.lib().rsk_conn_pick_bytes(cap, int(by_id)) % 16 == 0
    cols, pool, _ = R.sized_table(257, True)
    tab = R.make_table(rc, cols, True, "cpu")
    cp = tab.to("cpu")
    assert cp.pick is not tab.pick and bool((cp.pick == tab.pick).all())
