"""CPU: rsk_conn_create_host (include/rsk_codec.h), the host twin of rsk_conn_create_batch, against
tests/conn_create_ref: the capacities and batch sizes at the tile edges with both table flavours, the patterns
(nothing missing, no offers, one conn, every packet a new key, one key, the table full and exactly full, two keys
on one offer, two offers of one tuple, unclaimed offers, *n_offer > m_max), new rows around a group's candidates,
new and reborn groups, the repeat loop, the list form, the row initialisation pinned by tests/golden/tcpstate.npz,
the equivalence with the host procedure the call replaces, sequences with closes, and the argument checks.
tests/test_gpu_conn_create.py runs the same scenarios on the device."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_create_ref as R
from tests import tcpstate_golden as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", R.CAPACITIES)
def test_capacities(capacity, by_id):
    R.scenario_sizes(rc, capacity, 700, by_id, "cpu")


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("n", R.SIZES)
def test_batch_sizes(n, by_id):
    made = R.scenario_sizes(rc, 1025, n, by_id, "cpu")
    assert (made > 0) == (n > 0)


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1, 2, 257, 1025])
def test_patterns(capacity, by_id):
    R.scenario_patterns(rc, capacity, by_id, "cpu")


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity,live0,k", R.COLLIDE_CASES)
def test_constructed_cluster(capacity, live0, k, by_id, wrap):
    """Table keys, new keys, offered 4-tuples and group ids that all probe from one entry (tests/collide.py)."""
    assert R.scenario_collide(rc, capacity, live0, k, by_id, wrap, "cpu") > capacity // 2


@pytest.mark.parametrize("capacity", [257, 1025])
def test_constructed_cluster_of_new_groups(capacity):
    assert R.scenario_collide_groups(rc, capacity, "cpu") == 70


@pytest.mark.parametrize("by_id", [False, True])
def test_groups_grow_and_are_reborn(by_id):
    assert R.scenario_groups(rc, by_id, "cpu") > 100


@pytest.mark.parametrize("capacity", [2, 257])
def test_idbuf_churn_beyond_the_group_entries(capacity):
    assert R.scenario_churn(rc, capacity, "cpu") > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1025, 4097])
def test_repeat_loop_reaches_the_one_call_result(capacity, by_id):
    R.scenario_repeat(rc, capacity, by_id, "cpu")


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1, 2, 257, 1025])
def test_list_form(capacity, by_id):
    R.scenario_list(rc, capacity, by_id, "cpu")


@pytest.mark.parametrize("name", T.names()[:6])
def test_rows_hold_the_recorded_init_state(name):
    assert R.scenario_tcpstate(rc, name, "cpu") > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity,seed", [(257, 0), (1025, 1), (4097, 2)])
def test_equivalence_with_the_host_procedure(capacity, seed, by_id):
    assert R.scenario_equivalence(rc, capacity, by_id, "cpu", seed=seed) > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [2, 257, 1025])
def test_sequences(capacity, by_id):
    assert R.scenario_sequences(rc, capacity, by_id, "cpu") > 0


def test_host_argument_errors():
    R.check_einval(rc, "cpu")


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "rsk_codec.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m));
#define S(T) printf(#T " %zu\n", sizeof(T));
int main(void) {
  S(rsk_conn_create_rows) F(rsk_conn_create_rows, state) F(rsk_conn_create_rows, id) F(rsk_conn_create_rows, flag)
  S(rsk_conn_offers) F(rsk_conn_offers, ack) F(rsk_conn_offers, conn_key) F(rsk_conn_offers, n_offer) F(rsk_conn_offers, m_max)
  S(rsk_conn_create_in) F(rsk_conn_create_in, dp) F(rsk_conn_create_in, offers) F(rsk_conn_create_in, u_max)
  F(rsk_conn_create_in, flags) F(rsk_conn_create_in, now_ms) F(rsk_conn_create_in, established_ms)
  F(rsk_conn_create_in, ka_tries) F(rsk_conn_create_in, work)
  S(rsk_conn_create_out) F(rsk_conn_create_out, n_miss) F(rsk_conn_create_out, new_offer) F(rsk_conn_create_out, offer_row)
  F(rsk_conn_create_out, n_refused) F(rsk_conn_create_out, pick) F(rsk_conn_create_out, pick_counts)
  printf("LIST %u\nREPEAT %u\n", RSK_CONN_CREATE_LIST, RSK_CONN_CREATE_REPEAT);
  return 0;
}
"""


def test_struct_layouts_match_header():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe.c")
        open(src, "w").write(PROBE)
        exe = os.path.join(d, "probe")
        subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    c = {ln.split()[0]: int(ln.split()[1]) for ln in lines if ln.strip()}
    assert c.pop("LIST") == A.CONN_CREATE_LIST and c.pop("REPEAT") == A.CONN_CREATE_REPEAT
    m = {"rsk_conn_create_rows": A.ConnCreateRows, "rsk_conn_offers": A.ConnOffers, "rsk_conn_create_in": A.ConnCreateIn,
         "rsk_conn_create_out": A.ConnCreateOut}
    assert len(c) == 25
    for k, v in c.items():
        if "." in k:
            t, f = k.split(".")
            assert getattr(m[t], f).offset == v, k
        else:
            assert ctypes.sizeof(m[k]) == v, k


def test_work_size_is_the_documented_formula():
    def s(x):
        p = 4
        while p < 2 * x:
            p <<= 1
        return p

    r4 = lambda x: (x + 3) & ~3  # noqa: E731
    for u, mo, cap in ((0, 1, 1), (16, 8, 64), (2049, 300, 257), (1 << 20, 1 << 20, 1 << 20), (5, 4097, 1025)):
        ui, m = max(u, mo), min(mo, cap)
        words = (16 + r4(2 * ((ui + 63) // 64)) + s(ui) + 2 * r4(ui) + s(mo) + 2 * r4(mo) + 6 * r4(m) + 2 * r4(2 * m) + s(m)
                 + 2 * r4(cap))
        for flags in (0, 1):
            assert rc.lib().rsk_conn_create_bytes(u, mo, cap, flags) == 4 * words, (u, mo, cap)
