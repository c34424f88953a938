"""CPU: rsk_conn_close_host (include/rsk_codec.h), the host twin of rsk_conn_close_batch, against
tests/conn_close_ref: the capacities at the tile edges with every closing pattern in both forms, the list form's
edges, SWEEP, sequences of closes on one pick index, the reference's recorded control walk, keepalive timer and
doSend with the close in place of the host's state edit and rebuilds, and the argument checks.  After every close
the lookups equal conn_ref's on the new state and the picks equal pick_ref.rule_ref's and a fresh build's.
tests/test_gpu_conn_close.py runs the same scenarios on the device."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conn_close_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", K.CAPACITIES)
def test_patterns(capacity, by_id):
    assert K.scenario_patterns(rc, capacity, by_id, "cpu") > 0


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [2, 257, 1025])
def test_list_edges(capacity, by_id):
    K.scenario_list_edges(rc, capacity, by_id, "cpu")


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [1, 257, 4097])
def test_sweep(capacity, by_id):
    K.scenario_sweep(rc, capacity, by_id, "cpu")


@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", [2, 1025, 4097])
def test_sequences(capacity, by_id):
    K.scenario_sequences(rc, capacity, by_id, "cpu")


@pytest.mark.parametrize("capacity", [64, 257])
def test_emptied_group_keeps_probe_chains(capacity):
    K.scenario_probe_chains(rc, capacity, "cpu")


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("by_id", [False, True])
@pytest.mark.parametrize("capacity", K.COLLIDE_LENGTHS)
def test_constructed_cluster(capacity, by_id, wrap):
    """A full table that is one run of the index (and of the pick's group entries), closed in halves and group by group."""
    assert K.scenario_collide_close(rc, capacity, by_id, wrap, "cpu") == capacity


@pytest.mark.parametrize("name", K.WALK_CASES)
def test_reference_pin_walk(name):
    K.scenario_walk_golden(rc, name, "cpu")


@pytest.mark.parametrize("name", K.TIMER_CASES)
def test_reference_pin_timer(name):
    K.scenario_timer_golden(rc, name, "cpu")


@pytest.mark.parametrize("name", K.SEND_CASES)
def test_reference_pin_send(name):
    K.scenario_send_golden(rc, name, "cpu")


def test_host_argument_errors():
    K.check_einval(rc, "cpu")


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "rsk_codec.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m));
#define S(T) printf(#T " %zu\n", sizeof(T));
int main(void) {
  S(rsk_conn_rows) F(rsk_conn_rows, state)
  S(rsk_conn_close_in) F(rsk_conn_close_in, close_rows) F(rsk_conn_close_in, n_close) F(rsk_conn_close_in, m_max)
  F(rsk_conn_close_in, rst_first) F(rsk_conn_close_in, work) F(rsk_conn_close_in, flags)
  S(rsk_conn_close_out) F(rsk_conn_close_out, marked_rows) F(rsk_conn_close_out, n_marked)
  F(rsk_conn_close_out, closed_rows) F(rsk_conn_close_out, n_closed) F(rsk_conn_close_out, pick)
  F(rsk_conn_close_out, pick_counts)
  printf("REMOVE %u\nSWEEP %u\n", RSK_CONN_CLOSE_REMOVE, RSK_CONN_CLOSE_SWEEP);
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
    assert c.pop("REMOVE") == A.CONN_CLOSE_REMOVE and c.pop("SWEEP") == A.CONN_CLOSE_SWEEP
    m = {"rsk_conn_rows": A.ConnRows, "rsk_conn_close_in": A.ConnCloseIn, "rsk_conn_close_out": A.ConnCloseOut}
    assert len(c) == 16
    for k, v in c.items():
        if "." in k:
            t, f = k.split(".")
            assert getattr(m[t], f).offset == v, k
        else:
            assert ctypes.sizeof(m[k]) == v, k
