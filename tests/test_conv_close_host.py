"""CPU: rsk_conv_close_host (include/rsk_codec.h), the host twin of rsk_conv_close_batch, against
tests/conv_close_ref: the reference's recorded IGroup::Flush -> CloseConn rounds with the close in place of the
host's state edit and rebuild, the timer form on random lists, the chain resolve -> create -> close (HOLD) ->
create against the per-packet walk, the specified deviations, HOLD against not HOLD, calls that close nothing
(index bytes untouched), skew, poisoned columns, optional outputs and the argument checks.
tests/test_gpu_conv_close.py runs the same scenarios on the device."""
from __future__ import annotations

import ctypes
import os
import subprocess
import tempfile

import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conv_close_ref as K
from tests import conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", K.FLUSH_CASES)
def test_reference_pin_flush_close(name):
    assert K.scenario_flush_golden(rc, name, "cpu")["closed"] > 0


@pytest.mark.parametrize("length,shape,flags,wrap", K.INDEX_CLUSTERS)
def test_constructed_cluster_index(length, shape, flags, wrap):
    """The conn index's cluster families for the conv table's key forms (tests/collide.py; the client's conv-only keys
    by search): a full table that is one run of the index, two interleaved homes, duplicates inside the run (the
    lowest row wins, n_dup), absent keys of the same and of the neighbouring homes."""
    assert K.scenario_cluster_index(rc, length, shape, flags[0], flags[1], wrap, "cpu") > length // 2


@pytest.mark.parametrize("capacity,flags,wrap", K.LIFE_CLUSTERS)
def test_constructed_cluster(capacity, flags, wrap):
    """A create that fills the table (a run as long as the table has rows), the list-form close of every second row,
    a create in place into the index as the close left it, a close under HOLD (BY_DST), then the rest: on a conv table
    whose keys all probe from one entry of the index, across the index's end or not."""
    assert K.scenario_cluster(rc, capacity, flags[0], flags[1], wrap, "cpu") > capacity // 2


@pytest.mark.parametrize("by_dst,by_id", R.FLAG_COMBOS)
@pytest.mark.parametrize("capacity", K.CAPACITIES)
def test_timer_random(capacity, by_dst, by_id):
    K.scenario_timer_random(rc, capacity, by_dst, by_id, "cpu")


@pytest.mark.parametrize("capacity", K.CAPACITIES)
@pytest.mark.parametrize("n", K.SIZES)
def test_receive_against_walk(n, capacity):
    K.scenario_walk(rc, n, capacity, True, "cpu")


def test_receive_against_walk_without_ids():
    out, _w = K.scenario_walk(rc, 4097, 1025, False, "cpu")
    assert out["cl"]["n_closed"] > 10 and out["cl"]["n_reopened"] > 10


@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_receive_against_walk_golden(name, seed):
    K.scenario_walk_golden(rc, name, seed, "cpu")


def test_deviations():
    K.scenario_deviations(rc, "cpu")


def test_hold_against_plain():
    K.scenario_hold(rc, "cpu")


def test_nothing_to_close():
    K.scenario_nothing(rc, "cpu")


@pytest.mark.parametrize("kind", ["one_conv", "every_row", "edges"])
def test_skew(kind):
    K.scenario_skew(rc, kind, "cpu")


def test_reads():
    K.scenario_reads(rc, "cpu")


def test_optional_outputs():
    K.scenario_optional_outputs(rc, "cpu")


def test_host_argument_errors():
    K.check_einval(rc, "cpu")


PROBE = r"""
#include <stdio.h>
#include <stddef.h>
#include "rsk_codec.h"
#define F(T, m) printf(#T "." #m " %zu\n", offsetof(T, m));
#define S(T) printf(#T " %zu\n", sizeof(T));
int main(void) {
  S(rsk_conv_close_in) F(rsk_conv_close_in, close_rows) F(rsk_conv_close_in, n_close) F(rsk_conv_close_in, m_max)
  F(rsk_conv_close_in, rst_first) F(rsk_conv_close_in, ctl_kind) F(rsk_conv_close_in, work) F(rsk_conv_close_in, flags)
  S(rsk_conv_close_out) F(rsk_conv_close_out, conv_row) F(rsk_conv_close_out, unknown) F(rsk_conv_close_out, n_unknown)
  F(rsk_conv_close_out, closed_rows) F(rsk_conv_close_out, closed_at) F(rsk_conv_close_out, n_closed)
  F(rsk_conv_close_out, n_reopened) F(rsk_conv_close_out, n_rst_again)
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
    m = {"rsk_conv_close_in": A.ConvCloseIn, "rsk_conv_close_out": A.ConvCloseOut}
    assert len(c) == 17
    for k, v in c.items():
        if "." in k:
            t, f = k.split(".")
            assert getattr(m[t], f).offset == v, k
        else:
            assert ctypes.sizeof(m[k]) == v, k
