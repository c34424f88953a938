"""CPU: the host twins of the conv table (rsk_conv_index_build_host, rsk_conv_resolve_host,
rsk_conv_send_host, rsk_conv_flush_host; include/rsk_codec.h) against tests/conv_ref, pinned to the
reference's own leaves and conv resets (tests/golden/demux.npz), and every RSK_EINVAL of the four entry
points.  tests/test_gpu_conv.py runs the same scenarios on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import conv_ref as R


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CLIENT_MSGS))
def test_host_reference_pin_client(name):
    R.scenario_golden_client(rc, name, "cpu")


@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_host_reference_pin_server(name):
    R.scenario_golden_server(rc, name, "cpu")


@pytest.mark.parametrize("capacity", R.CAPACITIES)
@pytest.mark.parametrize("n", R.SIZES)
def test_host_sizes(n, capacity):
    R.scenario_sizes(rc, n, capacity, "cpu")


@pytest.mark.parametrize("by_dst,by_id", R.FLAG_COMBOS)
def test_host_flag_combinations(by_dst, by_id):
    got, want = R.scenario_sizes(rc, 4097, 257, "cpu", by_dst=by_dst, by_id=by_id)
    assert 0 < want["n_unknown"] < int((got["conv_row"] != R.NONE).sum())


@pytest.mark.parametrize("kind", ["one_row", "all_rows", "alternate", "runs"])
def test_host_skew(kind):
    R.scenario_skew(rc, kind, "cpu")


BAND_TABLES = {}


@pytest.mark.parametrize("pattern", R.BAND_PATTERNS)
@pytest.mark.parametrize("n", R.BAND_SIZES)
@pytest.mark.parametrize("call", ["resolve", "send"])
def test_host_counts_on_colliding_rows(call, n, pattern):
    """The counts over rows that share one run of the device's LDS row table (tests/collide.py): the twin's
    sums are the same np.bincount."""
    R.scenario_band_counts(rc, call, n, pattern, "cpu", cache=BAND_TABLES)


def test_host_conv_rst():
    R.scenario_conv_rst(rc, "cpu")


def test_host_reads():
    R.scenario_reads(rc, "cpu")


def test_host_optional_outputs():
    R.scenario_optional_outputs(rc, "cpu")


def test_host_send():
    R.scenario_send(rc, "cpu")


@pytest.mark.parametrize("capacity", [1, 1000, 65536])
def test_host_flush_steps(capacity):
    R.scenario_flush_steps(rc, capacity, "cpu")


def test_host_flush_life():
    R.scenario_flush_life(rc, "cpu")


def test_host_argument_errors_and_empty_batch():
    R.check_einval(rc, "cpu")


def test_host_index_duplicates_and_unaligned_id():
    """The lowest LIVE row of a key wins, n_dup counts the losers; the host twins take an IdBuf column at any
    alignment."""
    rng = np.random.default_rng(9)
    cols, c = R.random_case(rng, 2000, 300, True, True, pool=40, live=0.8)
    tab = R.make_table(rc, cols, "cpu", True, True)
    nd = np.zeros(1, np.uint32)
    assert rc.lib().rsk_conv_index_build_host(ctypes.byref(tab.abi()), nd.ctypes.data, 1) == A.OK
    tmap, dup = R.table_map(cols, True, True)
    assert int(nd[0]) == dup > 0
    want = R.resolve_ref(cols, True, True, c)
    buf = np.zeros(8 * 2000 + 1, np.uint8)
    buf[1:] = c["id"]
    row = np.zeros(2000, np.uint32)
    cin = A.ConvResolveIn(c["status"].ctypes.data, c["cmd"].ctypes.data, c["hit"].ctypes.data, buf.ctypes.data + 1,
                          c["conv"].ctypes.data, c["dst"].ctypes.data, c["ctl_kind"].ctypes.data, c["ctl_arg"].ctypes.data)
    cout = A.ConvResolveOut(row.ctypes.data, None, None, None, A.CtlMsgs())
    assert rc.lib().rsk_conv_resolve_host(ctypes.byref(tab.abi()), 2000, ctypes.byref(cin), ctypes.byref(cout), 2) == A.OK
    assert np.array_equal(row, want["conv_row"])


def test_conv_struct_layouts_match_header(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = {"rsk_conv_table": A.ConvTable, "rsk_conv_resolve_in": A.ConvResolveIn, "rsk_conv_resolve_out": A.ConvResolveOut,
         "rsk_conv_send_out": A.ConvSendOut, "rsk_conv_flush_out": A.ConvFlushOut}
    consts = {"RSK_CONV_BY_DST": A.CONV_BY_DST, "RSK_CONV_BY_ID": A.CONV_BY_ID, "RSK_CONN_LIVE": A.CONN_LIVE,
              "RSK_CONN_NONE": A.CONN_NONE, "RSK_CONN_MAX_ROWS": A.CONN_MAX_ROWS, "RSK_CTL_CONV_RST": A.CTL_CONV_RST,
              "RSK_CMD_CONV_RST": A.CMD_CONV_RST}
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
