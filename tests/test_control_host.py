"""CPU: the host twins rsk_control_host and rsk_keepalive_flush_host (include/rsk_codec.h) against
tests/control_ref -- the golden batches of tests/golden/demux.npz with synthetic frames, the snapshot
rule against the per-packet walk, the mechanics over batch sizes and capacities, the optional outputs,
the miss option, TCP_CLOSE, the keepalive timer, every RSK_EINVAL and the struct layouts.  Packets whose
frame must not be read carry offsets far outside the arena here: reading one crashes the test.
tests/test_gpu_control.py runs the same scenarios on the device."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import control_ref as C


@pytest.mark.parametrize("name", C.GOLDEN_NAMES)
def test_host_golden_classification(name):
    C.scenario_golden(rc, name, "cpu")


def test_host_snapshot_against_sequential():
    C.scenario_sequential(rc, "cpu")


@pytest.mark.parametrize("capacity", C.CAPACITIES)
@pytest.mark.parametrize("n", C.SIZES)
def test_host_sizes(n, capacity):
    C.scenario_sizes(rc, n, capacity, "cpu")


@pytest.mark.parametrize("n", [257, 4097])
def test_host_sizes_by_id(n):
    got, _ = C.scenario_sizes(rc, n, 257, "cpu", by_id=True)
    assert (got["conn"] != C.NONE).any()


def test_host_extremes():
    C.scenario_extremes(rc, "cpu")


def test_host_optional_outputs():
    C.scenario_optional_outputs(rc, "cpu")


@pytest.mark.parametrize("by_id", [False, True])
def test_host_miss_option(by_id):
    C.scenario_miss(rc, "cpu", by_id=by_id)


def test_host_tcp_close():
    C.scenario_tcp_close(rc, "cpu")


@pytest.mark.parametrize("max_retry", [1, 3])
@pytest.mark.parametrize("capacity", [1, 1000, 65536])
def test_host_flush_steps(capacity, max_retry):
    C.scenario_flush_steps(rc, capacity, max_retry, "cpu", by_id=capacity == 1000)


def test_host_flush_edges():
    C.scenario_flush_edges(rc, "cpu")


def test_host_argument_errors_and_empty_batch():
    L = rc.lib()
    client, server, keep, a = C.einval_fixture(rc, "cpu")
    for t in (client, server):
        t.rebuild()
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    ok, bad = C.control_einval_cases(client, server, a)
    for label, t, n, i, o in ok:
        assert L.rsk_control_host(ref(t), n, ref(i), ref(o), 1) == A.OK, label
    assert keep["kind"].tolist() == [0, 0, 0]
    keep["kind"].fill_(7)
    for label, t, n, i, o in bad:
        assert L.rsk_control_host(ref(t), n, ref(i), ref(o), 1) == A.EINVAL, label
    assert keep["kind"].tolist() == [7, 7, 7]
    # n == 0: null arrays; the counts are zeroed and rst_first filled
    rst = np.zeros(4, np.uint32)
    o = A.ControlOut(None, None, None, a["word"], rst.ctypes.data, None, A.CtlMsgs(*([None] * 7), a["word"]))
    assert L.rsk_control_host(ref(client.abi()), 0, ref(A.ControlIn(*([None] * 12))), ref(o), 1) == A.OK
    assert int(keep["word"][0]) == 0 and rst.tolist() == [C.NO_RST] * 4
    ok, bad = C.flush_einval_cases(client, a)
    for label, t, k, o in ok:
        assert L.rsk_keepalive_flush_host(ref(t), ref(k), ref(o), 1) == A.OK, label
    for label, t, k, o in bad:
        assert L.rsk_keepalive_flush_host(ref(t), ref(k), ref(o), 1) == A.EINVAL, label


def test_control_struct_layouts_match_header(tmp_path):
    import os
    import subprocess

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    m = {"rsk_control_in": A.ControlIn, "rsk_ctl_msgs": A.CtlMsgs, "rsk_control_out": A.ControlOut,
         "rsk_keepalive": A.Keepalive, "rsk_keepalive_out": A.KeepaliveOut}
    body = "".join(f'printf("{t} %zu\\n", sizeof({t}));' +
                   "".join(f'printf("{t}.{f} %zu\\n", offsetof({t}, {f}));' for f, _ in c._fields_) for t, c in m.items())
    consts = {"RSK_CONN_NEW": A.CONN_NEW, "RSK_CTL_NONE": A.CTL_NONE, "RSK_CTL_CONV_RST": A.CTL_CONV_RST,
              "RSK_CTL_NETCONN_RST": A.CTL_NETCONN_RST, "RSK_CTL_KA_REQ": A.CTL_KA_REQ, "RSK_CTL_KA_RESP": A.CTL_KA_RESP,
              "RSK_CTL_TCP_CLOSE": A.CTL_TCP_CLOSE, "RSK_CTL_SHORT": A.CTL_SHORT, "RSK_CTL_UNKNOWN": A.CTL_UNKNOWN,
              "RSK_KA_NONE": A.KA_NONE, "RSK_KA_REQUEST_DELAY_MS": A.KA_REQUEST_DELAY_MS, "RSK_KA_MAX_RETRY": A.KA_MAX_RETRY}
    body += "".join(f'printf("#{k} %u\\n", (unsigned)({k}));' for k in consts)
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rsk_codec.h"\nint main(void){' + body + "return 0;}\n")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", str(exe)], check=True)
    for ln in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n"):
        if not ln.strip():
            continue
        k, v = ln.split()
        if k.startswith("#"):
            assert consts[k[1:]] == int(v), k
        elif "." in k:
            t, f = k.split(".")
            assert getattr(m[t], f).offset == int(v), k
        else:
            assert ctypes.sizeof(m[k]) == int(v), k
