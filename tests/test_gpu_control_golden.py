"""GPU: rsk_control_batch (with rsk_conn_resolve_batch's miss column), rsk_keepalive_flush, rsk_conn_pick_batch
and rsk_conv_resolve_batch / rsk_conv_send_batch / rsk_conv_flush against what the REFERENCE's own classes did
with the same inputs: tests/golden/control.npz, read through tests/control_golden.py, whose scenarios
tests/test_control_golden_host.py runs on the host twins.  Only the fixture is read here."""
from __future__ import annotations

import pytest

from rsock_amd import codec as rc
from tests import control_golden as G

pytestmark = pytest.mark.gpu

KEY = b"hello135"
PLAIN, STAGED = 1, 2  # rsk_conn_pick_batch's candidates from global memory / staged in LDS


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


@pytest.mark.parametrize("name", G.names("walk"))
def test_walk(cx, gpu, name):
    s = G.scenario_walk(rc, name, gpu, cx)
    if name == "client_rst_nothing_sent":  # nothing sent: every lookup of the batch is the reference's
        assert s["n_gone"] == 0 and s["n_late"] > 20 and s["n_late_found"] == s["n_late"]
    if name.endswith("_rst_then_sends"):
        assert s["n_gone"] > 0 and 0 < s["n_late_found"] < s["n_late"]


@pytest.mark.parametrize("name", G.names("timer"))
def test_timer(cx, gpu, name):
    s = G.scenario_timer(rc, name, gpu, cx)
    assert s["flushes"] >= 4 and s["sent"] > 0


@pytest.mark.parametrize("name", G.names("send"))
def test_send(cx, gpu, name):
    s = G.scenario_send(rc, name, gpu, cx)
    if name.startswith("alive_") and not name.startswith("alive_1_"):
        assert s["exact"] and s["differ"] > 0
    if name == "avoid_one_10_65536":
        G.check_uniform(s["conn"], s["row"][[k for k in range(10) if k != 4]])


@pytest.mark.parametrize("name,path", [("alive_1024_2048", PLAIN), ("alive_1024_2048", STAGED), ("alive_1024_4097", PLAIN),
                                       ("alive_1024_4097", STAGED), ("avoid_outside_1024_2048", PLAIN),
                                       ("avoid_outside_1024_2048", STAGED), ("alive_1025_2049", PLAIN),
                                       ("alive_10_64", PLAIN), ("alive_10_64", STAGED), ("dead3_10_4097", PLAIN),
                                       ("dead3_10_4097", STAGED)])
def test_send_both_kernels(cx, gpu, name, path):
    """A 1024-row client table takes the LDS-staged kernel by itself, a 1025-row one the plain kernel (test_send);
    here each is forced.  The context does not tell which kernel ran: the internal path switch chooses it."""
    s = G.scenario_send(rc, name, gpu, cx, path=path)
    assert s["exact"] == name.startswith(("alive_", "avoid_outside_"))


@pytest.mark.parametrize("name", G.names("flush"))
def test_flush(cx, gpu, name):
    s = G.scenario_flush(rc, name, gpu, cx)
    assert s["closed"] > 0
