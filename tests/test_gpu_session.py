"""GPU: a server session of many batches on the device, call by call, against the packet walk and byte-for-byte
against the host-twin side (tests/session.py); and two sessions interleaved event by event on two streams of one
context, each with its own tables, each equal to its single-stream run."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from rsock_amd import codec as rc
from tests import session as S
from tests import session_ref as W

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


_HOST = {}


def host_trace(oracle, shape, seed=1):
    if (shape, seed) not in _HOST:
        sc = S.script(seed, shape)
        _HOST[(shape, seed)] = (sc, S.run(sc, S.ServerChain("host", sc["params"], oracle), oracle)[1])
    return _HOST[(shape, seed)]


_DEVICE = {}


def device_trace(cx, gpu, oracle, shape):
    """The shape's session on the device, call by call, against the walk: run once, whichever test asks first."""
    if shape not in _DEVICE:
        sc = host_trace(oracle, shape)[0]
        _DEVICE[shape] = S.run(sc, S.ServerChain("device", sc["params"], oracle, cx, gpu), oracle)
    return _DEVICE[shape]


@pytest.mark.parametrize("shape", sorted(S.SHAPES))
def test_device_equals_the_walk_and_the_host_twins(cx, gpu, oracle, shape):
    sc, want = host_trace(oracle, shape)
    seen, trace = device_trace(cx, gpu, oracle, shape)
    for k, floor in S.SHAPES[shape]["floors"].items():
        assert seen[k] >= floor
    S.same_trace(trace, want, shape)
    assert cx.check_device_errors() == 0


@pytest.mark.parametrize("shape", ["churn", "clustered"])
def test_device_from_captured_graphs(gpu, oracle, shape):
    """The DATA chain (offers .. the second conv create) and the tick's closes, each replayed from a graph captured on
    a side stream of a fresh context behind a reserve and one eager run, over buffers of the largest capture: against
    the walk after every event, and byte for byte against the host-twin side."""
    sc, want = host_trace(oracle, shape)
    caps = [e for e, ev in enumerate(sc["events"]) if ev[0] == "CAPTURE"]
    n_max = max(len(sc["events"][e][1]) for e in caps)
    arena_max = max(len(S.frames_of(oracle, sc, e)[0]) for e in caps)
    ticks = sum(1 for ev in sc["events"] if ev[0] == "TICK" and "ka" in ev[2] and "conv" in ev[2])
    cxg = rc.Codec(KEY, 0)
    try:
        stream = torch.cuda.Stream(gpu)
        cxg.reserve(n_max, stream=stream)
        chain = S.ServerChain("graph", sc["params"], oracle, cxg, gpu, stream=stream, fixed=n_max, arena_max=arena_max)
        seen, trace = S.run(sc, chain, oracle)
        assert chain.replays == len(caps) - 1 + ticks - 1 and ticks >= 2
        S.same_trace(trace, want, shape + " from graphs")
        assert cxg.check_device_errors() == 0
        chain.graphs.clear()
    finally:
        torch.cuda.synchronize()
        cxg.close()


@pytest.mark.parametrize("shape", ["churn", "shrinking"])
def test_split_invariance(cx, gpu, oracle, shape):
    """Every capture once whole and once cut into the 2 to 5 consecutive batches the generator marked as safe, on two
    sets of tables: all tables, outputs, answers and delivered bytes are the same after every event.  No model."""
    sc = host_trace(oracle, shape)[0]
    cuts = [ev[4] for ev in sc["events"] if ev[0] == "CAPTURE"]
    assert all(1 <= len(c) <= 4 for c, n in zip(cuts, S.SHAPES[shape]["sizes"]) if n >= 63)
    n = S.run_split(sc, S.ServerChain("device", sc["params"], oracle, cx, gpu), S.ServerChain("device", sc["params"], oracle, cx, gpu), oracle)
    assert n == sum(len(c) + 1 for c in cuts)
    assert cx.check_device_errors() == 0


def test_two_sessions_on_two_streams_of_one_context(cx, gpu, oracle):
    """steady and churn, event by event in turn, each on a stream of its own with tables of its own: the per-stream
    scratch of one never shows in the other.  Each equals its single-stream run."""
    names = ("steady", "churn")
    scs = [host_trace(oracle, s)[0] for s in names]
    single = [device_trace(cx, gpu, oracle, s)[1] for s in names]
    streams = [torch.cuda.Stream(gpu) for _ in names]
    chains = [S.ServerChain("device", sc["params"], oracle, cx, gpu, stream=st) for sc, st in zip(scs, streams)]
    walks = [W.Walk(sc["params"]["cap_conn"], sc["params"]["cap_conv"], sc["params"]["cap_pool"], sc["params"]["cap_pool"], S.PERSIST_MS)
             for sc in scs]
    traces = [[], []]
    try:
        for e in range(max(len(sc["events"]) for sc in scs)):
            for j, sc in enumerate(scs):
                if e < len(sc["events"]):
                    with chains[j].on():
                        traces[j].append(S.step(sc, e, sc["events"][e], walks[j], chains[j], oracle, f"{names[j]} on its stream, event {e}"))
        for j, s in enumerate(names):
            S.same_trace(traces[j], single[j], s + " interleaved")
        assert cx.check_device_errors() == 0
    finally:
        torch.cuda.synchronize()
        for st in streams:
            cx.release_stream(st)
