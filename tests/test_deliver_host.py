"""CPU: rsk_deliver_host (include/rsk_codec.h; the host twin of rsk_deliver_batch) against numpy --
the payload slices concatenated in delivery order, np.cumsum of the rounded lengths -- on the
reference's own OnRecv fixture, on random cases and on the argument errors.  Byte-exact throughout."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd.codec import RskError, deliver_host, lib, segment_bytes
from tests.deliver_ref import STRAY, Case, expected, make_case

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def run_host(c: Case, align: int, nthreads: int = 1, **kw):
    return deliver_host(c.arena, c.base_off, c.pay_off, c.pay_len, c.status, inner_off=c.inner_off, order=c.order,
                        n_order=c.n_order, align=align, nthreads=nthreads, **kw)


def test_golden_onrecv_payloads():
    """tests/golden/onrecv.npz (the reference's own RConn::OnRecv over 428 frames): the delivered arena
    is the frames sliced at the reference's recorded pay_off / pay_len of the 187 VALID rows."""
    g = np.load(os.path.join(GOLD, "onrecv.npz"), allow_pickle=False)
    valid = np.nonzero(g["status"] == 1)[0]
    assert len(g["status"]) == 428 and len(valid) == 187 and int((g["hlen"][valid] != 23).sum()) == 32
    src = g["frame_off"][valid].astype(np.int64) + g["pay_off"][valid]
    assert set(src % 16) == set(range(16)) and g["pay_len"][valid].min() == 1 and g["pay_len"][valid].max() == 1453
    want = np.concatenate([g["frames"][int(s): int(s) + int(ln)] for s, ln in zip(src, g["pay_len"][valid])])
    got, off, total = deliver_host(g["frames"], g["frame_off"], g["pay_off"], g["pay_len"], g["status"])
    assert total == 88347 == len(want)
    assert np.array_equal(got, want)
    L = np.where(g["status"] == 1, g["pay_len"], 0).astype(np.uint64)
    assert np.array_equal(off, np.concatenate([[0], np.cumsum(L, dtype=np.uint64)]).astype(np.uint64))


@pytest.mark.parametrize("nthreads", [1, 4])
@pytest.mark.parametrize("align", [1, 16, 128])
@pytest.mark.parametrize("order", ["none", "valid_idx", "subset"])
@pytest.mark.parametrize("n,valid", [(1, 1.0), (63, 0.5), (65, 0.0), (1025, 0.5), (4097, 1.0), (5000, 0.5)])
def test_random_cases(n, valid, order, align, nthreads):
    c = make_case(n, n * 7 + align, valid, order)
    want, woff, wtotal = expected(c, align)
    got, off, total = run_host(c, align, nthreads)
    assert total == wtotal
    assert np.array_equal(off, woff)
    assert np.array_equal(got, want)


def test_all_one_byte_payloads():
    c = make_case(5000, 11, 1.0, lens=np.array([1], np.uint16))
    want, woff, wtotal = expected(c, 1)
    got, off, total = run_host(c, 1, 4)
    assert total == 5000 and np.array_equal(off, woff) and np.array_equal(got, want)


def test_nothing_else_is_touched_and_out_cap():
    c = make_case(4500, 5, 0.7, "subset")
    for align in (1, 16):
        want, woff, wtotal = expected(c, align)
        buf = np.full(wtotal + 64 + 16, 0xA5, np.uint8)
        sh = (-buf.ctypes.data) % 16
        out = buf[sh: sh + wtotal + 64]
        _, off, total = run_host(c, align, 4, out=out, cap=wtotal)
        assert total == wtotal and np.array_equal(out[:wtotal], want) and bool((out[wtotal:] == 0xA5).all())
        # out_cap inside a payload: those that fit are exact, the cut one and the rest stay untouched
        cand = np.nonzero(np.diff(woff) > 1)[0]
        k = int(cand[len(cand) // 3])
        cap = int(woff[k]) + 1
        out[:] = 0xA5
        _, off, total = run_host(c, align, 4, out=out, cap=cap)
        assert total == wtotal and np.array_equal(off, woff)
        fits = woff[1:] <= cap
        keep = np.zeros(len(out), bool)
        for a, b in zip(woff[:-1][fits], woff[1:][fits]):
            keep[int(a): int(b)] = True
        assert np.array_equal(out[keep], want[keep[:wtotal]]) and bool((out[~keep] == 0xA5).all())
        assert bool((out[int(woff[k]):] == 0xA5).all())


def test_plan_only_and_stray_order():
    c = make_case(3000, 9, 0.8, "subset")
    _, woff, wtotal = expected(c, 16)
    none, off, total = run_host(c, 16, plan_only=True)
    assert none is None and total == wtotal and np.array_equal(off, woff)
    # stray entries (>= n) and a poisoned count: zero-length positions, the rest exact
    c.order[::7] = STRAY
    c.order[3::11] = c.n + 5
    c.n_order = 0xFFFFFFFF
    want, woff, wtotal = expected(c, 1)
    got, off, total = run_host(c, 1, 4)
    assert total == wtotal and np.array_equal(off, woff) and np.array_equal(got, want)


def test_segment_bytes_slices_a_demuxed_delivery():
    """order = a demux's perm: segment s is out_off[seg_off[s]] .. out_off[seg_off[s + 1]]."""
    c = make_case(200, 3, 1.0)
    perm = np.random.default_rng(1).permutation(200).astype(np.uint32)
    seg_off = np.array([0, 10, 11, 150, 200], np.uint32)
    got, off, _ = deliver_host(c.arena, c.base_off, c.pay_off, c.pay_len, c.status, inner_off=c.inner_off,
                               order=perm, n_order=200)
    for s in range(4):
        want = [c.arena[int(o): int(o) + int(ln)] for o, ln in
                ((int(c.base_off[i]) + int(c.inner_off[i]) + int(c.pay_off[i]), c.pay_len[i])
                 for i in perm[seg_off[s]: seg_off[s + 1]])]
        assert np.array_equal(segment_bytes(got, off, seg_off, s), np.concatenate(want))


def _structs(c: Case, out, off, tot, align=1):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    cnt = None if c.n_order is None else np.array([c.n_order], np.uint32)
    din = A.DeliverIn(p(c.arena), p(c.base_off), p(c.inner_off), p(c.pay_off), p(c.pay_len), p(c.status), p(c.order),
                      p(cnt))
    dout = A.DeliverOut(p(out), 0 if out is None else len(out), p(off), p(tot), align)
    return din, dout, cnt


def test_argument_errors_and_empty_batch():
    L = lib()
    c = make_case(10, 1, 1.0)
    off, tot = np.full(11, 7, np.uint64), np.full(1, 7, np.uint64)
    buf = np.zeros(20000 + 16, np.uint8)
    out = buf[(-buf.ctypes.data) % 16:][:20000]
    din, dout, _ = _structs(c, out, off, tot)
    call = lambda n=10, i=din, o=dout: L.rsk_deliver_host(n, ctypes.byref(i) if i else None,  # noqa: E731
                                                          ctypes.byref(o) if o else None, 1)
    assert call() == A.OK
    assert call(i=None) == A.EINVAL and call(o=None) == A.EINVAL
    for f in ("base_off", "pay_off", "pay_len", "status"):
        bad, _, _ = _structs(c, out, off, tot)
        setattr(bad, f, None)
        assert call(i=bad) == A.EINVAL, f
    bad = _structs(c, out, None, tot)[1]
    assert call(o=bad) == A.EINVAL
    for al in (0, 3, 24, 256):
        assert call(o=_structs(c, out, off, tot, al)[1]) == A.EINVAL, al
    assert call(o=_structs(c, out[1:], off, tot)[1]) == A.EINVAL  # misaligned out_arena
    only_order = _structs(c, out, off, tot)[0]
    only_order.order = np.arange(10, dtype=np.uint32).ctypes.data
    assert call(i=only_order) == A.EINVAL
    only_count = _structs(c, out, off, tot)[0]
    cnt = np.array([10], np.uint32)
    only_count.n_order = cnt.ctypes.data
    assert call(i=only_count) == A.EINVAL
    assert call(n=(1 << 30) + 1) == A.EINVAL
    with pytest.raises(RskError):
        deliver_host(c.arena, c.base_off, c.pay_off, c.pay_len, c.status, align=3)
    # n == 0: out_off[0] = 0 and *total = 0, the arrays may be NULL
    empty = A.DeliverIn(None, None, None, None, None, None, None, None)
    off[:], tot[:] = 7, 7
    assert call(n=0, i=empty) == A.OK and off[0] == 0 and tot[0] == 0 and off[1] == 7
    dout.total = None  # total may be NULL
    assert call() == A.OK
