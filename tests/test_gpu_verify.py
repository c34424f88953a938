"""GPU: rsk_verify_wire_batch (include/rsk_codec.h; rsock_amd/csrc/rsk_verify.hip) against
tests/csum_ref -- csum, status_out and n_bad exactly -- on the shapes of tests/verify_cases: every
start alignment and segment length, every covered byte, nothing outside the packet, carries, every
rung of the rule, gating and aliasing, batch sizes; then every packet the wire build writes on each of
its paths, the receive pipeline with and without the check, a captured graph, and the host twin."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import workload
from tests import csum_ref as R
from tests import verify_cases as V
from tests.test_verify_host import assert_right_bit

pytestmark = pytest.mark.gpu
KEY = b"hello135"
FILL = 0xEE


@pytest.fixture(scope="module")
def cx(gpu):
    from rsock_amd.codec import Codec

    c = Codec(KEY, 0)
    yield c
    c.close()


def dev(a, gpu, dt=None):
    import torch

    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(dt) if dt is not None else a).to(gpu)


def run_gpu(cx, gpu, c: V.Case, alias: bool = False, stream=None):
    """-> (csum, status_out or None, n_bad) on the host; the device arena is exactly the case's bytes."""
    import torch

    n = c.n
    csum = torch.full((n,), FILL, dtype=torch.uint8, device=gpu)
    nb = torch.full((1,), -1, dtype=torch.int32, device=gpu)
    st = dev(c.status, gpu)
    so = None if st is None else (st if alias else torch.full((n,), 0x55, dtype=torch.int8, device=gpu))
    cx.verify_wire_batch(dev(c.arena, gpu), dev(c.cap_off, gpu, np.int64), dev(c.cap_len, gpu, np.int32), c.datalink,
                         csum, status=st, status_out=so, n_bad=nb, stream=stream)
    torch.cuda.synchronize()
    return csum.cpu().numpy(), None if so is None else so.cpu().numpy(), int(nb.cpu().numpy().view(np.uint32)[0])


def check(cx, gpu, c: V.Case, alias: bool = False):
    want, wst, wbad = c.expected()
    got, gst, gbad = run_gpu(cx, gpu, c, alias)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]], c.cap_off[bad[:8]] % 16, c.cap_len[bad[:8]])
    assert gbad == wbad
    if c.status is not None:
        assert np.array_equal(gst, wst)
    return want


# ---- 1. alignment x length --------------------------------------------------------------------------
@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_alignment_and_lengths(cx, gpu, datalink):
    for pad in range(16):
        check(cx, gpu, V.alignment_case(datalink, pad))


# ---- 2. every byte counts ---------------------------------------------------------------------------
def test_every_byte_counts(cx, gpu):
    c, where = V.every_byte_case()
    want = check(cx, gpu, c)
    assert want[0] == R.ALL_OK
    assert_right_bit(want, where)


# ---- 3. nothing outside counts ----------------------------------------------------------------------
def test_nothing_outside_counts(cx, gpu):
    a, b = check(cx, gpu, V.neighbours_case(0x00)), check(cx, gpu, V.neighbours_case(0xFF))
    assert np.array_equal(a, b) and bool((a == R.ALL_OK).all())


# ---- 4. carries -------------------------------------------------------------------------------------
@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_carries(cx, gpu, datalink):
    assert bool((check(cx, gpu, V.carries_case(datalink)) == R.ALL_OK).all())


# ---- 5. the ladder ----------------------------------------------------------------------------------
@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_ladder(cx, gpu, datalink):
    want = check(cx, gpu, V.ladder_case(datalink))
    assert (want == 0).sum() >= 6 and (want & R.TCP_TRUNC).any()


# ---- 6. gating, aliasing, errors --------------------------------------------------------------------
@pytest.mark.parametrize("datalink", V.DATALINKS)
@pytest.mark.parametrize("alias", [False, True])
def test_gating_and_aliasing(cx, gpu, datalink, alias):
    c = V.gated_case(datalink)
    want = check(cx, gpu, c, alias)
    assert bool((want[c.status != 1] == 0).all()) and R.is_bad(want).any()


def test_argument_errors_and_empty_batch(cx, gpu):
    import torch

    from rsock_amd.codec import RskError, lib

    c = V.sized_case(9)
    arena, off, cl = dev(c.arena, gpu), dev(c.cap_off, gpu, np.int64), dev(c.cap_len, gpu, np.int32)
    csum = torch.zeros(9, dtype=torch.uint8, device=gpu)
    st = torch.ones(9, dtype=torch.int8, device=gpu)
    nb = torch.full((1,), 7, dtype=torch.int32, device=gpu)
    L = lib()
    s = torch.cuda.current_stream().cuda_stream

    def structs():
        return (A.VerifyIn(arena.data_ptr(), off.data_ptr(), cl.data_ptr(), None),
                A.VerifyOut(csum.data_ptr(), None, nb.data_ptr()))

    def call(vin, vout, n=9, dl=A.DLT_EN10MB, ctx=cx._ctx):
        return L.rsk_verify_wire_batch(ctx, n, ctypes.byref(vin) if vin else None, dl,
                                       ctypes.byref(vout) if vout else None, s)

    assert call(*structs()) == A.OK
    assert call(*structs(), ctx=None) == A.EINVAL
    assert call(None, structs()[1]) == A.EINVAL and call(structs()[0], None) == A.EINVAL
    for f in ("cap_arena", "cap_off", "cap_len"):
        vin, vout = structs()
        setattr(vin, f, None)
        assert call(vin, vout) == A.EINVAL, f
    vin, vout = structs()
    vout.csum = None
    assert call(vin, vout) == A.EINVAL
    vin, vout = structs()
    vout.status_out = st.data_ptr()  # status_out without status
    assert call(vin, vout) == A.EINVAL
    with pytest.raises(RskError):
        cx.verify_wire_batch(arena, off, cl, A.DLT_EN10MB, csum, status_out=st)
    for dl in (-1, 2, 11, 13, 113):
        assert call(*structs(), dl=dl) == A.EINVAL, dl
    assert call(*structs(), n=A.VERIFY_MAX_BATCH + 1) == A.EINVAL
    vin, vout = structs()
    vout.n_bad = None  # n_bad may be NULL
    assert call(vin, vout) == A.OK
    # n == 0: zeroes a given n_bad and nothing else; the arrays may be NULL
    torch.cuda.synchronize()
    nb.fill_(7)
    csum.fill_(FILL)
    assert call(A.VerifyIn(None, None, None, None), A.VerifyOut(None, None, nb.data_ptr()), n=0) == A.OK
    assert call(A.VerifyIn(None, None, None, None), A.VerifyOut(None, None, None), n=0) == A.OK
    torch.cuda.synchronize()
    assert int(nb.item()) == 0 and bool((csum == FILL).all())
    # the parse and filter entry points still reject the verify-only datalink
    from rsock_amd.codec import DecodeBuffers, TcpInfoBuffers, make_filter

    with pytest.raises(RskError):
        cx.rawinput_batch(arena, off, cl, cl, A.DLT_RAW, 0, TcpInfoBuffers.alloc(9, gpu), DecodeBuffers.alloc(9, gpu))
    with pytest.raises(RskError):
        cx.capture_filter_batch(arena, off, cl, A.DLT_RAW, make_filter(), csum)


# ---- 7. sizes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 70001])
def test_sizes(cx, gpu, n):
    check(cx, gpu, V.sized_case(n))


# ---- 8. the wire build's packets verify ---------------------------------------------------------------
WIRE_PATHS = [(1, 0), (2, 1), (2, 2), (2, 4)]  # tests/test_gpu_wire.py's wpath list
WIRE_LAYOUTS = ["aligned", "odd_payload", "odd_wire", "any_wire", "packed_wire"]
WIRE_EDGE_LENS = [0, 1, 2, 8, 9, 10, 11, 12, 15, 16, 17, 31, 32, 33, 100, 1000, 1400, 1468, 1469, 1470]


@pytest.mark.parametrize("eth", [False, True])
@pytest.mark.parametrize("wpath", WIRE_PATHS, ids=["perset", "two_pass_k1", "two_pass_k2", "two_pass_k4"])
def test_wire_build_round_trip(cx, gpu, eth, wpath):
    """tests/test_gpu_wire.py's layouts, pad modes and length mixes at n = 20000 on one held build path:
    every packet written (status > 0) has both checksums right -- RSK_DLT_RAW for the RAW4 layout,
    EN10MB for Ethernet -- and n_bad is 0.  An independent check of the wire build (the build kernels
    fill the checksums in; nothing of theirs is used here)."""
    import torch

    n, pitch_p = 20000, 1504
    rng = np.random.default_rng(80 + 2 * WIRE_PATHS.index(wpath) + eth)
    g = torch.Generator(device=gpu)
    g.manual_seed(8)
    ri = lambda hi, dt: torch.randint(0, hi, (n,), device=gpu, generator=g, dtype=torch.int64).to(dt)  # noqa: E731
    payload = torch.randint(0, 256, (n * pitch_p + 64,), device=gpu, generator=g, dtype=torch.int64).to(torch.uint8)
    cmd, conv, ckey = ri(5, torch.uint8), ri(2**31, torch.int32), ri(2**62, torch.int64)
    fields = [ri(2**31, torch.int32), ri(2**31, torch.int32), ri(2**15, torch.int16) + 1, ri(2**15, torch.int16) + 1,
              ri(2**31, torch.int32), ri(2**31, torch.int32), ri(256, torch.uint8), ri(2**15, torch.int16)]
    wire = torch.randint(0, 256, (n * 1664 + 64,), device=gpu, generator=g, dtype=torch.int64).to(torch.uint8)
    status = torch.empty(n, dtype=torch.int32, device=gpu)
    csum = torch.empty(n, dtype=torch.uint8, device=gpu)
    nb = torch.empty(1, dtype=torch.int32, device=gpu)
    ethb = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + b"\x08\x00" if eth else None
    L = 14 if eth else 0
    idx = np.arange(n)
    verdicts = []
    try:
        cx.set_encode_path(wpath[0])
        cx.set_copy_k(wpath[1])
        for layout in WIRE_LAYOUTS:
            for pad in (0, 16, 128):
                if layout == "packed_wire" and pad:
                    continue  # back-to-back packets leave no room for the zero pad
                for mix in ("mixed", "short", "bimodal", "long"):
                    lo, hi = (1200 if mix == "long" else 1), (1470 if mix in ("mixed", "long") else 160)
                    lens = np.concatenate([WIRE_EDGE_LENS, rng.integers(lo, hi, n - 20)])
                    if mix == "bimodal":
                        lens[n // 2:] = rng.integers(1000, 1470, n - n // 2)
                    pay_off = idx * pitch_p + (idx % 13 if layout == "odd_payload" else 0)
                    pitch_w = 1664 if pad == 128 else 1600
                    wire_off = idx * pitch_w + (5 if layout == "odd_wire" else 0)
                    if layout == "any_wire":
                        wire_off = idx * pitch_w + (idx * 7) % 16
                    elif layout == "packed_wire":
                        wl = np.where((lens > 0) & (lens <= 1469), L + 40 + 31 + lens, 0)
                        wire_off = np.concatenate([[3], np.cumsum(wl + rng.integers(0, 4, n))[:-1] + 3])
                    woff = dev(wire_off.astype(np.int64), gpu)
                    cx.output_wire_batch(payload, dev(pay_off.astype(np.int64), gpu), dev(lens.astype(np.uint16), gpu, np.int16),
                                         cmd, conv, ckey, *fields, wire, woff, status, eth=ethb,
                                         id_uniform=workload.ID_UNIFORM, pad16=pad == 16, pad128=pad == 128)
                    took = (cx.last_encode_path, cx.last_copy_k if wpath[0] == 2 else 0)
                    assert took == wpath, f"wire build held to {wpath} ran {took}"
                    cap_len = status.clamp(min=0)
                    cx.verify_wire_batch(wire, woff, cap_len, A.DLT_EN10MB if eth else A.DLT_RAW, csum, n_bad=nb)
                    written = status > 0
                    want_written = torch.from_numpy((lens > 0) & (lens <= 1469)).to(gpu)
                    verdicts.append(torch.stack([(written == want_written).all().float(),
                                                 (csum[written] == R.ALL_OK).all().float(), (csum[~written] == 0).all().float(),
                                                 (nb[0] == 0).float()]))
    finally:
        cx.set_encode_path(0)
        cx.set_copy_k(0)
    v = torch.stack(verdicts).cpu().numpy()
    assert len(v) == 52 and bool((v == 1).all()), np.nonzero(v != 1)


# ---- 9. the receive pipeline with and without the check -----------------------------------------------
@pytest.mark.parametrize("verify", [True, False])
def test_pipeline_drops_corrupted_payloads(cx, gpu, verify):
    """Ethernet wire packets, one payload byte (not byte 0, the only byte the tag covers) flipped in every
    7th, then parse_decode -> verify in place -> demux -> deliver: exactly the untouched packets' payloads
    arrive.  Without the verify step the corrupted payloads are delivered too: the gap the check closes."""
    import torch

    from rsock_amd.codec import DecodeBuffers, DeliverBuffers, DemuxBuffers, TcpInfoBuffers
    from tests.test_demux_oracle import ALL

    n = 4000
    d = workload.describe("c4", 0, n, n=n)
    w = workload.DeviceWorkload(d, gpu)
    g = torch.Generator(device=gpu)
    g.manual_seed(9)
    ri = lambda hi, dt: torch.randint(0, hi, (n,), device=gpu, generator=g, dtype=torch.int64).to(dt)  # noqa: E731
    fields = [ri(2**31, torch.int32), ri(2**31, torch.int32), ri(2**15, torch.int16) + 1, ri(2**15, torch.int16) + 1,
              ri(2**31, torch.int32), ri(2**31, torch.int32), torch.full((n,), 0x18, dtype=torch.uint8, device=gpu),
              ri(2**15, torch.int16)]
    plen = d.pay_len.astype(np.int64)
    wl = 54 + 31 + plen
    woff_h = np.concatenate([[0], np.cumsum(wl)[:-1]])  # back to back: every alignment
    wire = torch.zeros(int(wl.sum()), dtype=torch.uint8, device=gpu)
    woff = dev(woff_h, gpu)
    st = torch.empty(n, dtype=torch.int32, device=gpu)
    eth = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
    cx.output_wire_batch(w.payload, w.pay_off, w.pay_len, w.cmd, w.conv, w.conn_key, *fields, wire, woff, st, eth=eth,
                         id_uniform=workload.ID_UNIFORM)
    rng = np.random.default_rng(9)
    hit = np.arange(3, n, 7)
    at = woff_h[hit] + 85 + 1 + (rng.random(len(hit)) * (plen[hit] - 1)).astype(np.int64)
    wire[dev(at, gpu)] ^= 0x40
    tcp, dec = TcpInfoBuffers.alloc(n, gpu), DecodeBuffers.alloc(n, gpu)
    cx.rawinput_batch(wire, woff, st, st, 1, 0, tcp, dec)
    torch.cuda.synchronize()
    assert bool((dec.status == 1).all()), "the tag does not see the flipped bytes"
    csum = torch.empty(n, dtype=torch.uint8, device=gpu)
    nb = torch.zeros(1, dtype=torch.int32, device=gpu)
    if verify:
        cx.verify_wire_batch(wire, woff, st, A.DLT_EN10MB, csum, status=dec.status, status_out=dec.status, n_bad=nb)
    dmx = DemuxBuffers.alloc(n, gpu)
    cx.demux_batch(dec.status, dec.cmd, ALL | A.DEMUX_CMD_BARRIER, dmx, id=dec.id, conv=dec.conv, conn_key=dec.conn_key,
                   dst=tcp.dst)
    out = DeliverBuffers.alloc(n, gpu, int(plen.sum()))
    cx.deliver_batch(wire, woff, dec.pay_off, dec.pay_len, dec.status, out, inner_off=tcp.cap_pay_off, order=dmx.perm,
                     n_order=dmx.n_valid)
    torch.cuda.synchronize()
    clean = np.ones(n, bool)
    clean[hit] = False
    nv = int(dmx.n_valid.item())
    perm = dmx.perm[:nv].cpu().numpy().view(np.uint32)
    payload = workload.payload_bytes_np(d)
    orig = lambda i: payload[int(d.pay_off[i]): int(d.pay_off[i]) + int(d.pay_len[i])]  # noqa: E731
    got = out.arena.cpu().numpy()[:int(out.total.item())]
    if verify:
        assert int(nb.item()) == len(hit)
        assert np.array_equal(dec.status.cpu().numpy(), np.where(clean, 1, -1))
        assert np.array_equal(csum.cpu().numpy() == R.ALL_OK, clean)
        assert sorted(perm.tolist()) == np.nonzero(clean)[0].tolist()
        assert np.array_equal(got, np.concatenate([orig(i) for i in perm]))
    else:
        assert nv == n and len(got) == int(plen.sum())
        want = np.concatenate([orig(i) for i in perm])
        assert int((got != want).sum()) == len(hit), "every corrupted payload byte is delivered unnoticed"


# ---- 10. captured graph -----------------------------------------------------------------------------
def test_verify_in_captured_graph(cx, gpu):
    """A verify captured on a side stream of a fresh context, with no reserve: replayed, then replayed
    again after a byte of the arena and a status changed -- the outputs follow the inputs.  (The eager
    call on the module's context first only makes sure the kernel's code object is loaded.)"""
    import torch

    from rsock_amd.codec import Codec

    check(cx, gpu, V.sized_case(9))
    c = V.gated_case(R.DLT_EN10MB)
    cxg = Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        arena, off, cl = dev(c.arena, gpu), dev(c.cap_off, gpu, np.int64), dev(c.cap_len, gpu, np.int32)
        st = dev(c.status, gpu)
        so = torch.empty(c.n, dtype=torch.int8, device=gpu)
        csum = torch.empty(c.n, dtype=torch.uint8, device=gpu)
        nb = torch.empty(1, dtype=torch.int32, device=gpu)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            cxg.verify_wire_batch(arena, off, cl, c.datalink, csum, status=st, status_out=so, n_bad=nb,
                                  stream=torch.cuda.current_stream())
        good = int(np.nonzero((c.status == 1) & ~R.is_bad(c.expected()[0]))[0][0])
        for r in range(2):
            if r:  # corrupt a good packet's last byte, and gate another packet out
                c.arena[int(c.cap_off[good]) + int(c.cap_len[good]) - 1] ^= 0x80
                c.status[int(np.nonzero(c.status == 1)[0][-1])] = 0
                arena.copy_(dev(c.arena, gpu))
                st.copy_(dev(c.status, gpu))
            csum.fill_(FILL)
            so.fill_(0x55)
            nb.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want, wst, wbad = c.expected()
            assert np.array_equal(csum.cpu().numpy(), want), r
            assert np.array_equal(so.cpu().numpy(), wst) and int(nb.item()) == wbad, r
            assert r == 0 or (want[good] == R.ALL_OK & ~R.TCP_OK and wst[good] == -1)
        del g
    finally:
        cxg.close()


# ---- 11. host and device agree ----------------------------------------------------------------------
@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_host_twin_matches_device(cx, gpu, datalink):
    from rsock_amd.codec import verify_wire_host

    for pad in range(16):
        c = V.alignment_case(datalink, pad)
        h = verify_wire_host(c.arena, c.cap_off, c.cap_len, datalink)
        got, _, gbad = run_gpu(cx, gpu, c)
        assert np.array_equal(got, h[0]) and gbad == h[2]
