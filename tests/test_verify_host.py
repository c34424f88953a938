"""CPU: rsk_verify_wire_host (the host twin of rsk_verify_wire_batch, include/rsk_codec.h) against
tests/csum_ref, on the shapes of tests/verify_cases; and csum_ref itself pinned to the oracle's RFC 1071
sum (orc_inet_csum) and to the packets the oracle's wire build writes."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from tests import csum_ref as R
from tests import verify_cases as V


def check_host(c: V.Case, nthreads: int = 1):
    want, wst, wbad = c.expected()
    got, gst, gbad = rc.verify_wire_host(c.arena, c.cap_off, c.cap_len, c.datalink, status=c.status,
                                         want_status_out=c.status is not None, nthreads=nthreads)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])
    assert gbad == wbad
    if c.status is not None:
        assert np.array_equal(gst, wst)
    return want


# ---- the reference itself ---------------------------------------------------------------------------
def test_ref_sum_is_the_oracles(oracle):
    rng = np.random.default_rng(1)
    for ln in list(range(0, 65)) + [1479, 1480, 1481]:
        for _ in range(3):
            b = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
            assert R.halfword_sum(b) == (~oracle.L.orc_inet_csum(b, ln, 0)) & 0xFFFF, ln
    assert R.halfword_sum(b"") == 0 and R.halfword_sum(b"\xff\xff") == 0xFFFF
    assert R.halfword_sum(b"\xff\xff\xff\xff\x00\x01") == 1


@pytest.mark.parametrize("eth", [False, True])
def test_ref_accepts_the_oracles_wire_packets(oracle, eth):
    from rsock_amd import workload

    rng = np.random.default_rng(2)
    ethb = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + b"\x08\x00" if eth else None
    dl = R.DLT_EN10MB if eth else R.DLT_RAW
    pkts = []
    for P in (1, 2, 17, 1469):
        for _ in range(4):
            st, frame = oracle.rconn_output(b"hello135", rng.integers(0, 256, P, dtype=np.uint8).tobytes(),
                                            int(rng.integers(0, 5)), workload.ID_UNIFORM, int(rng.integers(0, 2**32)),
                                            int(rng.integers(0, 2**63)))
            assert st == 31 + P
            f = [int(rng.integers(0, hi)) for hi in (2**32, 2**32, 65536, 65536, 2**32, 2**32, 256, 65536)]
            pkts.append(oracle.build_wire(frame, *f, eth=ethb))
    for p in pkts:
        assert R.verify_one(p, len(p), dl) == R.ALL_OK
    c = V.Case(*V.pack(pkts, base_pad=1), dl)
    assert bool((check_host(c) == R.ALL_OK).all())


@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_ref_batch_form_equals_packet_form(datalink):
    """verify_ref (prefix sums over the arena) against verify_one (the rule as written), packet by packet."""
    for c in (V.alignment_case(datalink, 3), V.ladder_case(datalink), V.carries_case(datalink)):
        want = c.expected()[0]
        pad = np.concatenate([c.arena, np.zeros(70000, np.uint8)])  # verify_one slices past a cut cap_len
        for i in range(c.n):
            o = int(c.cap_off[i])
            assert R.verify_one(pad[o:o + 66000].tobytes(), int(c.cap_len[i]), datalink) == want[i], i


# ---- the host twin ----------------------------------------------------------------------------------
@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_host_alignment_and_lengths(datalink):
    seen = set()
    for pad in range(16):
        c = V.alignment_case(datalink, pad)
        want = check_host(c)
        seen |= set((c.cap_off % 16).tolist())
        assert 0 < R.is_bad(want).sum() < c.n
    assert seen == set(range(16))


def test_host_every_byte_counts():
    c, where = V.every_byte_case()
    want = check_host(c)
    assert want[0] == R.ALL_OK
    assert_right_bit(want, where)


def assert_right_bit(csum, where):
    """Packet 1 + j has a bit of byte where[j] flipped: outside the bytes the rule branches on, exactly
    the checksum(s) covering that byte fail."""
    L = 14
    for j, k in enumerate(where):
        if k - L in (0, 2, 3, 6, 7, 9):  # version / ihl, total length, fragment word, protocol
            continue
        lost = R.IP_OK if k < L + 20 else R.TCP_OK
        if L + 12 <= k < L + 20:
            lost = R.IP_OK | R.TCP_OK  # the addresses are in the header and in the pseudo-header
        assert csum[1 + j] == R.ALL_OK & ~lost, (k, csum[1 + j])


def test_host_nothing_outside_counts():
    a, b = check_host(V.neighbours_case(0x00)), check_host(V.neighbours_case(0xFF))
    assert np.array_equal(a, b) and bool((a == R.ALL_OK).all())


@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_host_carries(datalink):
    assert bool((check_host(V.carries_case(datalink)) == R.ALL_OK).all())


@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_host_ladder(datalink):
    want = check_host(V.ladder_case(datalink))
    assert want[0] == R.ALL_OK and (want == 0).sum() >= 6 and (want & R.TCP_TRUNC).any()
    assert bool((want[(want & R.TCP_TRUNC) != 0] == (R.IP_CHECKED | R.IP_OK | R.TCP_TRUNC)).all())


@pytest.mark.parametrize("datalink", V.DATALINKS)
def test_host_gating(datalink):
    c = V.gated_case(datalink)
    want = check_host(c)
    assert bool((want[c.status != 1] == 0).all()) and (want != 0).any()


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 70001])
def test_host_sizes(n):
    check_host(V.sized_case(n), nthreads=4 if n > 4096 else 1)


def test_host_argument_errors_and_empty_batch():
    import ctypes

    c = V.sized_case(9)
    csum, st, nb = np.zeros(9, np.uint8), np.ones(9, np.int8), np.full(1, 7, np.uint32)
    L = rc.lib()

    def structs():
        return (A.VerifyIn(c.arena.ctypes.data, c.cap_off.ctypes.data, c.cap_len.ctypes.data, None),
                A.VerifyOut(csum.ctypes.data, None, nb.ctypes.data))

    def call(vin, vout, n=9, dl=R.DLT_EN10MB):
        return L.rsk_verify_wire_host(n, ctypes.byref(vin) if vin else None, dl, ctypes.byref(vout) if vout else None, 1)

    assert call(*structs()) == A.OK
    assert call(None, structs()[1]) == A.EINVAL and call(structs()[0], None) == A.EINVAL
    for f in ("cap_arena", "cap_off", "cap_len"):
        vin, vout = structs()
        setattr(vin, f, None)
        assert call(vin, vout) == A.EINVAL, f
    vin, vout = structs()
    vout.csum = None
    assert call(vin, vout) == A.EINVAL
    vin, vout = structs()
    vout.status_out = st.ctypes.data  # status_out without status
    assert call(vin, vout) == A.EINVAL
    for dl in (-1, 2, 11, 13, 113):
        assert call(*structs(), dl=dl) == A.EINVAL, dl
    nb[0] = 7
    assert call(A.VerifyIn(None, None, None, None), A.VerifyOut(None, None, nb.ctypes.data), n=0) == A.OK and nb[0] == 0
    assert call(A.VerifyIn(None, None, None, None), A.VerifyOut(None, None, None), n=0) == A.OK
    assert A.DLT_RAW == 12 and (A.CSUM_IP_CHECKED, A.CSUM_IP_OK, A.CSUM_TCP_CHECKED, A.CSUM_TCP_OK,
                                A.CSUM_TCP_TRUNC) == (R.IP_CHECKED, R.IP_OK, R.TCP_CHECKED, R.TCP_OK, R.TCP_TRUNC)
