"""GPU: the conv table on the device (rsk_conv_index_build, rsk_conv_resolve_batch, rsk_conv_send_batch,
rsk_conv_flush; include/rsk_codec.h) against tests/conv_ref: the scenarios of tests/test_conv_host.py on the
device (the reference's leaves and conv resets, batch sizes and capacities, exact counts under skew,
CONV_RST and the snapshot rule, poisoned columns, optional outputs, send, flush), the index built on either
side, the whole receive chain down to delivered bytes, a captured graph, and the argument checks."""
from __future__ import annotations

import numpy as np
import pytest

from rsock_amd import _abi as A
from rsock_amd import codec as rc
from rsock_amd import workload
from tests import conn_ref as CR
from tests import conv_ref as R

pytestmark = pytest.mark.gpu

KEY = b"hello135"


@pytest.fixture(scope="module")
def cx(gpu):
    c = rc.Codec(KEY, 0)
    yield c
    c.close()


def u32(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("name", sorted(R.GOLDEN_CLIENT_MSGS))
def test_reference_pin_client(cx, gpu, name):
    R.scenario_golden_client(rc, name, gpu, cx)


@pytest.mark.parametrize("name", R.GOLDEN_SERVER)
def test_reference_pin_server(cx, gpu, name):
    import torch

    def demux_first(c, unknown):
        """rsk_demux_batch on the unknown column: seg_first lists the new keys in first-arrival order."""
        n = len(unknown)
        dmx = rc.DemuxBuffers.alloc(n, gpu)
        t = lambda k: R.tensor(c[k], gpu)  # noqa: E731
        cx.demux_batch(R.tensor(unknown, gpu), t("cmd"), A.DEMUX_ID | A.DEMUX_DST | A.DEMUX_CONV, dmx, id=t("id"),
                       conv=t("conv"), dst=t("dst"))
        torch.cuda.synchronize()
        return u32(dmx.seg_first)[:int(u32(dmx.n_seg)[0])].astype(np.int64)

    R.scenario_golden_server(rc, name, gpu, cx, first_fn=demux_first)


@pytest.mark.parametrize("capacity", R.CAPACITIES)
@pytest.mark.parametrize("n", R.SIZES)
def test_sizes(cx, gpu, n, capacity):
    R.scenario_sizes(rc, n, capacity, gpu, cx)


@pytest.mark.parametrize("by_dst,by_id", R.FLAG_COMBOS)
def test_flag_combinations(cx, gpu, by_dst, by_id):
    R.scenario_sizes(rc, 4097, 257, gpu, cx, by_dst=by_dst, by_id=by_id)


@pytest.mark.parametrize("kind", ["one_row", "all_rows", "alternate", "runs"])
def test_skew(cx, gpu, kind):
    R.scenario_skew(rc, kind, gpu, cx)


BAND_TABLES = {}


@pytest.mark.parametrize("pattern", R.BAND_PATTERNS)
@pytest.mark.parametrize("n", R.BAND_SIZES)
@pytest.mark.parametrize("call", ["resolve", "send"])
def test_counts_on_colliding_rows(cx, gpu, call, n, pattern):
    """tile_count_rows "exact under any skew", on the skew of many rows: 2048 distinct rows of one tile whose
    entries in the LDS table all start inside one band of 40 across the table's end (one run of 2048 entries),
    every row three times, and half a tile on one row; cur_in / cur_out from just below the 32-bit wrap."""
    R.scenario_band_counts(rc, call, n, pattern, gpu, cx, cache=BAND_TABLES)


def test_conv_rst(cx, gpu):
    R.scenario_conv_rst(rc, gpu, cx)


def test_reads(cx, gpu):
    R.scenario_reads(rc, gpu, cx)


def test_optional_outputs(cx, gpu):
    R.scenario_optional_outputs(rc, gpu, cx)


def test_send(cx, gpu):
    R.scenario_send(rc, gpu, cx)


def test_send_skew(cx, gpu):
    """cur_out exact with every packet on one row, and with every packet on another row."""
    rng = np.random.default_rng(5)
    cap = 65536
    cols = R.random_columns(rng, cap, False, False)
    cols["state"][:] = A.CONN_LIVE
    cols["cur_out"][:] = 0xFFFFFFF0
    tab = R.make_table(rc, cols, gpu, False, False, cx)
    one, every = np.full(70000, 4242, np.uint32), rng.permutation(cap).astype(np.uint32)
    R.run_send(rc, tab, one, gpu, cx, sent=np.full(70000, 100, np.int32), cols=())
    R.run_send(rc, tab, every, gpu, cx, sent=np.full(cap, 100, np.int32), cols=())
    want = np.full(cap, 0xFFFFFFF1, np.uint32)
    want[4242] = (0xFFFFFFF1 + 70000) & 0xFFFFFFFF
    assert np.array_equal(tab.column("cur_out"), want)


@pytest.mark.parametrize("capacity", [1, 1000, 65536])
def test_flush_steps(cx, gpu, capacity):
    R.scenario_flush_steps(rc, capacity, gpu, cx)


def test_flush_life(cx, gpu):
    R.scenario_flush_life(rc, gpu, cx)


def test_device_argument_errors_and_empty_batch(cx, gpu):
    R.check_einval(rc, gpu, cx)


@pytest.mark.parametrize("by_dst,by_id", [(False, False), (True, True)])
def test_index_built_on_either_side(cx, gpu, by_dst, by_id):
    """The index built on the host and copied to the device resolves the same as the device-built one, and
    the reverse; n_dup agrees."""
    import torch

    rng = np.random.default_rng(77)
    cols, c = R.random_case(rng, 6000, 5000, by_dst, by_id, pool=3000)
    want = R.resolve_ref(cols, by_dst, by_id, c)
    _tmap, dup = R.table_map(cols, by_dst, by_id)
    host_tab = R.make_table(rc, cols, "cpu", by_dst, by_id)
    dev_tab = R.make_table(rc, cols, gpu, by_dst, by_id, cx)
    nd = torch.zeros(1, dtype=torch.int32, device=gpu)
    dev_tab.rebuild(cx, n_dup=nd)
    torch.cuda.synchronize()
    assert int(u32(nd)[0]) == dup > 0
    moved_up, moved_down = host_tab.to(gpu), dev_tab.to("cpu")
    for tab, side in ((moved_up, cx), (moved_down, None), (dev_tab, cx)):
        got = R.run_resolve(rc, tab, c, gpu if side else "cpu", side)
        R.compare(got, want)


def test_receive_chain_to_delivered_bytes(cx, gpu):
    """parse_decode -> verify -> conn resolve -> control -> conv resolve -> demux -> deliver over a wire batch:
    every segment's conv_row[seg_first] names the row whose bytes it holds."""
    import torch

    n, nconn, nconv, cap = 6000, 8, 12, 40
    rng = np.random.default_rng(30)
    d = workload.describe("c4", 0, n, n=n)
    w = workload.DeviceWorkload(d, gpu)
    e = lambda dt, k=n: torch.empty(k, dtype=dt, device=gpu)  # noqa: E731
    a_ip, b_ip = rc.ip_u32("10.0.0.1"), rc.ip_u32("10.0.0.2")
    # the sender's and the receiver's connection tables (a client's: keyed by connKey alone)
    sp, dp = 40000 + np.arange(nconn), 10001 + np.arange(nconn) % 10
    keys = (0x10000000 | (dp << 16) | sp).astype(np.uint64)
    a_cols = CR.random_columns(rng, nconn)
    CR.place(a_cols, np.arange(nconn), keys)
    a_cols["src"][:], a_cols["dst"][:], a_cols["sp"][:], a_cols["dp"][:], a_cols["flag"][:] = a_ip, b_ip, sp, dp, 0x18
    b_cols = {k: (None if v is None else v.copy()) for k, v in a_cols.items()}
    b_cols["state"][nconn - 1] = 0  # the receiver lacks one conn: its packets never reach the conv level
    ta, tb = CR.make_table(rc, a_cols, nconn, gpu), CR.make_table(rc, b_cols, nconn, gpu)
    ta.rebuild(cx)
    tb.rebuild(cx)
    # the receiver's conv table: a SubGroup's keys (dst, conv), dst being the parse's TcpInfo dst -- the packet's
    # source address, RawInput stores the info reversed; two of the convs in flight are unknown to it
    convs = rng.integers(1, 2**32, nconv, dtype=np.uint64).astype(np.uint32)
    ccols = R.random_columns(rng, cap, True, False)
    crow = rng.permutation(cap)[:nconv - 2]
    ccols["conv"][crow], ccols["dst"][crow], ccols["state"][crow] = convs[:nconv - 2], a_ip, A.CONN_LIVE
    ccols["cur_in"][:] = 0
    ctab = R.make_table(rc, ccols, gpu, True, False, cx)
    pick = rng.integers(0, nconv, n)
    conv = R.tensor(convs[pick], gpu)
    conn_h = rng.integers(0, nconn, n).astype(np.uint32)
    conn = R.tensor(conn_h, gpu)
    # send
    x = {"src": e(torch.int32), "dst": e(torch.int32), "sp": e(torch.int16), "dp": e(torch.int16), "ack": e(torch.int32),
         "flag": e(torch.uint8), "conn_key": e(torch.int64)}
    ok = e(torch.uint8)
    cx.conn_expand_batch(ta, conn, ok, **x)
    seq, ipid, ipn = e(torch.int32), e(torch.int16), torch.zeros(1, dtype=torch.int16, device=gpu)
    cx.tcp_send_seq_batch(conn, 31 + w.pay_len.to(torch.int32), ta.seq, ipn, seq, ipid)
    wl = 54 + 31 + d.pay_len.astype(np.int64)
    woff = torch.from_numpy(np.concatenate([[0], np.cumsum(wl)[:-1]])).to(gpu)
    wire = torch.zeros(int(wl.sum()) + 64, dtype=torch.uint8, device=gpu)
    wst = e(torch.int32)
    eth = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
    cx.output_wire_batch(w.payload, w.pay_off, w.pay_len, w.cmd, conv, x["conn_key"], x["src"], x["dst"], x["sp"], x["dp"],
                         seq, x["ack"], x["flag"], ipid, wire, woff, wst, eth=eth, id_uniform=workload.ID_UNIFORM)
    # receive
    tcp, dec = rc.TcpInfoBuffers.alloc(n, gpu), rc.DecodeBuffers.alloc(n, gpu)
    cx.rawinput_batch(wire, woff, wst, wst, A.DLT_EN10MB, 0, tcp, dec)
    csum = e(torch.uint8)
    cx.verify_wire_batch(wire, woff, wst, A.DLT_EN10MB, csum, status=dec.status, status_out=dec.status)
    rconn, hit = e(torch.int32), e(torch.uint8)
    cx.conn_resolve_batch(tb, dec.status, dec.conn_key, rconn, cmd=dec.cmd, hit=hit)
    ctl = rc.ControlBuffers.alloc(n, gpu, capacity=nconn)
    cx.control_batch(tb, dec.status, dec.cmd, dec.pay_off, dec.pay_len, wire, woff, ctl, id=dec.id, conn_key=dec.conn_key,
                     inner_off=tcp.cap_pay_off)
    conv_row, unknown, n_unk = e(torch.int32), e(torch.int8), e(torch.int32, 1)
    rst_first = e(torch.int32, cap)
    msgs = rc.ControlBuffers.alloc(n, gpu)
    cx.conv_resolve_batch(ctab, dec.status, dec.conv, conv_row, cmd=dec.cmd, hit=hit, id=dec.id, dst=tcp.dst,
                          ctl_kind=ctl.kind, ctl_arg=ctl.arg, unknown=unknown, n_unknown=n_unk, rst_first=rst_first, msgs=msgs)
    found = torch.where(conv_row != -1, 1, -1).to(torch.int8) * (dec.cmd == 0).to(torch.int8)
    dmx = rc.DemuxBuffers.alloc(n, gpu)
    cx.demux_batch(found, dec.cmd, A.DEMUX_DST | A.DEMUX_CONV, dmx, conv=dec.conv, dst=tcp.dst)
    out = rc.DeliverBuffers.alloc(n, gpu, int(d.pay_len.astype(np.int64).sum()))
    cx.deliver_batch(wire, woff, dec.pay_off, dec.pay_len, found, out, inner_off=tcp.cap_pay_off, order=dmx.perm,
                     n_order=dmx.n_valid)
    torch.cuda.synchronize()
    assert bool((ok == 1).all()) and np.array_equal(wst.cpu().numpy(), wl) and bool((dec.status == 1).all())
    # the restatement
    data, reached = d.cmd == 0, conn_h != nconn - 1
    known = pick < nconv - 2
    row_of = np.full(nconv, R.NONE, np.uint32)
    row_of[:nconv - 2] = crow
    rows = u32(conv_row)
    want_rows = np.where(data & reached, row_of[pick], R.NONE)
    is_rst = d.cmd == 1  # its body is payload bytes: whatever conv they spell, the column says what was found
    assert np.array_equal(rows[~is_rst], want_rows[~is_rst]) and is_rst.sum() > 0
    unk = data & reached & ~known
    assert np.array_equal(unknown.cpu().numpy() == 1, unk) and int(u32(n_unk)[0]) == int(unk.sum()) > 0
    m = msgs.messages()
    assert np.array_equal(m["src"], np.nonzero(unk)[0].astype(np.uint32)) and np.array_equal(m["body"], convs[pick][unk].astype(np.uint64))
    assert bool((m["pay_len"] == 4).all()) and bool((m["cmd"] == A.CMD_CONV_RST).all())
    assert np.array_equal(m["id"], np.tile(np.frombuffer(workload.ID_UNIFORM, np.uint8), (len(m["src"]), 1)))
    assert np.array_equal(ctab.column("cur_in"), np.bincount(rows[data & (rows != R.NONE)].astype(np.int64), minlength=cap))
    # every segment holds one row's packets in arrival order, and its bytes are their payloads
    payload = workload.payload_bytes_np(d)
    arena = out.arena.cpu().numpy()
    segs = dmx.segments()
    assert len(segs) == nconv - 2
    for s, (first, idx) in enumerate(segs):
        r = rows[first]
        assert r != R.NONE and idx == np.nonzero(data & (rows == r))[0].tolist()
        want = np.concatenate([payload[int(d.pay_off[i]):int(d.pay_off[i]) + int(d.pay_len[i])] for i in idx])
        assert np.array_equal(rc.segment_bytes(arena, out.out_off, dmx, s), want)


def test_resolve_and_flush_in_captured_graph(cx, gpu):
    """Resolve (with messages) + flush captured as one linear chain on a side stream of a fresh context after
    a reserve and one eager call; replayed twice: outputs equal, cur_in advanced twice."""
    import torch

    rng = np.random.default_rng(40)
    n, cap = 5000, 300
    cols, c = R.random_case(rng, n, cap, True, True, pool=80)
    want = R.resolve_ref(cols, True, True, c)
    tab = R.make_table(rc, cols, gpu, True, True, cx)
    t = {k: R.tensor(v, gpu) for k, v in c.items()}
    cxg = rc.Codec(KEY, 0)
    try:
        s = torch.cuda.Stream(gpu)
        cxg.reserve(n, stream=s)
        e = lambda dt, k=n: torch.empty(k, dtype=dt, device=gpu)  # noqa: E731
        o = {"conv_row": e(torch.int32), "unknown": e(torch.int8), "n_unknown": e(torch.int32, 1), "rst_first": e(torch.int32, cap)}
        msgs = rc.ControlBuffers.alloc(n, gpu)
        dead, nd, na = e(torch.int32, cap), e(torch.int32, 1), e(torch.int32, 1)
        kw = dict(cmd=t["cmd"], hit=t["hit"], id=t["id"], dst=t["dst"], ctl_kind=t["ctl_kind"], ctl_arg=t["ctl_arg"], msgs=msgs, **o)

        def chain(codec, stream=None):
            codec.conv_resolve_batch(tab, t["status"], t["conv"], stream=stream, **kw)
            codec.conv_flush(tab, dead_rows=dead, n_dead=nd, n_alive=na, stream=stream)

        with torch.cuda.stream(s):
            chain(cxg)  # the eager call: loads the kernels and runs the chain once
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            chain(cxg, torch.cuda.current_stream())
        state = dict(cols, cur_in=cols["cur_in"] + want["add"])
        new, dead_ref, n_alive = R.flush_ref(state)
        state.update(new)
        for rep in range(2):
            for x in list(o.values()) + [msgs.msg_body, msgs.msg_src, msgs.n_msg, dead, nd, na]:
                x.view(torch.uint8).fill_(R.SENT)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            state["cur_in"] = state["cur_in"] + want["add"]
            assert np.array_equal(tab.column("cur_in"), state["cur_in"]), rep
            new, dead_ref, n_alive = R.flush_ref(state)
            state.update(new)
            assert np.array_equal(u32(o["conv_row"]), want["conv_row"]) and int(u32(o["n_unknown"])[0]) == want["n_unknown"]
            assert np.array_equal(o["unknown"].cpu().numpy(), want["unknown"]) and np.array_equal(u32(o["rst_first"]), want["rst_first"])
            got = msgs.messages()
            assert np.array_equal(got["body"], want["msgs"]["body"]) and np.array_equal(got["src"], want["msgs"]["src"])
            assert np.array_equal(u32(dead)[:int(u32(nd)[0])], dead_ref) and int(u32(na)[0]) == n_alive
            for k in ("alive", "prev_in", "prev_out"):
                assert np.array_equal(tab.column(k), state[k]), (rep, k)
        del g
    finally:
        cxg.close()
