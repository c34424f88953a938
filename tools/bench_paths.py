#!/usr/bin/env python3
"""Per-path kernel timings on one config (device-resident, HIP events, interleaved rounds in one
process): encode (framing), encode_wire RAW4 / Ethernet (framing + IPv4/TCP build + checksums),
decode (verify + compaction), parse_decode (pcap parse of the Ethernet wire packets + verify), ...,
deliver / deliver_demux / deliver_plan (the VALID payloads packed in valid_idx / demux order; offsets only),
verify_wire_eth / verify_wire_raw4 (IPv4 + TCP checksum check of the wire packets built above),
conn_resolve / conn_resolve_64conn / conn_resolve_miss / conn_expand (the connection table: the decoded
batch against its own connKeys, 64 connections, half of the keys absent; the send side's gather) /
control_<config> / control_dense / keepalive_flush_28k / keepalive_flush_1m (control packets and the
keepalive timer on the connection table; the _kind rows write kind and the messages only) /
conv_per_conn / conv_bursts / conv_one / conv_each (+ _nocount) / conv_flush_1m (the conv table: one conv per
connection of the batch, the same in runs of 37 neighbours, one conv for all packets, another conv per packet
over 2^20 rows, each with and without the
cur_in counts; IGroup::Flush over 2^20 rows) /
conv_close_none / conv_close_rst / conv_close_timer_1m / conv_old_close / conv_old_close_1m (rsk_conv_close_batch
with no reset hitting, with 1 % of the convs reset, behind the flush of 2^20 rows, and the index rebuild it replaces) /
conn_create_none / _all / _1pct / conn_create_list_1m (+ _by_id) / conn_old_create_* (rsk_conn_create_batch: conns
born on the device table against the demux + both builds + second resolve it replaces),
conn_close_none / conn_close_rst / conn_close_timer_1m (+ _by_id) / conn_old_* (rsk_conn_close_batch with the pick
index kept current: nothing marked, 1 % of the batch's conns reset and removed, a fifth of 2^20 rows timed out and
removed, and the rsk_conn_index_build + rsk_conn_pick_build they replace) /
conv_resolve_unknown / conv_create_none / conv_create_born / conv_old_born (rsk_conv_create_batch on the one-conv-
per-connection column: no packet unknown beside the resolve alone, every conv born in the call on an empty table,
and the demux + index build + second resolve that the same outcome takes without the call) /
conn_pick_client (+ _lds) / conn_pick_server / conn_pick_own_one (+ _lds) / conn_pick_own_groups /
conn_pick_avoid / conn_pick_build_1m (+ _by_id) (the send pick: one group of 10 conns with the candidates from
global memory and staged in LDS, 64 groups of 10, the batch's own conns as one group and as groups of 10, an
avoid key on every packet, the index build over 2^20 rows; the host twin with 16 threads beside them).
    python tools/bench_paths.py [--config c3] [--rounds 5] [--reps 10]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--packets", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--wire-align", type=int, default=0,
                    help="wire packet pitch alignment (bytes); 0 = the frame slot rule (128 with PAD128 for "
                         "mixed lengths, else 16)")
    ap.add_argument("--only", default="", help="time only these paths (comma list; a trailing * matches a prefix), e.g. demux,demux_64conn")
    ap.add_argument("--copy-yardstick", action="store_true",
                    help="also time tools/libhbm_probe.so's dense 16-B copy of the delivered byte count (rows "
                         "dense_copy@GRID) and report deliver's time over the fastest of them")
    ap.add_argument("--read-yardstick", action="store_true",
                    help="also time tools/libhbm_probe.so's dense 16-B read of the byte count verify_wire_eth sums "
                         "(rows dense_read@GRID) and report the verify rows' times over the fastest of them")
    ap.add_argument("--encode-path", type=int, default=0,
                    help="rsk_set_encode_path for the encode paths: 0 chosen per call, 1 k_encode, 2 two-pass, 3 short")
    args = ap.parse_args()
    import torch

    from rsock_amd import codec as rc
    from rsock_amd import workload

    dev = torch.device("cuda:0")
    n = args.packets or workload.CONFIGS[args.config][1]
    d = workload.describe(args.config, 0, n, n=n)
    w = workload.DeviceWorkload(d, dev)
    cx = rc.Codec(b"hello135", 0)
    if args.encode_path:
        cx.set_encode_path(args.encode_path)
    cx.reserve(n)
    s = torch.cuda.current_stream()
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    ri = lambda hi, dt: torch.randint(0, hi, (n,), device=dev, generator=g, dtype=torch.int64).to(dt)  # noqa: E731
    src, dst, seq, ack = ri(2**31, torch.int32), ri(2**31, torch.int32), ri(2**31, torch.int32), ri(2**31, torch.int32)
    sp, dp, ipid = ri(2**15, torch.int16) + 1, ri(2**15, torch.int16) + 1, ri(2**15, torch.int16)
    flag = torch.full((n,), 0x18, dtype=torch.uint8, device=dev)
    pmax = workload.CONFIGS[args.config][3]
    al = args.wire_align or (128 if d.pad == 128 else 16)
    wpad = dict(pad16=al != 128, pad128=al == 128)
    p4, pe = (40 + 31 + pmax + al - 1) // al * al, (54 + 31 + pmax + al - 1) // al * al
    wire4 = torch.empty(n * p4, dtype=torch.uint8, device=dev)
    wiree = torch.empty(n * pe, dtype=torch.uint8, device=dev)
    off4 = torch.arange(n, device=dev, dtype=torch.int64) * p4
    offe = torch.arange(n, device=dev, dtype=torch.int64) * pe
    st4 = torch.empty(n, dtype=torch.int32, device=dev)
    ste = torch.empty(n, dtype=torch.int32, device=dev)
    eth = bytes([2, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 2, 8, 0])
    tcp = rc.TcpInfoBuffers.alloc(n, dev)
    pdec = rc.DecodeBuffers.alloc(n, dev)
    common = (w.payload, w.pay_off, w.pay_len, w.cmd, w.conv, w.conn_key)
    ops = {
        "encode": lambda: cx.output_batch(*common, w.frame, w.frame_off, w.status, id_uniform=workload.ID_UNIFORM,
                                          pad16=d.pad == 16, pad128=d.pad == 128, stream=s),
        "encode_wire_raw4": lambda: cx.output_wire_batch(*common, src, dst, sp, dp, seq, ack, flag, ipid, wire4, off4,
                                                         st4, id_uniform=workload.ID_UNIFORM, stream=s, **wpad),
        "encode_wire_eth": lambda: cx.output_wire_batch(*common, src, dst, sp, dp, seq, ack, flag, ipid, wiree, offe,
                                                        ste, eth=eth, id_uniform=workload.ID_UNIFORM, stream=s,
                                                        **wpad),
        # the per-set wire kernels held (round 6: AUTO takes the two-pass wire build for long frames)
        "encode_wire_raw4_perset": lambda: (cx.set_encode_path(1), cx.output_wire_batch(
            *common, src, dst, sp, dp, seq, ack, flag, ipid, wire4, off4, st4, id_uniform=workload.ID_UNIFORM,
            stream=s, **wpad), cx.set_encode_path(0)),
        "encode_wire_eth_perset": lambda: (cx.set_encode_path(1), cx.output_wire_batch(
            *common, src, dst, sp, dp, seq, ack, flag, ipid, wiree, offe, ste, eth=eth, id_uniform=workload.ID_UNIFORM,
            stream=s, **wpad), cx.set_encode_path(0)),
        "decode": lambda: cx.onrecv_batch(w.frame, w.frame_off, w.frame_len, w.dec, stream=s),
        "parse_decode": lambda: cx.rawinput_batch(wiree, offe, ste, ste, 1, 0, tcp, pdec, stream=s),
    }
    # fake-TCP connection state: seq / IP id of a send batch over 64 connections, ack of a receive batch
    conn64 = (torch.arange(n, device=dev, dtype=torch.int64) % 64).to(torch.int32)
    cseq, cack = torch.zeros(64, dtype=torch.int32, device=dev), torch.zeros(64, dtype=torch.int32, device=dev)
    ipn = torch.zeros(1, dtype=torch.int16, device=dev)
    sq_seq, sq_ip = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int16, device=dev)
    deliv = torch.ones(n, dtype=torch.uint8, device=dev)
    ops["tcp_send_seq"] = lambda: cx.tcp_send_seq_batch(conn64, w.status, cseq, ipn, sq_seq, sq_ip, stream=s)
    ops["tcp_send_seq_groupby"] = lambda: (cx.set_send_seq_groupby(1), cx.tcp_send_seq_batch(
        conn64, w.status, cseq, ipn, sq_seq, sq_ip, stream=s), cx.set_send_seq_groupby(0))
    ops["tcp_send_seq_scan1"] = lambda: (cx.set_send_seq_groupby(2), cx.tcp_send_seq_batch(
        conn64, w.status, cseq, ipn, sq_seq, sq_ip, stream=s), cx.set_send_seq_groupby(0))
    conn2k = (torch.arange(n, device=dev, dtype=torch.int64) * 7919 % 2047).to(torch.int32)
    cseq2k = torch.zeros(2047, dtype=torch.int32, device=dev)
    ops["tcp_send_seq_2047conn"] = lambda: cx.tcp_send_seq_batch(conn2k, w.status, cseq2k, ipn, sq_seq, sq_ip,
                                                                 stream=s)
    ops["tcp_recv_ack"] = lambda: cx.tcp_recv_ack_batch(conn64, deliv, sq_seq, cack, stream=s)
    # receive demux on the decoded fields (frames of this config; C4 marks 1/16 corrupted, 5% control)
    w.corrupt_frames()
    dmx = rc.DemuxBuffers.alloc(n, dev)
    dfields = rc._abi.DEMUX_ID | rc._abi.DEMUX_CONN_KEY | rc._abi.DEMUX_CMD_BARRIER
    # each demux shape on a context of its own: a context sizes its key table from its previous call
    # (steady traffic); one context alternating between shapes is tests/test_gpu_demux.py's business
    cx_dm = {k: rc.Codec(b"hello135", 0) for k in ("demux", "demux_64conn", "demux_server", "demux_server_group")}
    ops["demux"] = lambda: cx_dm["demux"].demux_batch(w.dec.status, w.dec.cmd, dfields, dmx, id=w.dec.id,
                                                      conv=w.dec.conv, conn_key=w.dec.conn_key, stream=s)
    # capture filter (server form) over the Ethernet wire packets: a 4M-packet capture batch
    fmatch = torch.empty(n, dtype=torch.uint8, device=dev)
    fidx = torch.empty(n, dtype=torch.int32, device=dev)
    fnm = torch.empty(1, dtype=torch.int32, device=dev)
    filt = rc.make_filter(dst_singles=[10001, 10002], dst_ranges=[(20000, 30000)], is_server=True)
    ops["capture_filter"] = lambda: cx.capture_filter_batch(wiree, offe, ste, 1, filt, fmatch, fidx, fnm, stream=s)
    tcp2, pdec2 = rc.TcpInfoBuffers.alloc(n, dev), rc.DecodeBuffers.alloc(n, dev)
    ops["filter_parse_decode"] = lambda: cx.filter_rawinput_batch(wiree, offe, ste, ste, 1, 0, filt, fmatch, tcp2,
                                                                  pdec2, stream=s)
    # header-only kernels: contiguous 32-B slots (no dependent offset load, no scattered headers)
    slots = w.frame[w.frame_off.view(-1, 1) + torch.arange(32, device=dev).view(1, -1)].reshape(-1).contiguous()
    hdec = rc.DecodeBuffers.alloc(n, dev)
    b0 = w.payload[w.pay_off].contiguous()
    hslot = torch.empty(32 * n, dtype=torch.uint8, device=dev)
    hst = torch.empty(n, dtype=torch.int32, device=dev)
    ops["decode_hdr"] = lambda: cx.onrecv_headers_batch(slots, w.frame_len, hdec, stream=s)
    ops["encode_hdr"] = lambda: cx.output_headers_batch(b0, w.pay_len, w.cmd, w.conv, w.conn_key, hslot, hst,
                                                        id_uniform=workload.ID_UNIFORM, stream=s)
    # realistic connection counts: 64 conns, 0.1% control packets, every packet VALID
    gk = torch.Generator(device=dev)
    gk.manual_seed(7)
    k_st = torch.ones(n, dtype=torch.int8, device=dev)
    k_cmd = (torch.rand(n, device=dev, generator=gk) < 0.001).to(torch.uint8) * 3
    k_key = torch.randint(0, 64, (n,), device=dev, generator=gk, dtype=torch.int64) * 0x10001 + 0x10000000
    k_id = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    dmx64 = rc.DemuxBuffers.alloc(n, dev)
    ops["demux_64conn"] = lambda: cx_dm["demux_64conn"].demux_batch(k_st, k_cmd, dfields, dmx64, id=k_id,
                                                                    conn_key=k_key, stream=s)
    # the server's leaf key (tests/demux_ref.py): 64 clients (IdBuf, dst) x 64 convs,
    # 0.1 % control packets, every packet VALID -- 4096 SConns
    A = rc._abi
    sfields = A.DEMUX_ID | A.DEMUX_DST | A.DEMUX_CONV | A.DEMUX_CMD_BARRIER
    grp = torch.randint(0, 64, (n,), device=dev, generator=gk, dtype=torch.int64)
    s_id = torch.randint(0, 256, (64, 8), device=dev, generator=gk, dtype=torch.int64).to(torch.uint8)[grp].reshape(-1)
    s_dst = (0x0a000000 + grp).to(torch.int32)
    s_conv = torch.randint(1, 65, (n,), device=dev, generator=gk, dtype=torch.int64).to(torch.int32)
    dmxs = rc.DemuxBuffers.alloc(n, dev)
    ops["demux_server"] = lambda: cx_dm["demux_server"].demux_batch(k_st, k_cmd, sfields, dmxs, id=s_id,
                                                                    conv=s_conv, dst=s_dst, stream=s)
    # the same batch with the IdBuf-scoped barrier (RSK_DEMUX_GROUP_BARRIER: ServerGroup routes a
    # control packet to its own IdBuf's SubGroup only): two group-by passes, ~1 segment per SConn
    gfields = A.DEMUX_ID | A.DEMUX_DST | A.DEMUX_CONV | A.DEMUX_GROUP_BARRIER
    dmxg = rc.DemuxBuffers.alloc(n, dev)
    ops["demux_server_group"] = lambda: cx_dm["demux_server_group"].demux_batch(k_st, k_cmd, gfields, dmxg, id=s_id,
                                                                                conv=s_conv, dst=s_dst, stream=s)
    for k, f in ops.items():
        if k == "demux":
            cx.onrecv_batch(w.frame, w.frame_off, w.frame_len, w.dec, stream=s)
        f()
    torch.cuda.synchronize()
    assert bool((pdec.status == 1).all()) and int(pdec.n_valid.item()) == n
    ops.pop("decode")  # decode now sees the corrupted frames; time it on them too
    ops["decode"] = lambda: cx.onrecv_batch(w.frame, w.frame_off, w.frame_len, w.dec, stream=s)
    # syncInput hand-off records: 21-B TcpInfo (from the parse above) + the frame, one per slot
    fp = d.frame_pitch
    rp = (21 + fp + 15) // 16 * 16
    hand = torch.zeros(n * rp, dtype=torch.uint8, device=dev)
    h2 = hand.view(n, rp)
    h2[:, 21:21 + fp] = w.frame[: n * fp].view(n, fp)
    hrec = torch.empty(n * 21, dtype=torch.uint8, device=dev)
    cx.tcpinfo_encode_batch(tcp.src, tcp.dst, tcp.sp, tcp.dp, tcp.seq, tcp.ack, tcp.flag, hrec, stream=s)
    h2[:, :21] = hrec.view(n, 21)
    hoff = torch.arange(n, device=dev, dtype=torch.int64) * rp
    hlen = w.frame_len.to(torch.int32) + 21
    tcp3, sdec = rc.TcpInfoBuffers.alloc(n, dev), rc.DecodeBuffers.alloc(n, dev)
    ops["syncinput_decode"] = lambda: cx.syncinput_batch(hand, hoff, hlen, tcp3, sdec, stream=s)
    # payload delivery (rsk_deliver_batch) of the decoded batch: the VALID payloads packed in valid_idx
    # order, in the segment order of the ALL | CMD_BARRIER demux, and the offsets alone
    # (decoded into buffers of its own with the config's corrupted frames -- C4: 1 in 16 dropped -- and
    # the frames restored, so the rows do not depend on which of the ops above ran last)
    ddec = rc.DecodeBuffers.alloc(n, dev)
    w.corrupt_frames()
    cx.onrecv_batch(w.frame, w.frame_off, w.frame_len, ddec, stream=s)
    w.corrupt_frames()
    dmxa = rc.DemuxBuffers.alloc(n, dev)
    afields = A.DEMUX_ID | A.DEMUX_CONN_KEY | A.DEMUX_CONV | A.DEMUX_DST | A.DEMUX_CMD_BARRIER
    zdst = torch.zeros(n, dtype=torch.int32, device=dev)
    cx_all = rc.Codec(b"hello135", 0)
    cx_all.demux_batch(ddec.status, ddec.cmd, afields, dmxa, id=ddec.id, conv=ddec.conv, conn_key=ddec.conn_key,
                       dst=zdst, stream=s)
    plan = rc.DeliverBuffers.alloc(n, dev)
    dl_in = (w.frame, w.frame_off, ddec.pay_off, ddec.pay_len, ddec.status)
    cx.deliver_batch(*dl_in, plan, order=ddec.valid_idx, n_order=ddec.n_valid, stream=s)
    torch.cuda.synchronize()
    dl_bytes = int(plan.total.item())
    dlv = rc.DeliverBuffers.alloc(n, dev, max(dl_bytes, 16))
    ops["deliver"] = lambda: cx.deliver_batch(*dl_in, dlv, order=ddec.valid_idx, n_order=ddec.n_valid, stream=s)
    ops["deliver_demux"] = lambda: cx.deliver_batch(*dl_in, dlv, order=dmxa.perm, n_order=dmxa.n_valid, stream=s)
    ops["deliver_plan"] = lambda: cx.deliver_batch(*dl_in, plan, order=ddec.valid_idx, n_order=ddec.n_valid,
                                                   stream=s)
    # the same delivery with every payload on a 16-B boundary: whole-chunk stores only (what the byte
    # borders of align = 1 cost is deliver's time over this row's)
    cx.deliver_batch(*dl_in, plan, order=ddec.valid_idx, n_order=ddec.n_valid, align=16, stream=s)
    torch.cuda.synchronize()
    dl16_bytes = int(plan.total.item())
    dlv16 = rc.DeliverBuffers.alloc(n, dev, max(dl16_bytes, 16))
    ops["deliver_align16"] = lambda: cx.deliver_batch(*dl_in, dlv16, order=ddec.valid_idx, n_order=ddec.n_valid,
                                                      align=16, stream=s)
    if args.copy_yardstick:
        # the dense 16-B copy of tools/hbm_probe.hip over the delivered byte count, in this process
        import ctypes

        hp = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhbm_probe.so"))
        hp.probe_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                 ctypes.c_void_p]
        ysrc = torch.randint(0, 255, (dl_bytes + 16,), dtype=torch.uint8, device=dev)
        for grid in (2048, 8192, 65536):
            ops[f"dense_copy@{grid}"] = lambda grid=grid: hp.probe_run(0, ysrc.data_ptr(), dlv.arena.data_ptr(),
                                                                       dl_bytes, grid, s.cuda_stream)
    # checksum verification (rsk_verify_wire_batch) of the wire packets built above: link header + IPv4
    # total length read per packet, one flag byte written
    vcs = torch.empty(n, dtype=torch.uint8, device=dev)
    vnb = torch.empty(1, dtype=torch.int32, device=dev)
    ops["verify_wire_eth"] = lambda: cx.verify_wire_batch(wiree, offe, ste, A.DLT_EN10MB, vcs, n_bad=vnb, stream=s)
    ops["verify_wire_raw4"] = lambda: cx.verify_wire_batch(wire4, off4, st4, A.DLT_RAW, vcs, n_bad=vnb, stream=s)
    vf_bytes = {"eth": int(ste.clamp(min=0).sum().item()), "raw4": int(st4.clamp(min=0).sum().item())}
    for k, (st_k, dl) in {"verify_wire_eth": (ste, A.DLT_EN10MB), "verify_wire_raw4": (st4, A.DLT_RAW)}.items():
        ops[k]()
        torch.cuda.synchronize()
        written = st_k > 0
        assert int(vnb.item()) == 0 and bool((vcs[written] == 0x0F).all()) and bool((vcs[~written] == 0).all()), k
    if args.read_yardstick:
        # the dense 16-B read of tools/hbm_probe.hip (k_read16) over the Ethernet rows' byte count, in
        # this process: the wire arena's own first bytes
        import ctypes

        hp = ctypes.CDLL(os.path.join(os.path.dirname(os.path.abspath(__file__)), "libhbm_probe.so"))
        hp.probe_run.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int,
                                 ctypes.c_void_p]
        ysink = torch.zeros(16, dtype=torch.int32, device=dev)
        assert vf_bytes["eth"] <= wiree.numel()
        for grid in (2048, 8192, 65536):
            ops[f"dense_read@{grid}"] = lambda grid=grid: hp.probe_run(1, wiree.data_ptr(), ysink.data_ptr(),
                                                                       vf_bytes["eth"], grid, s.cuda_stream)
    # connection table (rsk_conn_resolve_batch / rsk_conn_expand_batch): the decoded batch against a table
    # of its own connKeys, the 64-connection batch of demux_64conn, half of the keys absent, and the send
    # side's gather over 64 connections
    def conn_table(keys):
        t = rc.ConnTable.alloc(max(int(keys.numel()), 1), dev)
        t.conn_key[:keys.numel()] = keys
        t.state[:keys.numel()] = A.CONN_LIVE | A.CONN_ALIVE
        for col in (t.src, t.dst, t.sp, t.dp, t.seq, t.ack):
            col.copy_(torch.randint(0, 2**15, (t.capacity,), device=dev, generator=gk, dtype=torch.int64).to(col.dtype))
        t.flag.fill_(0x18)
        t.rebuild(cx, stream=s)
        return t

    own_keys = torch.unique(ddec.conn_key[ddec.status == 1])
    tab_own, tab_half, tab_64 = conn_table(own_keys), conn_table(own_keys[::2]), conn_table(torch.unique(k_key))
    r_conn, r_hit = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev)
    r_nm = torch.empty(1, dtype=torch.int32, device=dev)
    ops["conn_resolve"] = lambda: cx.conn_resolve_batch(tab_own, ddec.status, ddec.conn_key, r_conn, cmd=ddec.cmd,
                                                        hit=r_hit, stream=s)
    ops["conn_resolve_64conn"] = lambda: cx.conn_resolve_batch(tab_64, k_st, k_key, r_conn, cmd=k_cmd, hit=r_hit,
                                                               stream=s)
    ops["conn_resolve_miss"] = lambda: cx.conn_resolve_batch(tab_half, ddec.status, ddec.conn_key, r_conn,
                                                             cmd=ddec.cmd, hit=r_hit, n_miss=r_nm, stream=s)
    x_cols = {"src": torch.int32, "dst": torch.int32, "sp": torch.int16, "dp": torch.int16, "ack": torch.int32,
              "flag": torch.uint8, "conn_key": torch.int64}
    x_out = {k: torch.empty(n, dtype=dt, device=dev) for k, dt in x_cols.items()}
    x_ok = torch.empty(n, dtype=torch.uint8, device=dev)
    ops["conn_expand"] = lambda: cx.conn_expand_batch(tab_64, conn64, x_ok, stream=s, **x_out)
    looked = int(((ddec.status == 1) & (ddec.cmd == 0)).sum().item())
    for k in ("conn_resolve", "conn_resolve_64conn", "conn_resolve_miss", "conn_expand"):
        ops[k]()
    torch.cuda.synchronize()
    assert int(r_nm.item()) > 0 and bool((x_ok == 1).all())
    ops["conn_resolve"]()
    torch.cuda.synchronize()
    assert int(r_hit.sum().item()) == looked
    conn_tables = {"conn_resolve": tab_own.capacity, "conn_resolve_miss": tab_half.capacity,
                   "conn_resolve_64conn": tab_64.capacity, "conn_expand": tab_64.capacity,
                   "conn_resolve_miss_packets": int(r_nm.item())}
    # status, cmd, connKey read; conn, hit written.  conn read; the seven columns and ok written
    conn_alg = {"conn_resolve": 1 + 1 + 8 + 4 + 1, "conn_expand": 4 + 4 + 4 + 2 + 2 + 4 + 1 + 8 + 1}
    if args.read_yardstick:
        # the dense 16-B read of the same byte counts (the wire arena's first bytes)
        for name, per in (("resolve", conn_alg["conn_resolve"]), ("expand", conn_alg["conn_expand"])):
            assert n * per <= wiree.numel()
            for grid in (2048, 8192, 65536):
                ops[f"dense_read_{name}@{grid}"] = lambda grid=grid, per=per: hp.probe_run(
                    1, wiree.data_ptr(), ysink.data_ptr(), n * per, grid, s.cuda_stream)
    # the send pick (rsk_conn_pick_batch / rsk_conn_pick_build): a client's one group of 10 conns (rsock's
    # default port count) with the candidates read from global memory and staged in LDS, a server's 64 groups
    # of 10, the batch's own conns as one group and as groups of 10, the 64 x 10 table with an avoid key on
    # every packet, and the build over 2^20 rows.  Draws from the seed (no column).  Yardsticks of the same
    # run: conn_resolve and conn_expand above; the host twin with 16 threads on the same batch.
    import ctypes
    import time

    def pick_table(m, groups, keys=None):
        """A table of m candidates spread over `groups` IdBufs (0: a client table); every row LIVE | ALIVE."""
        t = rc.ConnTable.alloc(m, dev, by_id=groups > 0)
        t.conn_key.copy_(keys if keys is not None else torch.arange(1, m + 1, device=dev, dtype=torch.int64) * 0x9E3779B1)
        t.state.fill_(A.CONN_LIVE | A.CONN_ALIVE)
        if groups:
            gid = (torch.arange(m, device=dev, dtype=torch.int64) % groups + 1) * 0x100000001B3
            t.id.copy_(gid.view(torch.uint8))
        t.flag.fill_(0x18)
        t.rebuild(cx, stream=s)
        t.rebuild_pick(cx, stream=s)
        return t

    def group_ids(groups):
        g = torch.randint(0, groups, (n,), device=dev, generator=gk, dtype=torch.int64)
        return g, ((g + 1) * 0x100000001B3).view(torch.uint8)

    n_own = int(own_keys.numel())
    g_own = max(n_own // 10, 1)
    pk_client, pk_server = pick_table(10, 0), pick_table(640, 64)
    pk_own1, pk_owng = pick_table(n_own, 0, own_keys), pick_table(n_own, g_own, own_keys)
    g64, id64 = group_ids(64)
    _gown, idown = group_ids(g_own)
    # the avoid key of packet i: a conn of its own group (rows g, g + 64, ... hold group g)
    av64 = pk_server.conn_key[g64 + 64 * torch.randint(0, 10, (n,), device=dev, generator=gk, dtype=torch.int64)]
    p_conn, p_nn = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    set_path = rc.lib().rsk__set_pick_path
    set_path.argtypes, set_path.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int

    def pick_op(tab, path=1, **kw):
        def f():
            set_path(cx._ctx, path)
            cx.conn_pick_batch(tab, p_conn, seed=7, n_none=p_nn, stream=s, **kw)
        return f

    ops["conn_pick_client"] = pick_op(pk_client)
    ops["conn_pick_client_lds"] = pick_op(pk_client, path=2)
    ops["conn_pick_server"] = pick_op(pk_server, id=id64)
    ops["conn_pick_own_one"] = pick_op(pk_own1)
    ops["conn_pick_own_one_lds"] = pick_op(pk_own1, path=2)  # past the LDS limit: the plain loads plus the test
    ops["conn_pick_own_groups"] = pick_op(pk_owng, id=idown)
    ops["conn_pick_avoid"] = pick_op(pk_server, id=id64, avoid_key=av64)
    pk_1m, pk_1mg = pick_table(1 << 20, 0), pick_table(1 << 20, (1 << 20) // 10)
    ops["conn_pick_build_1m"] = lambda: cx.conn_pick_build(pk_1m, stream=s)
    ops["conn_pick_build_1m_by_id"] = lambda: cx.conn_pick_build(pk_1mg, stream=s)
    pick_check = {}
    for k in [k for k in ops if k.startswith("conn_pick_") and "build" not in k]:
        ops[k]()
        torch.cuda.synchronize()
        assert int(p_nn.item()) == 0, k
        pick_check[k] = int(torch.unique(p_conn).numel())
    assert pick_check["conn_pick_client"] == pick_check["conn_pick_client_lds"] == 10 and pick_check["conn_pick_server"] == 640
    ops["conn_pick_avoid"]()
    torch.cuda.synchronize()
    assert not bool((pk_server.conn_key[p_conn.to(torch.int64)] == av64).any())
    pick_host = {}
    for name, tab, idc in (("conn_pick_client", pk_client, None), ("conn_pick_server", pk_server, id64)):
        ht, hid = tab.to("cpu"), None if idc is None else idc.cpu().numpy()
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            rc.conn_pick_host(ht, n, id=hid, seed=7, nthreads=16)
            ts.append((time.perf_counter() - t0) * 1e3)
        pick_host[name] = round(float(np.median(ts)), 3)
    # control packets and the keepalive timer (rsk_control_batch / rsk_keepalive_flush): the decoded batch
    # with its own cmd column against the table of its connKeys (control_<config>: C4 has 5 % control
    # packets, C3 none -- the cost of finding nothing), the same batch with 20 % control packets
    # (control_dense), and the timer over 28 K and 2^20 rows.  The bodies are written into a copy of the
    # frames (~80 % keys of the table), so the frames the other rows decode stay as they are; a config whose
    # frames exceed 2 GiB is not copied and gets no control_dense row (its own batch has no body to write).
    ctl_rows = {}
    c_own = ((ddec.status == 1) & (ddec.cmd >= 1) & (ddec.cmd <= 4)).nonzero().flatten()
    dense_cmd = torch.where(torch.rand(n, device=dev, generator=gk) < 0.2,
                            torch.randint(1, 5, (n,), device=dev, generator=gk, dtype=torch.int64).to(torch.uint8), ddec.cmd)
    dense_cmd = torch.where(ddec.status == 1, dense_cmd, ddec.cmd)
    c_dense = ((ddec.status == 1) & (dense_cmd >= 1) & (dense_cmd <= 4)).nonzero().flatten()
    want_dense = w.frame.numel() <= (1 << 31)
    cframe = w.frame.clone() if (want_dense or c_own.numel()) and w.frame.numel() <= (1 << 31) else w.frame
    c_len = ddec.pay_len.clone()
    if cframe is not w.frame:
        idx = c_dense if want_dense else c_own
        k_body = own_keys[torch.randint(0, own_keys.numel(), (idx.numel(),), device=dev, generator=gk)]
        k_body = torch.where(torch.rand(idx.numel(), device=dev, generator=gk) < 0.8, k_body, k_body ^ (1 << 40))
        at = w.frame_off[idx] + ddec.pay_off[idx].to(torch.int64)
        cframe[(at[:, None] + torch.arange(8, device=dev)[None, :]).flatten()] = k_body.view(torch.uint8)
        c_len[idx] = torch.clamp(c_len[idx], min=8)
    ctl_full = rc.ControlBuffers.alloc(n, dev, capacity=tab_own.capacity)
    ctl_kind = rc.ControlBuffers.alloc(n, dev, capacity=tab_own.capacity)
    ctl_kind.arg = ctl_kind.conn = None
    ctl_tries = torch.zeros(tab_own.capacity, dtype=torch.uint8, device=dev)

    def control_op(cmd_col, out):
        return lambda: cx.control_batch(tab_own, ddec.status, cmd_col, ddec.pay_off, c_len, cframe, w.frame_off, out,
                                        id=ddec.id, ka_tries=ctl_tries, stream=s)

    ops[f"control_{args.config}"] = control_op(ddec.cmd, ctl_full)
    ops[f"control_{args.config}_kind"] = control_op(ddec.cmd, ctl_kind)
    if want_dense:
        ops["control_dense"] = control_op(dense_cmd, ctl_full)
        ops["control_dense_kind"] = control_op(dense_cmd, ctl_kind)
    for k in [k for k in ops if k.startswith("control_")]:
        ops[k]()
        torch.cuda.synchronize()
        kinds = torch.bincount(ctl_full.kind.to(torch.int64), minlength=8).tolist() if not k.endswith("_kind") else None
        ctl_rows[k] = {"n_ctl": int(ctl_full.n_ctl.item() if kinds else ctl_kind.n_ctl.item()),
                       "n_msg": int(ctl_full.n_msg.item() if kinds else ctl_kind.n_msg.item())}
        if kinds:
            look = (ctl_full.kind >= 2) & (ctl_full.kind <= 4)
            ctl_rows[k].update(kinds=kinds, lookups=int(look.sum().item()),
                               hits=int((look & (ctl_full.conn != -1)).sum().item()))
    own_ctl = ctl_rows[f"control_{args.config}"]
    assert own_ctl["n_ctl"] == int(((ddec.status == 1) & (ddec.cmd != 0)).sum().item())
    # the timer: every row LIVE and old enough, a third of them with a pending request
    ka = {}
    for label, cap in (("28k", 28232), ("1m", 1 << 20)):
        t = rc.ConnTable.alloc(cap, dev)
        t.state.fill_(A.CONN_LIVE | A.CONN_ALIVE)
        t.conn_key.copy_(torch.arange(cap, device=dev, dtype=torch.int64) + (1 << 28))
        tries0 = torch.where(torch.arange(cap, device=dev) % 3 == 0, 1, 255).to(torch.uint8)
        tries, est = tries0.clone(), torch.zeros(cap, dtype=torch.int64, device=dev)
        fo = rc.ControlBuffers.alloc(0, dev, capacity=cap, m=cap)
        ka[label] = (t, tries, tries0, est, fo)
        # every call starts from the same tries (the 1-B column copied back on the stream is part of the row)
        ops[f"keepalive_flush_{label}"] = lambda a=ka[label]: (a[1].copy_(a[2]), cx.keepalive_flush(
            a[0], a[1], a[3], 10**9, a[4], stream=s))
        ops[f"keepalive_flush_{label}"]()
        torch.cuda.synchronize()
        assert int(fo.n_msg.item()) == cap and int(fo.n_dead.item()) == 0
        ctl_rows[f"keepalive_flush_{label}"] = {"rows": cap, "n_msg": cap, "n_dead": 0}
    # algorithmic bytes per packet: status and cmd read, the per-packet outputs written, and per control
    # packet pay_len 2 + base_off 8 + pay_off 2 + id 8 + body 8 read; per message 37 written
    def ctl_alg(k):
        r = ctl_rows[k]
        per_out = 1 if k.endswith("_kind") else 1 + 8 + 4
        return 2 + per_out + ((r["n_ctl"] * 28 + r["n_msg"] * 37) / n)

    ka_alg = 1 + 1 + 8 + 1 + 8 + 37  # state, tries, est read; tries written; conn_key read; the message written
    if args.read_yardstick:
        for k in [k for k in ops if k.startswith("control_")]:
            for grid in (2048, 8192):
                ops[f"dense_read_{k}@{grid}"] = lambda grid=grid, b=int(n * ctl_alg(k)): hp.probe_run(
                    1, wiree.data_ptr(), ysink.data_ptr(), b, grid, s.cuda_stream)
        for label, cap in (("28k", 28232), ("1m", 1 << 20)):
            for grid in (256, 2048):
                ops[f"dense_read_keepalive_flush_{label}@{grid}"] = lambda grid=grid, b=cap * ka_alg: hp.probe_run(
                    1, wiree.data_ptr(), ysink.data_ptr(), b, grid, s.cuda_stream)
    # conv table (rsk_conv_resolve_batch / rsk_conv_flush): the decoded batch with three conv columns -- one
    # conv per connection of the batch (conv_per_conn: its own traffic shape, a row per distinct connKey), one
    # conv for every packet (conv_one), another conv for every packet of a 2^20 window (conv_each, capacity
    # 2^20, every row LIVE) -- each with and without the cur_in counts (_nocount), and the flush over 2^20
    # rows.  Yardsticks of the same run: conn_resolve on the same batch, keepalive_flush_1m on as many rows.
    import dataclasses

    def conv_table(convs):
        t = rc.ConvTable.alloc(int(convs.numel()), dev)
        t.conv.copy_(convs)
        t.state.fill_(A.CONN_LIVE)
        t.alive.fill_(1)
        t.rebuild(cx, stream=s)
        return t

    v_row = torch.empty(n, dtype=torch.int32, device=dev)
    ctab_conn = conv_table(torch.arange(own_keys.numel(), device=dev, dtype=torch.int32) * 7 + 3)
    ctab_each = conv_table(torch.arange(1 << 20, device=dev, dtype=torch.int32) * 5 + 1)
    col_conn = (torch.searchsorted(own_keys, ddec.conn_key).clamp(max=own_keys.numel() - 1) * 7 + 3).to(torch.int32)
    # bursts: runs of 37 neighbours carry the conv of the run's first packet (the config itself draws a
    # connection per packet, so its neighbours share nothing)
    col_burst = col_conn[(torch.arange(n, device=dev, dtype=torch.int64) // 37) * 37]
    conv_cols = {"conv_per_conn": (ctab_conn, col_conn),
                 "conv_bursts": (ctab_conn, col_burst),
                 "conv_one": (ctab_conn, torch.full((n,), 3, dtype=torch.int32, device=dev)),
                 "conv_each": (ctab_each, ((torch.arange(n, device=dev, dtype=torch.int64) % (1 << 20)) * 5 + 1).to(torch.int32))}
    for k, (t, col) in conv_cols.items():
        ops[k] = lambda t=t, col=col: cx.conv_resolve_batch(t, ddec.status, col, v_row, cmd=ddec.cmd, stream=s)
        ops[k + "_nocount"] = lambda t=dataclasses.replace(t, cur_in=None), col=col: cx.conv_resolve_batch(
            t, ddec.status, col, v_row, cmd=ddec.cmd, stream=s)
        t.cur_in.zero_()
        ops[k]()
        torch.cuda.synchronize()
        # every VALID DATA packet found its row and was counted once
        assert int((v_row != -1).sum().item()) == looked and int(t.cur_in.to(torch.int64).sum().item()) == looked, k
    assert int(ctab_conn.cur_in[0].item()) == looked  # conv_one ran last on this table: all on one row
    fl_alive0 = (torch.arange(1 << 20, device=dev) % 5 != 0).to(torch.uint8)
    fl_dead, fl_nd, fl_na = (torch.empty(k, dtype=torch.int32, device=dev) for k in (1 << 20, 1, 1))
    ctab_each.cur_out.copy_(ctab_each.cur_in)
    ops["conv_flush_1m"] = lambda: (ctab_each.alive.copy_(fl_alive0), cx.conv_flush(
        ctab_each, dead_rows=fl_dead, n_dead=fl_nd, n_alive=fl_na, stream=s))
    ops["conv_flush_1m"]()
    torch.cuda.synchronize()
    conv_rows = {**{k: t.capacity for k, (t, _col) in conv_cols.items()},
                 "conv_flush_1m": {"rows": 1 << 20, "n_dead": int(fl_nd.item()), "n_alive": int(fl_na.item())}}
    assert conv_rows["conv_flush_1m"]["n_dead"] == int((fl_alive0 == 0).sum().item())
    # conv create (rsk_conv_create_batch) on the decoded batch with one conv per connection:
    #   conv_create_none   no packet unknown (the table holds every conv): what keeping the call in the chain
    #                      costs; beside it conv_resolve_unknown, the resolve alone that leaves unknown / n_unknown
    #   conv_create_born   an empty table: every conv of the batch is born in the call (u_max = n)
    #   conv_old_born      the device work the same outcome takes without the call: rsk_demux_batch on `unknown`,
    #                      rsk_conv_index_build, the second rsk_conv_resolve_batch on the unknown packets -- on a
    #                      table whose rows are already written (the device -> host copy of the keys and the row
    #                      writes between the demux and the build are left out)
    # The born rows start every call from the same columns: `prep` (outside the timed span) restores them.
    prep = {}
    cr_data = (ddec.status == 1) & (ddec.cmd == 0)
    cr_keys = int(torch.unique(col_conn[cr_data]).numel())  # the convs that DATA packets name
    cr_cap = min(1 << 20, 1 << (2 * cr_keys - 1).bit_length())
    cr_row0, cr_unk0 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    cr_row, cr_unk = torch.empty_like(cr_row0), torch.empty_like(cr_unk0)
    cr_cnt = torch.zeros(4, dtype=torch.int32, device=dev)  # n_unknown, n_new, n_full, the resolve's n_unknown
    cr_new, cr_first = torch.empty(cr_cap, dtype=torch.int32, device=dev), torch.empty(cr_cap, dtype=torch.int32, device=dev)
    cr_tab = rc.ConvTable.alloc(cr_cap, dev)
    cr_tab.rebuild(cx, stream=s)
    cr_work = cr_tab.create_work(n)
    cr_none_work = ctab_conn.create_work(n)
    cx.conv_resolve_batch(cr_tab, ddec.status, col_conn, cr_row0, cmd=ddec.cmd, unknown=cr_unk0, stream=s)
    cr_old = rc.ConvTable.alloc(cr_cap, dev)  # the old path's table: the rows as the host would have written them
    cr_old.conv[:cr_keys] = torch.unique(col_conn[cr_data])
    cr_old.state[:cr_keys] = A.CONN_LIVE
    cr_old.alive[:cr_keys] = 1
    cx_cr = rc.Codec(b"hello135", 0)  # the demux of the old path on a context of its own (its table hint)
    dmx_cr = rc.DemuxBuffers.alloc(n, dev)

    def create_op(tab, work):
        return lambda: cx.conv_create_batch(tab, col_conn, cr_row, cr_unk, n, work, n_unknown=cr_cnt[0:1], new_rows=cr_new,
                                            new_first=cr_first, n_new=cr_cnt[1:2], n_full=cr_cnt[2:3], stream=s)

    def cr_reset(tab):
        def f():
            tab.state.zero_()
            tab.rebuild(cx, stream=s)
            cr_row.copy_(cr_row0)
            cr_unk.copy_(cr_unk0)
        return f

    ops["conv_resolve_unknown"] = lambda: cx.conv_resolve_batch(ctab_conn, ddec.status, col_conn, cr_row, cmd=ddec.cmd,
                                                                unknown=cr_unk, n_unknown=cr_cnt[3:4], stream=s)
    ops["conv_create_none"] = create_op(ctab_conn, cr_none_work)
    ops["conv_create_born"] = create_op(cr_tab, cr_work)
    prep["conv_create_born"] = cr_reset(cr_tab)
    ops["conv_old_born"] = lambda: (
        cx_cr.demux_batch(cr_unk0, ddec.cmd, A.DEMUX_CONV, dmx_cr, conv=col_conn, stream=s),
        cx.conv_index_build(cr_old, stream=s),
        cx.conv_resolve_batch(cr_old, cr_unk0, col_conn, cr_row, unknown=cr_unk, n_unknown=cr_cnt[3:4], stream=s))
    ops["conv_resolve_unknown"]()
    ops["conv_create_none"]()
    torch.cuda.synchronize()
    assert cr_cnt.tolist() == [0, 0, 0, 0] and int((cr_row != -1).sum().item()) == looked
    prep["conv_create_born"]()
    ops["conv_create_born"]()
    torch.cuda.synchronize()
    assert cr_cnt[:3].tolist() == [0, cr_keys, 0] and int((cr_row != -1).sum().item()) == looked
    assert int(cr_tab.cur_in.to(torch.int64).sum().item()) == looked and int((cr_tab.state == 1).sum().item()) == cr_keys
    born_rows = cr_row.clone()
    ops["conv_old_born"]()
    torch.cuda.synchronize()
    assert int(cr_cnt[3].item()) == 0 and int(dmx_cr.n_seg.item()) == cr_keys
    # both ways name one row per conv: the packets of a row are the same packets
    assert int(torch.unique(torch.stack([born_rows[cr_data], cr_row[cr_data]]).to(torch.int64), dim=1).shape[1]) == cr_keys
    conv_rows["conv_create"] = {"convs": cr_keys, "capacity": cr_cap, "u_max": n, "unknown_packets": looked,
                                "work_bytes": int(cr_work.numel()) * 4}
    # conv close (rsk_conv_close_batch) on the decoded batch with one conv per connection, and behind the flush:
    #   conv_close_none       receive form, no reset hits: what keeping the call in the chain costs
    #   conv_close_rst        1 % of the batch's convs reset once (at their first packet), the tails reopened, HOLD;
    #                         state, index and the packet columns restored outside the timed span
    #   conv_close_timer_1m   behind conv_flush_1m's dead_rows: a fifth of 2^20 rows close (on a twin of the table's
    #                         state and index, so that the other rows of this run keep their table)
    #   conv_old_close(_1m)   the device share of the old path for the same outcome: rsk_conv_index_build over the
    #                         same capacity (2^20 rows for _1m); the host round trip and the state copy are left out
    cl_cap = ctab_conn.capacity
    cl_tab = dataclasses.replace(ctab_conn, state=ctab_conn.state.clone(), index=ctab_conn.index.clone())
    cl_state0, cl_index0 = cl_tab.state.clone(), cl_tab.index.clone()
    cl_row0, cl_unk0 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int8, device=dev)
    cx.conv_resolve_batch(cl_tab, ddec.status, col_conn, cl_row0, cmd=ddec.cmd, unknown=cl_unk0, stream=s)
    torch.cuda.synchronize()
    cl_row, cl_unk = cl_row0.clone(), cl_unk0.clone()
    cl_no_rst = torch.full((cl_cap,), -1, dtype=torch.int32, device=dev)
    cl_kind0 = torch.zeros(n, dtype=torch.uint8, device=dev)
    found = torch.nonzero(cl_row0 != -1).squeeze(1)
    first_pkt = torch.full((cl_cap,), n, dtype=torch.int64, device=dev).scatter_reduce(
        0, cl_row0[found].to(torch.int64), found, "amin")
    named = torch.nonzero(first_pkt < n).squeeze(1)
    cl_reset_rows = named[::100]
    cl_rst = cl_no_rst.clone()
    cl_rst[cl_reset_rows] = first_pkt[cl_reset_rows].to(torch.int32)
    cl_kind = cl_kind0.clone()
    cl_kind[first_pkt[cl_reset_rows]] = A.CTL_CONV_RST
    cl_cnt = torch.zeros(4, dtype=torch.int32, device=dev)  # n_unknown, n_closed, n_reopened, n_rst_again
    cl_rows, cl_at = torch.empty(cl_cap, dtype=torch.int32, device=dev), torch.empty(cl_cap, dtype=torch.int32, device=dev)

    def close_op(rst, kind):
        return lambda: cx.conv_close_batch(cl_tab, rst_first=rst, ctl_kind=kind, conv_row=cl_row, unknown=cl_unk,
                                           n_unknown=cl_cnt[0:1], hold=True, closed_rows=cl_rows, closed_at=cl_at,
                                           n_closed=cl_cnt[1:2], n_reopened=cl_cnt[2:3], n_rst_again=cl_cnt[3:4], stream=s)

    def cl_reset():
        cl_tab.index.copy_(cl_index0)
        cl_row.copy_(cl_row0)
        cl_unk.copy_(cl_unk0)
        cl_cnt.zero_()

    ops["conv_close_none"] = close_op(cl_no_rst, cl_kind0)
    ops["conv_close_rst"] = close_op(cl_rst, cl_kind)
    prep["conv_close_rst"] = cl_reset
    ops["conv_old_close"] = lambda: cx.conv_index_build(cl_tab, stream=s)
    cl_each = dataclasses.replace(ctab_each, state=ctab_each.state.clone(), index=ctab_each.index.clone())
    cl_each_state0, cl_each_index0 = cl_each.state.clone(), cl_each.index.clone()
    cl_each_work = cl_each.close_work()
    cl_each_rows, cl_each_n = torch.empty(1 << 20, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    ops["conv_close_timer_1m"] = lambda: cx.conv_close_batch(cl_each, close_rows=fl_dead, n_close=fl_nd, work=cl_each_work,
                                                             closed_rows=cl_each_rows, n_closed=cl_each_n, stream=s)
    prep["conv_close_timer_1m"] = lambda: (cl_each.state.copy_(cl_each_state0), cl_each.index.copy_(cl_each_index0))
    cl_old_1m = dataclasses.replace(ctab_each, index=ctab_each.index.clone())
    ops["conv_old_close_1m"] = lambda: cx.conv_index_build(cl_old_1m, stream=s)
    ops["conv_close_none"]()
    torch.cuda.synchronize()
    assert cl_cnt.tolist() == [0, 0, 0, 0] and torch.equal(cl_row, cl_row0) and torch.equal(cl_tab.index, cl_index0)
    cl_reset()
    ops["conv_close_rst"]()
    torch.cuda.synchronize()
    cl_tail = int(((cl_row0 != -1) & (cl_row == -1)).sum().item())
    assert cl_cnt.tolist() == [cl_tail, int(cl_reset_rows.numel()), cl_tail, 0] and cl_tail > 0
    assert torch.equal(cl_rows[:cl_reset_rows.numel()].to(torch.int64), cl_reset_rows) and torch.equal(cl_tab.state, cl_state0)
    cl_reset()
    ops["conv_close_timer_1m"]()
    torch.cuda.synchronize()
    assert int(cl_each_n.item()) == conv_rows["conv_flush_1m"]["n_dead"]
    assert torch.equal(cl_each_rows[:int(cl_each_n.item())], fl_dead[:int(cl_each_n.item())])
    assert int((cl_each.state == 1).sum().item()) == (1 << 20) - int(cl_each_n.item())
    prep["conv_close_timer_1m"]()
    conv_rows["conv_close"] = {"capacity": cl_cap, "convs_reset": int(cl_reset_rows.numel()), "packets_reopened": cl_tail,
                               "timer_rows": 1 << 20, "timer_closed": int(cl_each_n.item()),
                               "timer_work_bytes": int(cl_each_work.numel()) * 4}
    # conn close (rsk_conn_close_batch): conns killed and removed on the device table, the pick index kept current
    #   conn_close_none            column form on the table of the batch's own conns, nothing marked, with pick: what
    #                              keeping the call in the chain costs (5 launches)
    #   conn_close_rst             the same table, 1 % of the rows marked, REMOVE and pick
    #   conn_close_timer_1m(_by_id) 2^20 rows (one group / groups of 10), a fifth marked by a list, REMOVE and pick
    #   conn_old_*                 the device share of the old path for the same outcome on the same tables:
    #                              rsk_conn_index_build + rsk_conn_pick_build; the host's round trip and state edit
    #                              are left out, which favours the old path
    # state, index and pick are restored outside the timed span.
    def cc_twin(t):
        t = dataclasses.replace(t, state=t.state.clone(), index=t.index.clone(), pick=t.pick.clone())
        t.rebuild(cx, stream=s)
        t.rebuild_pick(cx, stream=s)
        torch.cuda.synchronize()
        return t, (t.state.clone(), t.index.clone(), t.pick.clone())

    def cc_restore(t, saved):
        return lambda: (t.state.copy_(saved[0]), t.index.copy_(saved[1]), t.pick.copy_(saved[2]))

    cc_out = {k: torch.empty(1 << 20, dtype=torch.int32, device=dev) for k in ("marked_rows", "closed_rows")}
    cc_cnt = torch.zeros(6, dtype=torch.int32, device=dev)  # n_marked, n_closed, pick_counts[2]
    cc_kw = dict(marked_rows=cc_out["marked_rows"], n_marked=cc_cnt[0:1], closed_rows=cc_out["closed_rows"],
                 n_closed=cc_cnt[1:2], pick=True, pick_counts=cc_cnt[2:4], stream=s)
    cc_own, cc_own0 = cc_twin(tab_own)
    cc_work = cc_own.close_work()
    cc_no_rst = torch.full((cc_own.capacity,), -1, dtype=torch.int32, device=dev)
    cc_rst = cc_no_rst.clone()
    cc_rst[::100] = 0
    ops["conn_close_none"] = lambda: cx.conn_close_batch(cc_own, cc_work, rst_first=cc_no_rst, **cc_kw)
    ops["conn_close_rst"] = lambda: cx.conn_close_batch(cc_own, cc_work, rst_first=cc_rst, remove=True, **cc_kw)
    prep["conn_close_rst"] = cc_restore(cc_own, cc_own0)
    ops["conn_old_none"] = ops["conn_old_rst"] = lambda: (cx.conn_index_build(cc_own, stream=s),
                                                          cx.conn_pick_build(cc_own, stream=s))
    cc_dead = torch.arange(0, 1 << 20, 5, device=dev, dtype=torch.int32)
    cc_nd = torch.tensor([cc_dead.numel()], dtype=torch.int32, device=dev)
    cc_rows = {"conn_close_none": {"rows": cc_own.capacity, "marked": 0},
               "conn_close_rst": {"rows": cc_own.capacity, "marked": int((cc_rst != -1).sum().item())}}
    for name, src_tab in (("timer_1m", pk_1m), ("timer_1m_by_id", pk_1mg)):
        t1, saved1 = cc_twin(src_tab)
        w1 = t1.close_work()
        ops["conn_close_" + name] = lambda t1=t1, w1=w1: cx.conn_close_batch(t1, w1, close_rows=cc_dead, n_close=cc_nd,
                                                                             remove=True, **cc_kw)
        prep["conn_close_" + name] = cc_restore(t1, saved1)
        ops["conn_old_" + name] = lambda t1=t1: (cx.conn_index_build(t1, stream=s), cx.conn_pick_build(t1, stream=s))
        ops["conn_close_" + name]()
        torch.cuda.synchronize()
        assert cc_cnt.tolist()[:4] == [cc_dead.numel(), cc_dead.numel(), (1 << 20) // 10 if name.endswith("by_id") else 1,
                                       (1 << 20) - cc_dead.numel()], (name, cc_cnt.tolist())
        assert int((t1.state == 3).sum().item()) == (1 << 20) - cc_dead.numel()
        prep["conn_close_" + name]()
        cc_rows["conn_close_" + name] = {"rows": 1 << 20, "marked": int(cc_dead.numel()), "work_bytes": int(w1.numel()) * 4}
    ops["conn_close_none"]()
    torch.cuda.synchronize()
    assert cc_cnt.tolist()[:2] == [0, 0] and torch.equal(cc_own.index, cc_own0[1]) and torch.equal(cc_own.pick, cc_own0[2])
    ops["conn_close_rst"]()
    torch.cuda.synchronize()
    assert cc_cnt.tolist()[:2] == [cc_rows["conn_close_rst"]["marked"]] * 2
    prep["conn_close_rst"]()
    # conn create (rsk_conn_create_batch): conns born on the device table, both indexes kept current.  The table is the
    # batch's own conns as one group (a client's flavour) and as groups of 10 (_by_id); a packet's 4-tuple and IdBuf
    # are its conn's, one offer per conn.
    #   conn_create_none(_by_id)   every conn LIVE, nothing missing: what keeping the call in the chain costs
    #   conn_create_all(_by_id)    the table empty, every conn of the batch born in one call
    #   conn_create_1pct(_by_id)   every 100th row vacant, its conn born again
    #   conn_create_list_1m(_by_id) list form on 2^20 rows (one group / groups of 10), a fifth of them vacant
    #   conn_old_create_*          the device share of the old path for the same outcome: the demux of miss,
    #                              rsk_conn_index_build, rsk_conn_pick_build and the second resolve on the filled table
    #                              (index and pick build alone for the list); the host round trip and its row writes
    #                              are left out, which favours the old path
    # state, both indexes and the packet columns are restored outside the timed span.
    cn_row = torch.searchsorted(own_keys, ddec.conn_key).clamp(max=n_own - 1)
    cn_tuple = lambda r: {"src": r.to(torch.int32), "dst": torch.full_like(r, 0x0A000001).to(torch.int32),  # noqa: E731
                          "sp": (r % 60000 + 1024).to(torch.int16), "dp": (r // 60000 + 443).to(torch.int16)}
    cn_pkt = cn_tuple(cn_row)
    cn_idcol = ((cn_row % g_own + 1) * 0x100000001B3).view(torch.uint8)

    def cn_offers(rows, tab=None):
        """One offer per row of `rows` (the conn's tuple); with `tab` also the list form's key columns."""
        o = cn_tuple(rows)
        o.update(ack=torch.randint(0, 2**31, (rows.numel(),), device=dev, generator=gk, dtype=torch.int64).to(torch.int32),
                 flag=torch.full((rows.numel(),), 0x18, dtype=torch.uint8, device=dev))
        if tab is not None:
            o["conn_key"] = tab.conn_key[rows].clone()
            o["id"] = tab.id.view(-1, 8)[rows].reshape(-1).clone() if tab.by_id else None
        return rc.ConnOffers(n_offer=torch.tensor([rows.numel()], dtype=torch.int32, device=dev), m_max=int(rows.numel()), **o)

    def cn_table(src_tab, vacant=None):
        """A copy of src_tab with the rows `vacant` (None: all) vacant, both indexes current, and what restores it."""
        t = src_tab.to(dev)
        if vacant is None:
            t.state.zero_()
        else:
            t.state[vacant] = 0
        t.rebuild(cx, stream=s)
        t.rebuild_pick(cx, stream=s)
        torch.cuda.synchronize()
        return t, (t.state.clone(), t.index.clone(), t.pick.clone())

    cn_cnt = torch.zeros(8, dtype=torch.int32, device=dev)  # n_miss, n_new, n_full, n_refused, pick_counts[2]
    cn_new = {k: torch.empty(1 << 20, dtype=torch.int32, device=dev) for k in ("new_rows", "new_first", "new_offer")}
    cn_cols = {k: (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.uint8, device=dev),
                   torch.empty(n, dtype=torch.int8, device=dev)) for k in ("none", "all", "1pct")}
    dmx_cn = rc.DemuxBuffers.alloc(n, dev)
    cn_rows, cn_saved = {}, {}
    for sfx, src_tab in (("", pk_own1), ("_by_id", pk_owng)):
        idc = cn_idcol if src_tab.by_id else None
        every = torch.arange(n_own, device=dev, dtype=torch.int64)
        for case, vacant, offer_rows in (("none", every[:0], every), ("all", None, every), ("1pct", every[::100], every[::100])):
            t, saved = cn_table(src_tab, vacant)
            conn, hit, miss = (c.clone() for c in cn_cols[case])
            cx.conn_resolve_batch(t, ddec.status, ddec.conn_key, conn, cmd=ddec.cmd, id=idc, hit=hit, miss=miss, stream=s)
            torch.cuda.synchronize()
            cols0 = (conn.clone(), hit.clone(), miss.clone())
            offers = cn_offers(offer_rows)
            work = t.create_work(n, offers.m_max)
            name = f"conn_create_{case}{sfx}"

            def op(t=t, offers=offers, work=work, conn=conn, hit=hit, miss=miss, idc=idc):
                cx.conn_create_batch(t, offers, work, stream=s, u_max=n, conn_key=ddec.conn_key, id=idc, conn=conn, hit=hit,
                                     miss=miss, n_miss=cn_cnt[0:1], n_new=cn_cnt[1:2], n_full=cn_cnt[2:3], n_refused=cn_cnt[3:4],
                                     pick=True, pick_counts=cn_cnt[4:6], **cn_pkt, **cn_new)

            def restore(t=t, saved=saved, cols=(conn, hit, miss), cols0=cols0):
                t.state.copy_(saved[0]), t.index.copy_(saved[1]), t.pick.copy_(saved[2])
                for c, c0 in zip(cols, cols0):
                    c.copy_(c0)

            ops[name] = op
            if case != "none":
                prep[name] = restore
                miss0 = cols0[2]
                full = cn_saved["full" + sfx]
                ops[f"conn_old_create_{case}{sfx}"] = lambda miss0=miss0, full=full, idc=idc: (
                    cx_cr.demux_batch(miss0, ddec.cmd, A.DEMUX_CONN_KEY | (A.DEMUX_ID if idc is not None else 0), dmx_cn,
                                      conn_key=ddec.conn_key, id=idc, stream=s),
                    cx.conn_index_build(full, stream=s), cx.conn_pick_build(full, stream=s),
                    cx.conn_resolve_batch(full, ddec.status, ddec.conn_key, r_conn, cmd=ddec.cmd, id=idc, hit=r_hit, stream=s))
            else:
                cn_saved["full" + sfx] = t
            op()
            torch.cuda.synchronize()
            # the conns born: the distinct keys of the missing packets (a conn whose packets are all control packets
            # is never missed: C4 has some)
            want_new = int(torch.unique(ddec.conn_key[cols0[2] == 1]).numel())
            live = n_own - (n_own if vacant is None else int(vacant.numel())) + want_new
            assert cn_cnt.tolist()[:4] == [0, want_new, 0, 0], (name, cn_cnt.tolist())
            assert int((conn != -1).sum().item()) == looked and int((t.state & 1).sum().item()) == live, name
            if case == "none":
                assert want_new == 0 and torch.equal(t.index, saved[1]) and torch.equal(t.pick, saved[2])
            else:
                assert want_new > 0 and cn_cnt[5].item() == live and (cn_cnt[4].item() == 1 or src_tab.by_id), (name, cn_cnt.tolist())
                restore()
            cn_rows[name] = {"rows": n_own, "born": want_new, "missing_packets": int((cols0[2] == 1).sum().item()),
                             "work_bytes": int(work.numel()) * 4}
    cn_fifth = torch.arange(0, 1 << 20, 5, device=dev, dtype=torch.int64)
    for sfx, src_tab in (("", pk_1m), ("_by_id", pk_1mg)):
        t, saved = cn_table(src_tab, cn_fifth)
        offers = cn_offers(cn_fifth, tab=t)
        work = t.create_work(0, offers.m_max)
        name = "conn_create_list_1m" + sfx
        ops[name] = lambda t=t, offers=offers, work=work: cx.conn_create_batch(
            t, offers, work, stream=s, list_form=True, n_new=cn_cnt[1:2], n_full=cn_cnt[2:3], n_refused=cn_cnt[3:4], pick=True,
            pick_counts=cn_cnt[4:6], new_rows=cn_new["new_rows"], new_offer=cn_new["new_offer"])
        prep[name] = cc_restore(t, saved)
        ops[name]()
        torch.cuda.synchronize()
        assert cn_cnt.tolist()[1:6] == [cn_fifth.numel(), 0, 0, (1 << 20) // 10 if src_tab.by_id else 1, 1 << 20], (name, cn_cnt.tolist())
        assert torch.equal(cn_new["new_rows"][:cn_fifth.numel()].to(torch.int64), cn_fifth)
        prep[name]()
        cn_rows[name] = {"rows": 1 << 20, "born": int(cn_fifth.numel()), "work_bytes": int(work.numel()) * 4}
    nseg =[int(dmx.n_seg.item()), int(dmx64.n_seg.item()), int(dmxs.n_seg.item()), int(dmxg.n_seg.item())]
    if args.only:
        keep = args.only.split(",")
        # an entry ending in * keeps every path it is a prefix of
        ops = {k: f for k, f in ops.items() if k in keep or any(e.endswith("*") and k.startswith(e[:-1]) for e in keep)}
    times = {k: [] for k in ops}
    for _ in range(args.rounds):
        for k, f in ops.items():
            if k in prep:  # a call that consumes its inputs: restore them before every call, outside the timed span
                evs = []
                for _ in range(args.reps):
                    prep[k]()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(s)
                    f()
                    e1.record(s)
                    evs.append((e0, e1))
                torch.cuda.synchronize()
                times[k].append(sum(a.elapsed_time(b) for a, b in evs) / args.reps)
                continue
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(args.reps):
                f()
            e1.record(s)
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.reps)
    p = float(d.pay_len.astype(np.float64).mean())
    alg = {  # algorithmic bytes per packet
        "encode": 2 * p + 66,
        "encode_wire_raw4": 2 * p + 66 + 40 + 23,
        "encode_wire_eth": 2 * p + 66 + 54 + 23,
        "encode_wire_raw4_pkt": 2 * p + 66 + 40 + 23,
        "encode_wire_raw4_flat": 2 * p + 66 + 40 + 23,
        "encode_wire_raw4_hyb1": 2 * p + 66 + 40 + 23,
        "decode": 73,
        "parse_decode": 54 + 32 + 16 + 21 + 4 + 73 - 42,
        "demux": 1 + 1 + 8 + 8 + 4,  # status, cmd, id, conn_key in; perm out (+ per-segment words)
        "demux_64conn": 1 + 1 + 8 + 8 + 4,
        "demux_server": 1 + 1 + 8 + 4 + 4 + 4,  # status, cmd, id, conv, dst in; perm out
        "demux_server_group": 1 + 1 + 8 + 4 + 4 + 4,
        "capture_filter": 8 + 4 + 64 + 16 + 1 + 4,  # cap_off, cap_len, header windows, match, match_idx
        "filter_parse_decode": 8 + 4 + 64 + 16 + 1 + 54 + 32 + 16 + 21 + 4 + 73 - 42,
        "decode_hdr": 32 + 2 + 27 + 4,
        "encode_hdr": 1 + 2 + 1 + 4 + 8 + 32 + 4,
        "tcp_send_seq": 4 + 4 + 4 + 2,  # conn, status in; seq, ip_id out
        "tcp_send_seq_groupby": 4 + 4 + 4 + 2,
        "tcp_send_seq_scan1": 4 + 4 + 4 + 2,
        "tcp_send_seq_2047conn": 4 + 4 + 4 + 2,
        "tcp_recv_ack": 4 + 1 + 4,      # conn, delivered, seq in
        # record bytes [0, 53) + rec_off + nread in; TcpInfo (26) + decode fields (27) + valid_idx out
        "syncinput_decode": 53 + 8 + 4 + 26 + 27 + 4,
        # payload bytes read + written, + 8 B per offset
        "deliver": 2 * dl_bytes / n + 8,
        "deliver_demux": 2 * dl_bytes / n + 8,
        "deliver_plan": 8,
        "deliver_align16": (dl_bytes + dl16_bytes) / n + 8,
    }
    alg.update({k: 2 * dl_bytes / n for k in ops if k.startswith("dense_copy@")})
    # verify: link header + IPv4 total length read, one flag byte written
    alg.update({"verify_wire_eth": vf_bytes["eth"] / n + 1, "verify_wire_raw4": vf_bytes["raw4"] / n + 1})
    alg.update({k: vf_bytes["eth"] / n for k in ops if k.startswith("dense_read@")})
    alg.update({k: conn_alg["conn_resolve"] for k in ("conn_resolve", "conn_resolve_64conn", "conn_resolve_miss")})
    alg["conn_expand"] = conn_alg["conn_expand"]
    alg.update({k: conn_alg["conn_resolve"] for k in ops if k.startswith("dense_read_resolve@")})
    alg.update({k: conn_alg["conn_expand"] for k in ops if k.startswith("dense_read_expand@")})
    items = {}  # rows that do not run over the batch's n packets: the timer's rows
    for k in ops:
        base = k[len("dense_read_"):].split("@")[0] if k.startswith("dense_read_") else k
        if base.startswith("control_"):
            alg[k] = ctl_alg(base)
        elif base.startswith("keepalive_flush_"):
            alg[k], items[k] = ka_alg, ctl_rows[base]["rows"]
    # conv: status, cmd, conv read, conv_row written; the flush reads state, alive and the four counters of a
    # row and writes alive and the two prev words
    alg.update({k: 1 + 1 + 4 + 4 for k in ops if k.startswith("conv_") and k != "conv_flush_1m"})
    # create: unknown read by the count, the list and the assign passes; with every packet unknown also conv read by
    # the dedup, the two first-arrival passes and the assign, the list written and read three times, conv_row and
    # unknown written.  The old path: the demux's status, conv, perm and the second resolve's bytes
    alg.update({"conv_resolve_unknown": 1 + 1 + 4 + 4 + 1, "conv_create_none": 3, "conv_create_born": 3 + 4 * 4 + 4 * 4 + 4 + 1,
                "conv_old_born": 1 + 4 + 4 + 1 + 4 + 4 + 1})
    if "conv_flush_1m" in ops:
        alg["conv_flush_1m"], items["conv_flush_1m"] = 1 + 1 + 16 + 1 + 8, 1 << 20
    # close, per row: state and the mark (rst_first or a byte) read by the count; with rows closing also read again
    # by the row pass, the index cleared and written (8 B per row and more: >= 2 entries per row) and the keys read;
    # the old path: the index cleared and written, state and the key read.  Per packet (conv_close_rst): conv_row
    # and the rst_first gather -- left out of the row figures
    for k, a_, rows_ in (("conv_close_none", 1 + 4, cl_cap), ("conv_close_rst", 2 * (1 + 4) + 8 + 4 + 4, cl_cap),
                         ("conv_old_close", 8 + 4 + 1 + 4, cl_cap), ("conv_close_timer_1m", 1 + 1 + 2 * (1 + 1) + 8 + 4 + 4, 1 << 20),
                         ("conv_old_close_1m", 8 + 4 + 1 + 4, 1 << 20)):
        if k in ops:
            alg[k], items[k] = a_, rows_
    # conn close / the old path, per row: state and the mark read (left as the figure for every row of the family)
    for k in ops:
        if k.startswith(("conn_close_", "conn_old_")):
            alg[k], items[k] = 1 + 4, (1 << 20) if "_1m" in k else cc_own.capacity
    # conn create, per packet: miss read by the count; with packets missing also the key and the tuple (left as the
    # figure for every row of the family); the list form per row of the table
    for k in ops:
        if k.startswith(("conn_create_", "conn_old_create_")):
            alg[k] = 1 + 8 + 4
            if "_1m" in k:
                items[k] = 1 << 20
            else:
                items.pop(k, None)
    # pick: id (BY_ID) and the avoid key read, conn written; the build reads state (and id) and writes cand, pos
    for k in ops:
        if k.startswith("conn_pick_build"):
            alg[k], items[k] = 1 + 8 + (8 + 20 if k.endswith("by_id") else 0), 1 << 20
        elif k.startswith("conn_pick_"):
            alg[k] = 4 + (8 if k in ("conn_pick_server", "conn_pick_own_groups", "conn_pick_avoid") else 0) + \
                (8 if k == "conn_pick_avoid" else 0)
    cx.onrecv_batch(w.frame, w.frame_off, w.frame_len, w.dec, stream=s)
    torch.cuda.synchronize()
    if "syncinput_decode" in ops:
        assert torch.equal(sdec.status, w.dec.status) and torch.equal(sdec.n_valid, w.dec.n_valid)
    out = {}
    for k, t in times.items():
        m = float(np.median(t))
        a = alg.get(k, alg["encode_wire_eth" if "_eth_" in k else "encode_wire_raw4"])
        cnt = items.get(k, n)
        out[k] = {"ms": round(m, 4), "Mpkt_s": round(cnt / m / 1e3, 1), "GBps_alg": round(cnt * a / m / 1e6, 1)}
    res = {"config": args.config, "packets": n, "wire_pitch": [p4, pe], "demux_segments": nseg,
           "deliver_bytes": dl_bytes, "paths": out}
    dense = [v["ms"] for k, v in out.items() if k.startswith("dense_copy@")]
    if dense and "deliver" in out:
        res["dense_copy_ms"] = min(dense)
        res["deliver_over_dense_copy"] = round(out["deliver"]["ms"] / min(dense), 3)
        if "deliver_demux" in out:
            res["deliver_demux_over_dense_copy"] = round(out["deliver_demux"]["ms"] / min(dense), 3)
    dread = [v["ms"] for k, v in out.items() if k.startswith("dense_read@")]
    if dread:
        res["verify_bytes"] = vf_bytes
        res["dense_read_ms"] = min(dread)
        for k in ("verify_wire_eth", "verify_wire_raw4"):
            if k in out:
                res[f"{k}_over_dense_read"] = round(out[k]["ms"] / min(dread), 3)
    if any(k.startswith("conn_") for k in out):
        res["conn_table_rows"] = conn_tables
    for name, rows in (("resolve", ("conn_resolve", "conn_resolve_64conn", "conn_resolve_miss")), ("expand", ("conn_expand",))):
        dr = [v["ms"] for k, v in out.items() if k.startswith(f"dense_read_{name}@")]
        if dr:
            res[f"dense_read_{name}_ms"] = min(dr)
            for k in rows:
                if k in out:
                    res[f"{k}_over_dense_read"] = round(out[k]["ms"] / min(dr), 3)
    ctl = [k for k in out if k.startswith(("control_", "keepalive_flush_"))]
    if ctl:
        res["control_rows"] = {k: dict(ctl_rows[k], bytes_alg=round(alg[k], 2)) for k in ctl}
    for k in ctl:
        dr = [v["ms"] for q, v in out.items() if q.startswith(f"dense_read_{k}@")]
        if dr:
            res[f"{k}_over_dense_read"] = round(out[k]["ms"] / min(dr), 3)
        if k.startswith("control_") and "conn_resolve" in out:
            res[f"{k}_over_conn_resolve"] = round(out[k]["ms"] / out["conn_resolve"]["ms"], 3)
    if any(k.startswith("conv_") for k in out):
        res["conv_table_rows"] = conv_rows
        for k in conv_cols:
            if k in out and k + "_nocount" in out:
                res[f"{k}_over_nocount"] = round(out[k]["ms"] / out[k + "_nocount"]["ms"], 3)
            for q in (k, k + "_nocount"):
                if q in out and "conn_resolve" in out:
                    res[f"{q}_over_conn_resolve"] = round(out[q]["ms"] / out["conn_resolve"]["ms"], 3)
        if "conv_one" in out and "conv_per_conn" in out:
            res["conv_one_over_conv_per_conn"] = round(out["conv_one"]["ms"] / out["conv_per_conn"]["ms"], 3)
        if "conv_create_none" in out and "conv_resolve_unknown" in out:
            res["conv_create_none_over_conv_resolve_unknown"] = round(out["conv_create_none"]["ms"] / out["conv_resolve_unknown"]["ms"], 3)
        if "conv_create_born" in out and "conv_old_born" in out:
            res["conv_create_born_over_conv_old_born"] = round(out["conv_create_born"]["ms"] / out["conv_old_born"]["ms"], 3)
        for k, y in (("conv_close_none", "conv_old_close"), ("conv_close_none", "conv_create_none"),
                     ("conv_close_rst", "conv_old_close"), ("conv_close_timer_1m", "conv_old_close_1m")):
            if k in out and y in out:
                res[f"{k}_over_{y}"] = round(out[k]["ms"] / out[y]["ms"], 3)
        if all(k in out for k in ("conv_close_timer_1m", "conv_flush_1m", "conv_old_close_1m")):
            res["conv_flush_close_timer_1m_over_flush_old_close_1m"] = round(
                (out["conv_flush_1m"]["ms"] + out["conv_close_timer_1m"]["ms"])
                / (out["conv_flush_1m"]["ms"] + out["conv_old_close_1m"]["ms"]), 3)
        if "conv_flush_1m" in out and "keepalive_flush_1m" in out:
            res["conv_flush_1m_over_keepalive_flush_1m"] = round(out["conv_flush_1m"]["ms"] / out["keepalive_flush_1m"]["ms"], 3)
    if any(k.startswith("conn_close_") for k in out):
        res["conn_close_rows"] = {k: v for k, v in cc_rows.items() if k in out}
        for k in [k for k in out if k.startswith("conn_close_")]:
            y = "conn_old_" + k[len("conn_close_"):]
            if y in out:
                res[f"{k}_over_{y}"] = round(out[k]["ms"] / out[y]["ms"], 3)
        if "conn_close_none" in out and "conv_close_none" in out:
            res["conn_close_none_over_conv_close_none"] = round(out["conn_close_none"]["ms"] / out["conv_close_none"]["ms"], 3)
    if any(k.startswith("conn_create_") for k in out):
        res["conn_create_rows"] = {k: v for k, v in cn_rows.items() if k in out}
        for k in [k for k in out if k.startswith("conn_create_")]:
            tail = k[len("conn_create_"):]
            y = "conn_old_timer_1m" + tail[len("list_1m"):] if tail.startswith("list_1m") else "conn_old_create_" + tail
            if y in out:
                res[f"{k}_over_{y}"] = round(out[k]["ms"] / out[y]["ms"], 3)
        for y in ("conn_close_none", "conn_resolve"):
            for k in ("conn_create_none", "conn_create_none_by_id"):
                if k in out and y in out:
                    res[f"{k}_over_{y}"] = round(out[k]["ms"] / out[y]["ms"], 3)
        res["rounds"], res["reps"] = args.rounds, args.reps
        res["ms_rounds"] = {k: [round(x, 4) for x in times[k]] for k in out
                            if k.startswith(("conn_create_", "conn_old_", "conn_close_none", "conn_resolve"))}
    picks = [k for k in out if k.startswith("conn_pick_")]
    if picks:
        res["conn_pick_rows"] = {"client": 10, "server": [64, 10], "own_one": n_own, "own_groups": [g_own, 10],
                                 "distinct_conns_picked": pick_check}
        res["conn_pick_host_16t_ms"] = pick_host
        for k in picks:
            for y in ("conn_resolve", "conn_expand"):
                if y in out and "build" not in k:
                    res[f"{k}_over_{y}"] = round(out[k]["ms"] / out[y]["ms"], 3)
            if k in pick_host:
                res[f"{k}_host_over_device"] = round(pick_host[k] / out[k]["ms"], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
