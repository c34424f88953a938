"""Host-side mirror of rsock's codec surface over the HIP C-ABI.

Names follow the reference:
  * ``Codec.compute_hash`` / ``Codec.hash_equal``   <- util/rhash.h:13-17
  * ``Codec.enc2buf`` / ``Codec.decodebuf``          <- EncHead::Enc2Buf / DecodeBuf (bean/EncHead.h:38-40)
  * ``Codec.output_batch`` (RConn::Output framing)   <- conn/RConn.cpp:87-105
  * ``Codec.onrecv_batch`` (RConn::OnRecv)           <- conn/RConn.cpp:64-85
  * ``Codec.rawinput_batch`` (RawTcp::RawInput + OnRecv) <- conn/RawTcp.cpp:138-244
Batch arguments are torch tensors on the codec's device (torch is used only for memory and
streams).  Every call goes through ``rsock_amd/librsk.so``; there is no CPU path here.
"""
from __future__ import annotations

import ctypes

import numpy as np
from dataclasses import dataclass, fields

import torch

from . import _abi

_lib = None


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        _lib = _abi.load()
    return _lib


def _ptr(t) -> int | None:
    if t is None:
        return None
    return t.data_ptr()


def _stream(stream) -> int | None:
    if stream is None:
        return torch.cuda.current_stream().cuda_stream
    if isinstance(stream, int):
        return stream
    return stream.cuda_stream


class RskError(RuntimeError):
    pass


def _check(rc: int, what: str) -> None:
    if rc != 0:
        err = lib().rsk_last_error()
        raise RskError(f"{what} failed: rc={rc} ({err.decode() if err else ''})")


@dataclass
class DecodeBuffers:
    """SoA outputs of RConn::OnRecv for n frames (rsk_decode_out)."""

    hlen: torch.Tensor
    cmd: torch.Tensor
    id: torch.Tensor  # n*8 bytes
    conv: torch.Tensor  # int32 storage of u32
    conn_key: torch.Tensor  # int64 storage of u64
    pay_off: torch.Tensor  # int16 storage of u16
    pay_len: torch.Tensor  # int16 storage of u16
    status: torch.Tensor  # int8
    valid_idx: torch.Tensor  # int32 storage of u32
    n_valid: torch.Tensor  # int32 [1]

    @classmethod
    def alloc(cls, n: int, device) -> "DecodeBuffers":
        e = lambda k, dt: torch.empty(k, dtype=dt, device=device)  # noqa: E731
        return cls(
            hlen=e(n, torch.uint8),
            cmd=e(n, torch.uint8),
            id=e(n * 8, torch.uint8),
            conv=e(n, torch.int32),
            conn_key=e(n, torch.int64),
            pay_off=e(n, torch.int16),
            pay_len=e(n, torch.int16),
            status=e(n, torch.int8),
            valid_idx=e(max(n, 1), torch.int32),
            n_valid=e(1, torch.int32),
        )

    def abi(self, compact: bool = True) -> _abi.DecodeOut:
        return _abi.DecodeOut(
            _ptr(self.hlen), _ptr(self.cmd), _ptr(self.id), _ptr(self.conv), _ptr(self.conn_key),
            _ptr(self.pay_off), _ptr(self.pay_len), _ptr(self.status),
            _ptr(self.valid_idx) if compact else None, _ptr(self.n_valid) if compact else None,
        )

    def to_host(self) -> dict:
        out = {}
        for f in fields(self):
            out[f.name] = getattr(self, f.name).cpu().numpy()
        return out


def stage_capture_slots(arena: np.ndarray, offs: np.ndarray, cap_len: np.ndarray, slot: int,
                        nthreads: int = 8) -> np.ndarray:
    """Host staging for rsk_parse_decode_slots_batch (rsk_stage_capture_slots): an (n, slot) uint8
    array, row i = the first min(cap_len[i], slot) captured bytes of packet i, zero-filled."""
    n = len(offs)
    arena = np.ascontiguousarray(arena, np.uint8)
    offs = np.ascontiguousarray(offs, np.uint64)
    cap_len = np.ascontiguousarray(cap_len, np.uint32)
    slots = np.empty((n, slot), np.uint8)
    _check(lib().rsk_stage_capture_slots(n, arena.ctypes.data, offs.ctypes.data, cap_len.ctypes.data, slot,
                                         slots.ctypes.data, nthreads), "rsk_stage_capture_slots")
    return slots


def stage_decode_headers(arena: np.ndarray, offs: np.ndarray, lens: np.ndarray) -> np.ndarray:
    """Host staging for rsk_decode_headers_batch, vectorised (same bytes as rsk_stage_decode_header):
    slot = frame[0:min(32, len)] zero-filled, byte 31 = frame[8 + frame[8]] when that is inside."""
    n = len(offs)
    offs = offs.astype(np.int64)
    lens = lens.astype(np.int64)
    k = np.arange(32)
    idx = offs[:, None] + k[None, :]
    inside = k[None, :] < lens[:, None]
    slots = np.where(inside, arena[np.minimum(idx, len(arena) - 1)], 0).astype(np.uint8)
    has8 = lens > 8
    ln = np.where(has8, arena[np.minimum(offs + 8, len(arena) - 1)], 0).astype(np.int64)
    at = 8 + ln
    ok = has8 & (at < lens)
    slots[ok, 31] = arena[(offs + at)[ok]]
    return slots.reshape(n, 32)


def ip_u32(ip: str) -> int:
    """Dotted IPv4 -> the u32 the header stores (network-order bytes read little-endian)."""
    b = bytes(int(x) for x in ip.split("."))
    return int.from_bytes(b, "little")


def make_filter(src_ip: str | None = None, dst_ip: str | None = None, src_singles=(), src_ranges=(), dst_singles=(),
                dst_ranges=(), is_server: bool = False) -> _abi.CaptureFilter:
    """rsk_capture_filter from BuildFilterStr's inputs (srcIp, dstIp, srcPorts, dstPorts, isServer)."""
    f = _abi.CaptureFilter()
    if src_ip:
        f.src_ip, f.has_src_ip = ip_u32(src_ip), 1
    if dst_ip:
        f.dst_ip, f.has_dst_ip = ip_u32(dst_ip), 1
    f.is_server = 1 if is_server else 0
    for pl, singles, ranges in ((f.src_ports, src_singles, src_ranges), (f.dst_ports, dst_singles, dst_ranges)):
        assert len(singles) <= _abi.FILTER_MAX_PORTS and len(ranges) <= _abi.FILTER_MAX_PORTS
        pl.n_single, pl.n_range = len(singles), len(ranges)
        for q, v in enumerate(singles):
            pl.single[q] = v
        for q, (a, b) in enumerate(ranges):
            pl.range[q][0], pl.range[q][1] = a, b
    return f


def filter_str(filt: _abi.CaptureFilter) -> str:
    """BuildFilterStr's string for this filter (host function of librsk; no GPU needed)."""
    buf = ctypes.create_string_buffer(16384)
    n = lib().rsk_filter_str(ctypes.byref(filt), buf, len(buf))
    if n < 0:
        raise RskError("rsk_filter_str: buffer too small")
    return buf.value.decode()


@dataclass
class DemuxBuffers:
    """Outputs of rsk_demux_batch for a batch of n packets (rsk_demux_out)."""

    perm: torch.Tensor
    seg_off: torch.Tensor
    seg_first: torch.Tensor
    n_seg: torch.Tensor
    n_valid: torch.Tensor

    @classmethod
    def alloc(cls, n: int, device) -> "DemuxBuffers":
        e = lambda k: torch.empty(k, dtype=torch.int32, device=device)  # noqa: E731
        return cls(perm=e(max(n, 1)), seg_off=e(n + 1), seg_first=e(max(n, 1)), n_seg=e(1), n_valid=e(1))

    def abi(self) -> _abi.DemuxOut:
        return _abi.DemuxOut(*[_ptr(getattr(self, f.name)) for f in fields(self)])

    def segments(self):
        """Host view: list of (first packet, [packet indices]) in segment order."""
        ns, nv = int(self.n_seg.item()), int(self.n_valid.item())
        perm = self.perm[:nv].cpu().numpy().astype("uint32")
        off = self.seg_off[: ns + 1].cpu().numpy().astype("uint32")
        first = self.seg_first[:ns].cpu().numpy().astype("uint32")
        return [(int(first[s]), perm[off[s]:off[s + 1]].tolist()) for s in range(ns)]


@dataclass
class DeliverBuffers:
    """Outputs of rsk_deliver_batch for a batch of n packets (rsk_deliver_out): the dense payload
    arena (`cap` bytes; None for a plan-only buffer set), out_off [n + 1] and total [1] (int64
    storage of u64).  `cap` is the out_cap the next call passes (at most the arena's size)."""

    arena: torch.Tensor | None
    out_off: torch.Tensor
    total: torch.Tensor
    cap: int

    @classmethod
    def alloc(cls, n: int, device, cap: int = 0) -> "DeliverBuffers":
        return cls(arena=torch.empty(cap, dtype=torch.uint8, device=device) if cap else None,
                   out_off=torch.empty(n + 1, dtype=torch.int64, device=device),
                   total=torch.empty(1, dtype=torch.int64, device=device), cap=int(cap))

    def abi(self, align: int, plan_only: bool = False) -> _abi.DeliverOut:
        arena = None if plan_only else self.arena
        if arena is not None:
            assert 0 <= self.cap <= arena.numel()
        return _abi.DeliverOut(_ptr(arena), self.cap if arena is not None else 0, _ptr(self.out_off),
                               _ptr(self.total), align)


def segment_bytes(host_arena: np.ndarray, out_off, dmx, s: int) -> np.ndarray:
    """Segment s of a delivery made with order = dmx.perm (a DemuxBuffers, or its seg_off as an
    array), sliced out of a host copy of the delivered arena: the payloads of the segment's packets in
    arrival order, back to back (each rounded up to the delivery's align)."""
    seg_off = getattr(dmx, "seg_off", dmx)
    lo, hi = (int(x) for x in seg_off[s:s + 2])
    if isinstance(out_off, torch.Tensor):
        out_off = out_off.cpu().numpy()
    off = np.asarray(out_off).view(np.uint64)
    return host_arena[int(off[lo]):int(off[hi])]


def deliver_host(arena: np.ndarray, base_off: np.ndarray, pay_off: np.ndarray, pay_len: np.ndarray,
                 status: np.ndarray, inner_off: np.ndarray | None = None, order: np.ndarray | None = None,
                 n_order: int | None = None, align: int = 1, out: np.ndarray | None = None, cap: int | None = None,
                 plan_only: bool = False, nthreads: int = 1):
    """rsk_deliver_host on numpy arrays (no GPU): -> (out_arena or None, out_off uint64 [n + 1], total).
    `out` is a 16-B aligned uint8 array to deliver into (cap defaults to its size); without one, the
    call plans first and allocates exactly the total."""
    n = len(status)
    c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    arena, base_off, inner_off = c(arena, np.uint8), c(base_off, np.uint64), c(inner_off, np.uint16)
    pay_off, pay_len, status, order = c(pay_off, np.uint16), c(pay_len, np.uint16), c(status, np.int8), c(order, np.uint32)
    if (order is None) != (n_order is None):
        raise RskError("rsk_deliver_host failed: rc=-22 (order and n_order go together)")
    cnt = None if n_order is None else np.array([n_order], np.uint32)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    din = _abi.DeliverIn(p(arena), p(base_off), p(inner_off), p(pay_off), p(pay_len), p(status), p(order), p(cnt))
    off = np.empty(n + 1, np.uint64)
    tot = np.zeros(1, np.uint64)

    def call(dst, dcap):
        dout = _abi.DeliverOut(p(dst), dcap, off.ctypes.data, tot.ctypes.data, align)
        rc = lib().rsk_deliver_host(n, ctypes.byref(din), ctypes.byref(dout), nthreads)
        if rc != 0:
            raise RskError(f"rsk_deliver_host failed: rc={rc}")

    if plan_only:
        call(None, 0)
        return None, off, int(tot[0])
    if out is None:
        call(None, 0)
        raw = np.empty(int(tot[0]) + 16, np.uint8)
        sh = (-raw.ctypes.data) % 16
        out = raw[sh:sh + int(tot[0])]
    call(out, len(out) if cap is None else cap)
    return out, off, int(tot[0])


def verify_wire_host(cap: np.ndarray, cap_off: np.ndarray, cap_len: np.ndarray, datalink: int,
                     status: np.ndarray | None = None, want_status_out: bool = False, nthreads: int = 1):
    """rsk_verify_wire_host on numpy arrays (no GPU): -> (csum uint8 [n], status_out int8 [n] or None,
    n_bad).  `status` gates the check to its RSK_RECV_VALID packets; want_status_out (needs `status`)
    also returns the status with the bad packets dropped."""
    n = len(cap_len)
    c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    cap, cap_off, cap_len, status = c(cap, np.uint8), c(cap_off, np.uint64), c(cap_len, np.uint32), c(status, np.int8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    csum = np.full(max(n, 1), 0xEE, np.uint8)
    sout = np.full(max(n, 1), 0x55, np.int8) if want_status_out else None
    nb = np.full(1, 0xFFFFFFFF, np.uint32)
    vin = _abi.VerifyIn(p(cap), p(cap_off), p(cap_len), p(status))
    vout = _abi.VerifyOut(p(csum), p(sout), p(nb))
    rc = lib().rsk_verify_wire_host(n, ctypes.byref(vin), datalink, ctypes.byref(vout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_verify_wire_host failed: rc={rc}")
    return csum[:n], None if sout is None else sout[:n], int(nb[0])


_CONN_COLUMNS = (("state", torch.uint8, 1), ("conn_key", torch.int64, 1), ("id", torch.uint8, 8),
                 ("src", torch.int32, 1), ("dst", torch.int32, 1), ("sp", torch.int16, 1), ("dp", torch.int16, 1),
                 ("seq", torch.int32, 1), ("ack", torch.int32, 1), ("flag", torch.uint8, 1))


@dataclass
class ConnTable:
    """The fake-TCP connection table (rsk_conn_table): `capacity` rows in columns of torch tensors (signed
    storage of the unsigned C types, as the other buffers here) plus the opaque index.  On a device the
    batch calls of Codec take it; on "cpu" the host twins below do.  Rows are edited with ordinary tensor
    writes; after any change to state, conn_key or id call rebuild()."""

    capacity: int
    by_id: bool
    state: torch.Tensor     # uint8: CONN_LIVE | CONN_ALIVE
    conn_key: torch.Tensor  # int64 storage of u64
    id: torch.Tensor | None  # capacity * 8 bytes; by_id only
    src: torch.Tensor
    dst: torch.Tensor
    sp: torch.Tensor
    dp: torch.Tensor
    seq: torch.Tensor       # the conn_seq of tcp_send_seq_batch
    ack: torch.Tensor       # the conn_ack of tcp_recv_ack_batch
    flag: torch.Tensor
    index: torch.Tensor     # opaque, rsk_conn_index_bytes bytes
    pick: torch.Tensor | None = None  # opaque, rsk_conn_pick_bytes bytes: the send pick's index (rebuild_pick)

    @classmethod
    def alloc(cls, capacity: int, device, by_id: bool = False) -> "ConnTable":
        nbytes = lib().rsk_conn_index_bytes(capacity, _abi.CONN_BY_ID if by_id else 0)
        pbytes = lib().rsk_conn_pick_bytes(capacity, _abi.CONN_BY_ID if by_id else 0)
        if nbytes == 0 or pbytes == 0:
            raise RskError(f"rsk_conn_index_bytes: bad capacity {capacity}")
        cols = {name: torch.zeros(capacity * k, dtype=dt, device=device) for name, dt, k in _CONN_COLUMNS}
        if not by_id:
            cols["id"] = None
        return cls(capacity=int(capacity), by_id=bool(by_id), index=torch.empty(nbytes // 4, dtype=torch.int32,
                                                                               device=device),
                   pick=torch.zeros(pbytes // 4, dtype=torch.int32, device=device), **cols)

    @property
    def flags(self) -> int:
        return _abi.CONN_BY_ID if self.by_id else 0

    def abi(self) -> _abi.ConnTable:
        return _abi.ConnTable(self.capacity, self.flags, *[_ptr(getattr(self, name)) for name, _, _ in _CONN_COLUMNS],
                              _ptr(self.index))

    def load(self, **cols) -> "ConnTable":
        """Copy numpy arrays (any integer dtype of the column's width) into the named columns."""
        for name, a in cols.items():
            t = getattr(self, name)
            a = np.ascontiguousarray(a)
            t.copy_(torch.from_numpy(a.view(f"i{a.dtype.itemsize}" if t.dtype != torch.uint8 else np.uint8)))
        return self

    def to(self, device) -> "ConnTable":
        """A copy of every column, of the index and of the pick index on `device` (both are valid on either
        side)."""
        mv = lambda t: None if t is None else t.to(device, copy=True)  # noqa: E731
        return ConnTable(self.capacity, self.by_id, *[mv(getattr(self, name)) for name, _, _ in _CONN_COLUMNS],
                         mv(self.index), mv(self.pick))

    def abi_rows(self) -> _abi.ConnRows:
        """The writable alias of state that conn_close_batch / conn_close_host take."""
        return _abi.ConnRows(_ptr(self.state))

    def close_work(self) -> torch.Tensor:
        """The work buffer of conn_close_batch / conn_close_host (rsk_conn_close_bytes), on the table's device;
        one per stream that runs the call."""
        nbytes = lib().rsk_conn_close_bytes(self.capacity, self.flags)
        if nbytes == 0:
            raise RskError(f"rsk_conn_close_bytes: bad capacity {self.capacity}")
        return torch.empty(nbytes // 4, dtype=torch.int32, device=self.index.device)

    def abi_create_rows(self) -> _abi.ConnCreateRows:
        """The writable aliases of the columns that conn_create_batch / conn_create_host take."""
        return _abi.ConnCreateRows(*[_ptr(getattr(self, name)) for name, _, _ in _CONN_COLUMNS])

    def create_work(self, u_max: int, m_max: int) -> torch.Tensor:
        """The work buffer of conn_create_batch / conn_create_host for at most u_max considered packets and m_max
        offers per call (rsk_conn_create_bytes), on the table's device; one per stream that runs the call."""
        nbytes = lib().rsk_conn_create_bytes(u_max, m_max, self.capacity, self.flags)
        if nbytes == 0:
            raise RskError(f"rsk_conn_create_bytes: bad u_max {u_max} / m_max {m_max}")
        return torch.empty(nbytes // 4, dtype=torch.int32, device=self.index.device)

    def rebuild(self, codec: "Codec | None" = None, stream=None, n_dup: torch.Tensor | None = None) -> None:
        """rsk_conn_index_build on `stream` (a device table, with its Codec), or the host twin (a "cpu"
        table, codec None).  n_dup [1] receives the LIVE rows that lost their key to a lower row."""
        if (codec is None) != (self.index.device.type == "cpu"):
            raise RskError("ConnTable.rebuild: a device table takes its Codec, a cpu table none")
        if codec is None:
            _check(lib().rsk_conn_index_build_host(ctypes.byref(self.abi()), _ptr(n_dup), 1),
                   "rsk_conn_index_build_host")
        else:
            codec.conn_index_build(self, n_dup=n_dup, stream=stream)

    def rebuild_pick(self, codec: "Codec | None" = None, stream=None, counts: torch.Tensor | None = None) -> None:
        """rsk_conn_pick_build on `stream` (a device table, with its Codec), or the host twin (a "cpu" table,
        codec None): the pick index from state (and id); call it after any change to them.  counts [2]
        receives the groups that have a candidate and the candidates."""
        if (codec is None) != (self.pick.device.type == "cpu"):
            raise RskError("ConnTable.rebuild_pick: a device table takes its Codec, a cpu table none")
        if codec is None:
            conn_pick_build_host(self, counts=counts)
        else:
            codec.conn_pick_build(self, counts=counts, stream=stream)


def _np_ptr(a):
    return None if a is None else a.ctypes.data


def conn_pick_build_host(tab: ConnTable, counts=None, nthreads: int = 1) -> None:
    """rsk_conn_pick_build_host on a "cpu" ConnTable: tab.pick from its state (and id) columns; counts [2]
    (tensor or numpy) receives the groups that have a candidate and the candidates."""
    _check(lib().rsk_conn_pick_build_host(ctypes.byref(tab.abi()), _ptr(tab.pick), _addr(counts), nthreads),
           "rsk_conn_pick_build_host")


def conn_pick_host(tab: ConnTable, n: int, len=None, id=None, avoid_key=None, draw=None, seed: int = 0,
                   used: np.ndarray | None = None, nthreads: int = 1):
    """rsk_conn_pick_host on a "cpu" ConnTable and numpy columns (no GPU): -> (conn uint32 [n], n_none).
    used [capacity] uint8, when given, gets 1 at every picked row."""
    c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    len, id, avoid_key, draw = c(len, np.int32), c(id, np.uint8), c(avoid_key, np.uint64), c(draw, np.uint32)
    conn = np.full(max(n, 1), 0xEEEEEEEE, np.uint32)
    nn = np.full(1, 0xFFFFFFFF, np.uint32)
    pin = _abi.ConnPickIn(_np_ptr(len), _np_ptr(id), _np_ptr(avoid_key), _np_ptr(draw), seed & 0xFFFFFFFFFFFFFFFF)
    pout = _abi.ConnPickOut(_np_ptr(conn), _np_ptr(nn), _np_ptr(used))
    rc = lib().rsk_conn_pick_host(ctypes.byref(tab.abi()), _ptr(tab.pick), n, ctypes.byref(pin), ctypes.byref(pout),
                                  nthreads)
    if rc != 0:
        raise RskError(f"rsk_conn_pick_host failed: rc={rc}")
    return conn[:n], int(nn[0])


def conn_resolve_host(tab: ConnTable, status: np.ndarray, conn_key: np.ndarray, cmd: np.ndarray | None = None,
                      id: np.ndarray | None = None, nthreads: int = 1):
    """rsk_conn_resolve_host on a "cpu" ConnTable and numpy columns (no GPU): -> (conn uint32 [n], hit
    uint8 [n], miss int8 [n], n_miss)."""
    n = len(status)
    c = lambda a, dt: None if a is None else np.ascontiguousarray(a, dt)  # noqa: E731
    status, conn_key, cmd, id = c(status, np.int8), c(conn_key, np.uint64), c(cmd, np.uint8), c(id, np.uint8)
    conn, hit, miss = np.full(max(n, 1), 0xEEEEEEEE, np.uint32), np.full(max(n, 1), 0xEE, np.uint8), np.full(max(n, 1), 0x55, np.int8)
    nm = np.full(1, 0xFFFFFFFF, np.uint32)
    rin = _abi.ConnResolveIn(_np_ptr(status), _np_ptr(cmd), _np_ptr(id), _np_ptr(conn_key))
    rout = _abi.ConnResolveOut(_np_ptr(conn), _np_ptr(hit), _np_ptr(miss), _np_ptr(nm))
    rc = lib().rsk_conn_resolve_host(ctypes.byref(tab.abi()), n, ctypes.byref(rin), ctypes.byref(rout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conn_resolve_host failed: rc={rc}")
    return conn[:n], hit[:n], miss[:n], int(nm[0])


def conn_expand_host(tab: ConnTable, conn: np.ndarray, nthreads: int = 1):
    """rsk_conn_expand_host on a "cpu" ConnTable (no GPU): -> (dict of the columns src, dst, sp, dp, ack,
    flag, conn_key, ok and, for a by_id table, id [n * 8]; n_bad)."""
    n = len(conn)
    conn = np.ascontiguousarray(conn, np.uint32)
    m = max(n, 1)
    o = {"src": np.full(m, 0xEEEEEEEE, np.uint32), "dst": np.full(m, 0xEEEEEEEE, np.uint32),
         "sp": np.full(m, 0xEEEE, np.uint16), "dp": np.full(m, 0xEEEE, np.uint16),
         "ack": np.full(m, 0xEEEEEEEE, np.uint32), "flag": np.full(m, 0xEE, np.uint8),
         "conn_key": np.full(m, 0xEE, np.uint64), "id": np.full(8 * m, 0xEE, np.uint8) if tab.by_id else None,
         "ok": np.full(m, 0xEE, np.uint8)}
    nb = np.full(1, 0xFFFFFFFF, np.uint32)
    eout = _abi.ConnExpandOut(*[_np_ptr(o[k]) for k in ("src", "dst", "sp", "dp", "ack", "flag", "conn_key", "id", "ok")],
                              _np_ptr(nb))
    rc = lib().rsk_conn_expand_host(ctypes.byref(tab.abi()), n, _np_ptr(conn), ctypes.byref(eout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conn_expand_host failed: rc={rc}")
    return {k: (v[:8 * n] if k == "id" else v[:n]) for k, v in o.items() if v is not None}, int(nb[0])


def _addr(a) -> int | None:
    """Address of a torch tensor or a numpy array (None stays None)."""
    if a is None:
        return None
    return a.data_ptr() if isinstance(a, torch.Tensor) else a.ctypes.data


def _conn_close_structs(tab, close_rows, n_close, m_max, rst_first, work, remove, sweep, marked_rows, n_marked,
                        closed_rows, n_closed, pick, pick_counts):
    if m_max is None:
        m_max = 0 if close_rows is None else len(close_rows)
    flags = (_abi.CONN_CLOSE_REMOVE if remove else 0) | (_abi.CONN_CLOSE_SWEEP if sweep else 0)
    cin = _abi.ConnCloseIn(_addr(close_rows), _addr(n_close), int(m_max), _addr(rst_first), _addr(work), flags)
    cout = _abi.ConnCloseOut(_addr(marked_rows), _addr(n_marked), _addr(closed_rows), _addr(n_closed),
                             _addr(tab.pick) if pick else None, _addr(pick_counts))
    return cin, cout


def conn_close_host(tab: ConnTable, work, close_rows=None, n_close=None, m_max: int | None = None, rst_first=None,
                    remove: bool = False, sweep: bool = False, marked_rows=None, n_marked=None, closed_rows=None,
                    n_closed=None, pick: bool = False, pick_counts=None, nthreads: int = 1) -> None:
    """rsk_conn_close_host on a "cpu" ConnTable (no GPU); the arguments of Codec.conn_close_batch."""
    cin, cout = _conn_close_structs(tab, close_rows, n_close, m_max, rst_first, work, remove, sweep, marked_rows,
                                    n_marked, closed_rows, n_closed, pick, pick_counts)
    rc = lib().rsk_conn_close_host(ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()), ctypes.byref(cin),
                                   ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conn_close_host failed: rc={rc}")


@dataclass
class ConnOffers:
    """The offers of conn_create_batch / conn_create_host (rsk_conn_offers): columns of m_max entries (torch
    tensors on the table's device, or numpy arrays for the host twin) and the device word n_offer.  conn_key and
    id are the list form's."""

    src: object
    dst: object
    sp: object
    dp: object
    ack: object
    flag: object
    n_offer: object
    conn_key: object = None
    id: object = None
    m_max: int | None = None

    def abi(self) -> _abi.ConnOffers:
        m = len(self.src) if self.m_max is None else int(self.m_max)
        return _abi.ConnOffers(_addr(self.src), _addr(self.dst), _addr(self.sp), _addr(self.dp), _addr(self.ack),
                               _addr(self.flag), _addr(self.conn_key), _addr(self.id), _addr(self.n_offer), m)


def _conn_create_structs(tab, offers, work, kw):
    """-> (n, rsk_conn_create_in, rsk_conn_create_out) from the keyword arguments of Codec.conn_create_batch."""
    g = kw.get
    flags = (_abi.CONN_CREATE_LIST if g("list_form") else 0) | (_abi.CONN_CREATE_REPEAT if g("repeat") else 0)
    miss = g("miss")
    n = g("n")
    if n is None:
        n = 0 if miss is None else len(miss)
    cin = _abi.ConnCreateIn(_addr(g("id")), _addr(g("conn_key")), _addr(g("src")), _addr(g("dst")), _addr(g("sp")),
                            _addr(g("dp")), offers.abi(), int(g("u_max") or 0), flags,
                            int(g("now_ms") or 0) & 0xFFFFFFFFFFFFFFFF, _addr(g("established_ms")), _addr(g("ka_tries")),
                            _addr(work))
    cout = _abi.ConnCreateOut(_addr(g("conn")), _addr(g("hit")), _addr(miss), _addr(g("n_miss")), _addr(g("new_rows")),
                              _addr(g("new_first")), _addr(g("new_offer")), _addr(g("offer_row")), _addr(g("n_new")),
                              _addr(g("n_full")), _addr(g("n_refused")), _addr(tab.pick) if g("pick") else None,
                              _addr(g("pick_counts")))
    return int(n), cin, cout


_CONN_CREATE_KW = frozenset(("n", "u_max", "id", "conn_key", "src", "dst", "sp", "dp", "conn", "hit", "miss", "n_miss",
                             "list_form", "repeat", "now_ms", "established_ms", "ka_tries", "new_rows", "new_first",
                             "new_offer", "offer_row", "n_new", "n_full", "n_refused", "pick", "pick_counts"))


def conn_create_bytes(u_max: int, m_max: int, capacity: int, by_id: bool = False) -> int:
    """rsk_conn_create_bytes: the work buffer's size, 0 for bad arguments."""
    return int(lib().rsk_conn_create_bytes(u_max, m_max, capacity, _abi.CONN_BY_ID if by_id else 0))


def conn_create_host(tab: ConnTable, offers: ConnOffers, work, nthreads: int = 1, **kw) -> None:
    """rsk_conn_create_host on a "cpu" ConnTable (no GPU); the keyword arguments of Codec.conn_create_batch."""
    if set(kw) - _CONN_CREATE_KW:
        raise TypeError(f"conn_create_host: unknown arguments {sorted(set(kw) - _CONN_CREATE_KW)}")
    n, cin, cout = _conn_create_structs(tab, offers, work, kw)
    rc = lib().rsk_conn_create_host(ctypes.byref(tab.abi()), ctypes.byref(tab.abi_create_rows()), n, ctypes.byref(cin),
                                    ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conn_create_host failed: rc={rc}")


_MSG_COLUMNS = (("msg_cmd", torch.uint8, 1), ("msg_body", torch.int64, 1), ("msg_id", torch.uint8, 8),
                ("msg_src", torch.int32, 1), ("msg_avoid_key", torch.int64, 1), ("msg_pay_off", torch.int64, 1),
                ("msg_pay_len", torch.int16, 1))


@dataclass
class ControlBuffers:
    """Outputs of rsk_control_batch for n packets and of rsk_keepalive_flush for a table of `capacity`
    rows (rsk_control_out, rsk_keepalive_out, rsk_ctl_msgs), on a device or on "cpu" for the host twins;
    signed storage of the unsigned C types.  kind / arg / conn [n] and n_ctl [1]; rst_first [capacity];
    the message columns msg_* [m] with n_msg [1] -- an rsk_encode_in as they stand: payload = msg_body
    viewed as bytes, pay_off = msg_pay_off, pay_len = msg_pay_len, cmd = msg_cmd, id = msg_id;
    dead_rows [capacity] with n_dead [1].  Any field may be set to None before a call: every output is
    optional (n_msg is needed with a message column, n_dead with dead_rows)."""

    kind: torch.Tensor | None
    arg: torch.Tensor | None
    conn: torch.Tensor | None
    n_ctl: torch.Tensor | None
    rst_first: torch.Tensor | None
    msg_cmd: torch.Tensor | None
    msg_body: torch.Tensor | None
    msg_id: torch.Tensor | None
    msg_src: torch.Tensor | None
    msg_avoid_key: torch.Tensor | None
    msg_pay_off: torch.Tensor | None
    msg_pay_len: torch.Tensor | None
    n_msg: torch.Tensor | None
    dead_rows: torch.Tensor | None
    n_dead: torch.Tensor | None

    @classmethod
    def alloc(cls, n: int, device, capacity: int = 0, m: int | None = None) -> "ControlBuffers":
        """For control_batch: alloc(n, device, capacity) (m = n message entries).  For keepalive_flush:
        alloc(0, device, capacity, m=capacity)."""
        m = n if m is None else m
        e = lambda k, dt: torch.empty(k, dtype=dt, device=device)  # noqa: E731
        return cls(kind=e(n, torch.uint8), arg=e(n, torch.int64), conn=e(n, torch.int32), n_ctl=e(1, torch.int32),
                   rst_first=e(capacity, torch.int32) if capacity else None,
                   **{name: e(m * k, dt) for name, dt, k in _MSG_COLUMNS}, n_msg=e(1, torch.int32),
                   dead_rows=e(capacity, torch.int32) if capacity else None, n_dead=e(1, torch.int32))

    def abi_msgs(self) -> _abi.CtlMsgs:
        return _abi.CtlMsgs(*[_addr(getattr(self, name)) for name, _, _ in _MSG_COLUMNS], _addr(self.n_msg))

    def abi_control(self, ka_tries=None) -> _abi.ControlOut:
        return _abi.ControlOut(_addr(self.kind), _addr(self.arg), _addr(self.conn), _addr(self.n_ctl),
                               _addr(self.rst_first), _addr(ka_tries), self.abi_msgs())

    def abi_flush(self) -> _abi.KeepaliveOut:
        return _abi.KeepaliveOut(self.abi_msgs(), _addr(self.dead_rows), _addr(self.n_dead))

    def messages(self) -> dict:
        """The first n_msg entries of the given message columns on the host (numpy, unsigned; id as
        [n_msg, 8] bytes)."""
        k = int(self.n_msg.cpu().numpy().view(np.uint32)[0])
        out = {}
        for name, dt, w in _MSG_COLUMNS:
            t = getattr(self, name)
            if t is not None:
                a = t[:k * w].cpu().numpy()
                out[name[4:]] = a.reshape(k, 8) if w == 8 else a.view(f"u{a.dtype.itemsize}")
        return out


def _control_in(status, cmd, pay_off, pay_len, arena, base_off, id, conn_key, inner_off, tcp_sp, tcp_dp,
                miss) -> _abi.ControlIn:
    return _abi.ControlIn(_addr(status), _addr(cmd), _addr(id), _addr(conn_key), _addr(pay_off), _addr(pay_len),
                          _addr(arena), _addr(base_off), _addr(inner_off), _addr(tcp_sp), _addr(tcp_dp), _addr(miss))


def control_host(tab: ConnTable, status, cmd, pay_off, pay_len, arena, base_off, out: ControlBuffers, id=None,
                 conn_key=None, inner_off=None, tcp_sp=None, tcp_dp=None, miss=None, ka_tries=None,
                 nthreads: int = 1) -> None:
    """rsk_control_host on a "cpu" ConnTable, with "cpu" tensors or numpy arrays of the C types' widths
    (no GPU); the arguments of Codec.control_batch."""
    cin = _control_in(status, cmd, pay_off, pay_len, arena, base_off, id, conn_key, inner_off, tcp_sp, tcp_dp, miss)
    rc = lib().rsk_control_host(ctypes.byref(tab.abi()), len(status), ctypes.byref(cin),
                                ctypes.byref(out.abi_control(ka_tries)), nthreads)
    if rc != 0:
        raise RskError(f"rsk_control_host failed: rc={rc}")


def keepalive_flush_host(tab: ConnTable, ka_tries, established_ms, now_ms: int, out: ControlBuffers,
                         request_delay_ms: int = _abi.KA_REQUEST_DELAY_MS, max_retry: int = _abi.KA_MAX_RETRY,
                         online: bool = True, nthreads: int = 1) -> None:
    """rsk_keepalive_flush_host on a "cpu" ConnTable (no GPU); the arguments of Codec.keepalive_flush."""
    ka = _abi.Keepalive(_addr(ka_tries), _addr(established_ms), now_ms, request_delay_ms, max_retry, int(online))
    rc = lib().rsk_keepalive_flush_host(ctypes.byref(tab.abi()), ctypes.byref(ka), ctypes.byref(out.abi_flush()),
                                        nthreads)
    if rc != 0:
        raise RskError(f"rsk_keepalive_flush_host failed: rc={rc}")


_CONV_COLUMNS = (("state", torch.uint8, 1), ("conv", torch.int32, 1), ("dst", torch.int32, 1), ("id", torch.uint8, 8),
                 ("cur_in", torch.int32, 1), ("cur_out", torch.int32, 1), ("prev_in", torch.int32, 1),
                 ("prev_out", torch.int32, 1), ("alive", torch.uint8, 1))


@dataclass
class ConvTable:
    """The conv table (rsk_conv_table): a group's convs at the app level -- a server's SubGroups
    (by_dst and by_id), a ClientGroup's mConvMap (neither) -- with the DataStat words of each, in columns
    of torch tensors (signed storage of the unsigned C types) plus the opaque index.  Shaped like
    ConnTable: on a device the batch calls of Codec take it, on "cpu" the host twins below; after any
    change to state, conv, dst or id call rebuild().  A column set to None is passed as NULL (cur_in
    None: the resolve does not count)."""

    capacity: int
    by_dst: bool
    by_id: bool
    state: torch.Tensor          # uint8: CONN_LIVE
    conv: torch.Tensor
    dst: torch.Tensor | None     # by_dst only
    id: torch.Tensor | None      # capacity * 8 bytes; by_id only
    cur_in: torch.Tensor | None
    cur_out: torch.Tensor | None
    prev_in: torch.Tensor | None
    prev_out: torch.Tensor | None
    alive: torch.Tensor | None   # uint8; set to 1 when a row is created
    index: torch.Tensor          # opaque, rsk_conn_index_bytes(capacity, 0) bytes

    @classmethod
    def alloc(cls, capacity: int, device, by_dst: bool = False, by_id: bool = False) -> "ConvTable":
        nbytes = lib().rsk_conn_index_bytes(capacity, 0)
        if nbytes == 0:
            raise RskError(f"rsk_conn_index_bytes: bad capacity {capacity}")
        cols = {name: torch.zeros(capacity * k, dtype=dt, device=device) for name, dt, k in _CONV_COLUMNS}
        if not by_dst:
            cols["dst"] = None
        if not by_id:
            cols["id"] = None
        return cls(capacity=int(capacity), by_dst=bool(by_dst), by_id=bool(by_id),
                   index=torch.empty(nbytes // 4, dtype=torch.int32, device=device), **cols)

    @property
    def flags(self) -> int:
        return (_abi.CONV_BY_DST if self.by_dst else 0) | (_abi.CONV_BY_ID if self.by_id else 0)

    def abi(self) -> _abi.ConvTable:
        return _abi.ConvTable(self.capacity, self.flags, *[_ptr(getattr(self, name)) for name, _, _ in _CONV_COLUMNS],
                              _ptr(self.index))

    def load(self, **cols) -> "ConvTable":
        """Copy numpy arrays (any integer dtype of the column's width) into the named columns."""
        for name, a in cols.items():
            t = getattr(self, name)
            a = np.ascontiguousarray(a)
            t.copy_(torch.from_numpy(a.view(f"i{a.dtype.itemsize}" if t.dtype != torch.uint8 else np.uint8)))
        return self

    def to(self, device) -> "ConvTable":
        """A copy of every column and of the index on `device` (the index is valid on either side)."""
        mv = lambda t: None if t is None else t.to(device, copy=True)  # noqa: E731
        return ConvTable(self.capacity, self.by_dst, self.by_id, *[mv(getattr(self, name)) for name, _, _ in _CONV_COLUMNS],
                         mv(self.index))

    def column(self, name: str) -> np.ndarray:
        """A column on the host as its unsigned C type."""
        a = getattr(self, name).cpu().numpy()
        return a.view(f"u{a.dtype.itemsize}")

    def abi_rows(self) -> _abi.ConvRows:
        """The writable aliases of the key columns that rsk_conv_create_batch takes."""
        return _abi.ConvRows(_ptr(self.state), _ptr(self.conv), _ptr(self.dst), _ptr(self.id))

    def create_work(self, u_max: int) -> torch.Tensor:
        """The work buffer of conv_create_batch / conv_create_host for at most u_max considered packets
        per call (rsk_conv_create_bytes), on the table's device; one per stream that runs the call."""
        nbytes = lib().rsk_conv_create_bytes(u_max, self.capacity)
        if nbytes == 0:
            raise RskError(f"rsk_conv_create_bytes: bad u_max {u_max}")
        return torch.empty(nbytes // 4, dtype=torch.int32, device=self.index.device)

    def close_work(self) -> torch.Tensor:
        """The work buffer of the timer form of conv_close_batch / conv_close_host (rsk_conv_close_bytes), on the
        table's device; one per stream that runs the call."""
        nbytes = lib().rsk_conv_close_bytes(self.capacity)
        if nbytes == 0:
            raise RskError(f"rsk_conv_close_bytes: bad capacity {self.capacity}")
        return torch.empty(nbytes // 4, dtype=torch.int32, device=self.index.device)

    def rebuild(self, codec: "Codec | None" = None, stream=None, n_dup: torch.Tensor | None = None) -> None:
        """rsk_conv_index_build on `stream` (a device table, with its Codec), or the host twin (a "cpu"
        table, codec None).  n_dup [1] receives the LIVE rows that lost their key to a lower row."""
        if (codec is None) != (self.index.device.type == "cpu"):
            raise RskError("ConvTable.rebuild: a device table takes its Codec, a cpu table none")
        if codec is None:
            _check(lib().rsk_conv_index_build_host(ctypes.byref(self.abi()), _ptr(n_dup), 1),
                   "rsk_conv_index_build_host")
        else:
            codec.conv_index_build(self, n_dup=n_dup, stream=stream)


def _conv_resolve_structs(status, conv, conv_row, cmd, hit, id, dst, ctl_kind, ctl_arg, unknown, n_unknown, rst_first,
                          msgs):
    cin = _abi.ConvResolveIn(_addr(status), _addr(cmd), _addr(hit), _addr(id), _addr(conv), _addr(dst),
                             _addr(ctl_kind), _addr(ctl_arg))
    cout = _abi.ConvResolveOut(_addr(conv_row), _addr(unknown), _addr(n_unknown), _addr(rst_first),
                               msgs.abi_msgs() if msgs is not None else _abi.CtlMsgs())
    return cin, cout


def conv_resolve_host(tab: ConvTable, status, conv, conv_row, cmd=None, hit=None, id=None, dst=None, ctl_kind=None,
                      ctl_arg=None, unknown=None, n_unknown=None, rst_first=None, msgs: "ControlBuffers | None" = None,
                      nthreads: int = 1) -> None:
    """rsk_conv_resolve_host on a "cpu" ConvTable, with "cpu" tensors or numpy arrays of the C types'
    widths (no GPU); the arguments of Codec.conv_resolve_batch."""
    cin, cout = _conv_resolve_structs(status, conv, conv_row, cmd, hit, id, dst, ctl_kind, ctl_arg, unknown, n_unknown,
                                      rst_first, msgs)
    rc = lib().rsk_conv_resolve_host(ctypes.byref(tab.abi()), len(status), ctypes.byref(cin), ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conv_resolve_host failed: rc={rc}")


def _conv_create_structs(conv, conv_row, unknown, u_max, work, id, dst, n_unknown, new_rows, new_first, n_new, n_full):
    cin = _abi.ConvCreateIn(_addr(id), _addr(conv), _addr(dst), int(u_max), _addr(work))
    cout = _abi.ConvCreateOut(_addr(conv_row), _addr(unknown), _addr(n_unknown), _addr(new_rows), _addr(new_first),
                              _addr(n_new), _addr(n_full))
    return cin, cout


def conv_create_host(tab: ConvTable, conv, conv_row, unknown, u_max: int, work, id=None, dst=None, n_unknown=None,
                     new_rows=None, new_first=None, n_new=None, n_full=None, nthreads: int = 1) -> None:
    """rsk_conv_create_host on a "cpu" ConvTable (no GPU); the arguments of Codec.conv_create_batch."""
    cin, cout = _conv_create_structs(conv, conv_row, unknown, u_max, work, id, dst, n_unknown, new_rows, new_first,
                                     n_new, n_full)
    rc = lib().rsk_conv_create_host(ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()), len(conv_row), ctypes.byref(cin),
                                    ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conv_create_host failed: rc={rc}")


def _conv_close_structs(close_rows, n_close, m_max, rst_first, ctl_kind, work, hold, conv_row, unknown, n_unknown,
                        closed_rows, closed_at, n_closed, n_reopened, n_rst_again):
    if m_max is None:
        m_max = 0 if close_rows is None else len(close_rows)
    cin = _abi.ConvCloseIn(_addr(close_rows), _addr(n_close), int(m_max), _addr(rst_first), _addr(ctl_kind), _addr(work),
                           _abi.CONV_CLOSE_HOLD if hold else 0)
    cout = _abi.ConvCloseOut(_addr(conv_row), _addr(unknown), _addr(n_unknown), _addr(closed_rows), _addr(closed_at),
                             _addr(n_closed), _addr(n_reopened), _addr(n_rst_again))
    return cin, cout


def conv_close_host(tab: ConvTable, close_rows=None, n_close=None, m_max: int | None = None, work=None, rst_first=None,
                    ctl_kind=None, conv_row=None, unknown=None, n_unknown=None, hold: bool = False, closed_rows=None,
                    closed_at=None, n_closed=None, n_reopened=None, n_rst_again=None, nthreads: int = 1) -> None:
    """rsk_conv_close_host on a "cpu" ConvTable (no GPU); the arguments of Codec.conv_close_batch."""
    cin, cout = _conv_close_structs(close_rows, n_close, m_max, rst_first, ctl_kind, work, hold, conv_row, unknown,
                                    n_unknown, closed_rows, closed_at, n_closed, n_reopened, n_rst_again)
    n = 0 if conv_row is None else len(conv_row)
    rc = lib().rsk_conv_close_host(ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()), n, ctypes.byref(cin),
                                   ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conv_close_host failed: rc={rc}")


def conv_send_host(tab: ConvTable, conv_row, sent=None, conv=None, dst=None, id=None, ok=None, n_bad=None,
                   nthreads: int = 1) -> None:
    """rsk_conv_send_host on a "cpu" ConvTable (no GPU); the arguments of Codec.conv_send_batch."""
    sout = _abi.ConvSendOut(_addr(conv), _addr(dst), _addr(id), _addr(ok), _addr(n_bad))
    rc = lib().rsk_conv_send_host(ctypes.byref(tab.abi()), len(conv_row), _addr(conv_row), _addr(sent), ctypes.byref(sout),
                                  nthreads)
    if rc != 0:
        raise RskError(f"rsk_conv_send_host failed: rc={rc}")


def conv_flush_host(tab: ConvTable, dead_rows=None, n_dead=None, n_alive=None, nthreads: int = 1) -> None:
    """rsk_conv_flush_host on a "cpu" ConvTable (no GPU); the arguments of Codec.conv_flush."""
    fout = _abi.ConvFlushOut(_addr(dead_rows), _addr(n_dead), _addr(n_alive))
    rc = lib().rsk_conv_flush_host(ctypes.byref(tab.abi()), ctypes.byref(fout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_conv_flush_host failed: rc={rc}")


_POOL_COLUMNS = (("state", torch.uint8), ("src", torch.int32), ("dst", torch.int32), ("sp", torch.int16),
                 ("dp", torch.int16), ("seq", torch.int32), ("ack", torch.int32), ("expiry", torch.int64))


@dataclass
class PoolTable:
    """A tuple pool (rsk_pool): TcpAckPool's records (vals=True: with seq / ack) or the accepted sockets nobody
    has asked for yet (vals=False), in columns of torch tensors (signed storage of the unsigned C types) plus the
    opaque index.  Shaped like ConnTable: on a device the pool calls of Codec take it, on "cpu" the pool_*_host
    twins below; after any host edit of state or a tuple column call rebuild()."""

    capacity: int
    state: torch.Tensor          # uint8: POOL_LIVE
    src: torch.Tensor
    dst: torch.Tensor
    sp: torch.Tensor
    dp: torch.Tensor
    seq: torch.Tensor | None
    ack: torch.Tensor | None
    expiry: torch.Tensor         # int64 storage of u64
    index: torch.Tensor          # opaque, rsk_conn_index_bytes(capacity, CONN_BY_ID) bytes

    @classmethod
    def alloc(cls, capacity: int, device, vals: bool = True) -> "PoolTable":
        nbytes = lib().rsk_conn_index_bytes(capacity, _abi.CONN_BY_ID)
        if nbytes == 0:
            raise RskError(f"rsk_conn_index_bytes: bad capacity {capacity}")
        cols = {name: torch.zeros(capacity, dtype=dt, device=device) for name, dt in _POOL_COLUMNS}
        if not vals:
            cols["seq"] = cols["ack"] = None
        return cls(capacity=int(capacity), index=torch.full((nbytes // 4,), -1, dtype=torch.int32, device=device), **cols)

    def abi(self) -> _abi.Pool:
        return _abi.Pool(*[_ptr(getattr(self, name)) for name, _ in _POOL_COLUMNS], _ptr(self.index), self.capacity)

    def load(self, **cols) -> "PoolTable":
        """Copy numpy arrays (any integer dtype of the column's width) into the named columns."""
        for name, a in cols.items():
            t = getattr(self, name)
            a = np.ascontiguousarray(a)
            t.copy_(torch.from_numpy(a.view(f"i{a.dtype.itemsize}" if t.dtype != torch.uint8 else np.uint8)))
        return self

    def to(self, device) -> "PoolTable":
        """A copy of every column and of the index on `device` (the index is valid on either side)."""
        mv = lambda t: None if t is None else t.to(device, copy=True)  # noqa: E731
        return PoolTable(self.capacity, *[mv(getattr(self, name)) for name, _ in _POOL_COLUMNS], mv(self.index))

    def column(self, name: str) -> np.ndarray:
        """A column (or the index) on the host as its unsigned C type."""
        a = getattr(self, name).cpu().numpy()
        return a.view(f"u{a.dtype.itemsize}")

    def add_work(self, u_max: int) -> torch.Tensor:
        """The work buffer of pool_add_batch / pool_add_host for at most u_max rows per call (rsk_pool_add_bytes),
        on the pool's device; one per stream that runs the call."""
        nbytes = lib().rsk_pool_add_bytes(u_max, self.capacity)
        if nbytes == 0:
            raise RskError(f"rsk_pool_add_bytes: bad u_max {u_max}")
        return torch.empty(nbytes // 4, dtype=torch.int32, device=self.index.device)

    def settle_work(self, sock: "PoolTable") -> torch.Tensor:
        """The work buffer of pool_settle_batch / pool_settle_host for this ack pool and the socket pool `sock`
        (rsk_pool_settle_bytes), on the pool's device; one per stream that runs the call."""
        nbytes = lib().rsk_pool_settle_bytes(self.capacity, sock.capacity)
        if nbytes == 0:
            raise RskError("rsk_pool_settle_bytes: bad capacity")
        return torch.empty(nbytes // 4, dtype=torch.int32, device=self.index.device)

    def rebuild(self, codec: "Codec | None" = None, stream=None, n_dup: torch.Tensor | None = None) -> None:
        """rsk_pool_index_build on `stream` (a device pool, with its Codec), or the host twin (a "cpu" pool,
        codec None).  n_dup [1] receives the LIVE rows that lost their tuple to a lower row."""
        if (codec is None) != (self.index.device.type == "cpu"):
            raise RskError("PoolTable.rebuild: a device pool takes its Codec, a cpu pool none")
        if codec is None:
            _check(lib().rsk_pool_index_build_host(ctypes.byref(self.abi()), _ptr(n_dup), 1), "rsk_pool_index_build_host")
        else:
            _check(lib().rsk_pool_index_build(codec._ctx, ctypes.byref(self.abi()), _ptr(n_dup), _stream(stream)),
                   "rsk_pool_index_build")


def _pool_add_structs(src, dst, sp, dp, expiry, u_max, work, seq, ack, parse_status, touch, row, new_rows, new_first,
                      n_new, n_again, n_full, n_zero_port):
    cin = _abi.PoolAddIn(_addr(src), _addr(dst), _addr(sp), _addr(dp), _addr(seq), _addr(ack), _addr(parse_status),
                         int(expiry) & 0xFFFFFFFFFFFFFFFF, int(u_max), _abi.POOL_TOUCH if touch else 0, _addr(work))
    cout = _abi.PoolAddOut(_addr(row), _addr(new_rows), _addr(new_first), _addr(n_new), _addr(n_again), _addr(n_full),
                           _addr(n_zero_port))
    return cin, cout


def _pool_offers_struct(offers: ConnOffers, offer_ack_row, offer_sock_row, n_over):
    m = len(offers.src) if offers.m_max is None else int(offers.m_max)
    return _abi.PoolOffersOut(_addr(offers.src), _addr(offers.dst), _addr(offers.sp), _addr(offers.dp), _addr(offers.ack),
                              _addr(offers.flag), _addr(offers.conn_key), _addr(offers.n_offer), _addr(offer_ack_row),
                              _addr(offer_sock_row), _addr(n_over), m)


def _pool_settle_structs(new_offer, n_new, offer_ack_row, offer_sock_row, m_max, miss, src, dst, sp, dp, work, new_max,
                         taken_sock_rows, closed_sock_rows, n_closed, n_purged_ack):
    if new_max is None:
        new_max = 0 if new_offer is None else len(new_offer)
    if m_max is None:
        m_max = max(1, 0 if offer_ack_row is None else len(offer_ack_row))
    cin = _abi.PoolSettleIn(_addr(new_offer), _addr(n_new), _addr(offer_ack_row), _addr(offer_sock_row), int(new_max),
                            int(m_max), _addr(miss), _addr(src), _addr(dst), _addr(sp), _addr(dp), _addr(work))
    cout = _abi.PoolSettleOut(_addr(taken_sock_rows), _addr(closed_sock_rows), _addr(n_closed), _addr(n_purged_ack))
    return (0 if miss is None else len(miss)), cin, cout


def pool_add_host(pool: PoolTable, src, dst, sp, dp, expiry: int, u_max: int, work, seq=None, ack=None,
                  parse_status=None, touch: bool = False, row=None, new_rows=None, new_first=None, n_new=None,
                  n_again=None, n_full=None, n_zero_port=None, nthreads: int = 1) -> None:
    """rsk_pool_add_host on a "cpu" PoolTable (no GPU); the arguments of Codec.pool_add_batch."""
    cin, cout = _pool_add_structs(src, dst, sp, dp, expiry, u_max, work, seq, ack, parse_status, touch, row, new_rows,
                                  new_first, n_new, n_again, n_full, n_zero_port)
    rc = lib().rsk_pool_add_host(ctypes.byref(pool.abi()), len(src), ctypes.byref(cin), ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_pool_add_host failed: rc={rc}")


def pool_offers_host(ack_pool: PoolTable, sock_pool: PoolTable, offers: ConnOffers, offer_ack_row=None,
                     offer_sock_row=None, n_over=None, nthreads: int = 1) -> None:
    """rsk_pool_offers_host on "cpu" PoolTables (no GPU); the arguments of Codec.pool_offers."""
    out = _pool_offers_struct(offers, offer_ack_row, offer_sock_row, n_over)
    rc = lib().rsk_pool_offers_host(ctypes.byref(ack_pool.abi()), ctypes.byref(sock_pool.abi()), ctypes.byref(out), nthreads)
    if rc != 0:
        raise RskError(f"rsk_pool_offers_host failed: rc={rc}")


def pool_settle_host(ack_pool: PoolTable, sock_pool: PoolTable, work, new_offer=None, n_new=None, offer_ack_row=None,
                     offer_sock_row=None, m_max: int | None = None, miss=None, src=None, dst=None, sp=None, dp=None,
                     new_max: int | None = None, taken_sock_rows=None, closed_sock_rows=None, n_closed=None,
                     n_purged_ack=None, nthreads: int = 1) -> None:
    """rsk_pool_settle_host on "cpu" PoolTables (no GPU); the arguments of Codec.pool_settle_batch."""
    n, cin, cout = _pool_settle_structs(new_offer, n_new, offer_ack_row, offer_sock_row, m_max, miss, src, dst, sp, dp,
                                        work, new_max, taken_sock_rows, closed_sock_rows, n_closed, n_purged_ack)
    rc = lib().rsk_pool_settle_host(ctypes.byref(ack_pool.abi()), ctypes.byref(sock_pool.abi()), n, ctypes.byref(cin),
                                    ctypes.byref(cout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_pool_settle_host failed: rc={rc}")


def pool_flush_host(pool: PoolTable, now_ms: int, dead_rows=None, n_dead=None, nthreads: int = 1) -> None:
    """rsk_pool_flush_host on a "cpu" PoolTable (no GPU); the arguments of Codec.pool_flush."""
    fout = _abi.PoolFlushOut(_addr(dead_rows), _addr(n_dead))
    rc = lib().rsk_pool_flush_host(ctypes.byref(pool.abi()), int(now_ms) & 0xFFFFFFFFFFFFFFFF, ctypes.byref(fout), nthreads)
    if rc != 0:
        raise RskError(f"rsk_pool_flush_host failed: rc={rc}")


@dataclass
class TcpInfoBuffers:
    """SoA TcpInfo outputs of RawTcp::RawInput for n captured packets (rsk_tcpinfo_out)."""

    src: torch.Tensor
    dst: torch.Tensor
    sp: torch.Tensor
    dp: torch.Tensor
    seq: torch.Tensor
    ack: torch.Tensor
    flag: torch.Tensor
    parse_status: torch.Tensor
    cap_pay_off: torch.Tensor
    cap_pay_len: torch.Tensor

    @classmethod
    def alloc(cls, n: int, device) -> "TcpInfoBuffers":
        e = lambda dt: torch.empty(n, dtype=dt, device=device)  # noqa: E731
        return cls(
            src=e(torch.int32), dst=e(torch.int32), sp=e(torch.int16), dp=e(torch.int16),
            seq=e(torch.int32), ack=e(torch.int32), flag=e(torch.uint8),
            parse_status=e(torch.int8), cap_pay_off=e(torch.int16), cap_pay_len=e(torch.int16),
        )

    def abi(self) -> _abi.TcpInfoOut:
        return _abi.TcpInfoOut(*[_ptr(getattr(self, f.name)) for f in fields(self)])

    def to_host(self) -> dict:
        return {f.name: getattr(self, f.name).cpu().numpy() for f in fields(self)}


TAG_MODES = {"md5": _abi.TAG_MD5, "table": _abi.TAG_TABLE}


class Codec:
    """One rsk_ctx: a hash key bound to a HIP device.  ``tag_mode`` "md5" (default: the MD5
    compression per packet, as util/rhash.cpp:20-41 computes it) or "table" (the key's 256 tags
    looked up; identical outputs), see rsk_set_tag_mode."""

    def __init__(self, key: bytes = b"hello135", device: int = 0, tag_mode: str = "md5"):
        self.key = bytes(key)
        self.device = int(device)
        self._ctx = lib().rsk_create(self.key, len(self.key), self.device)
        if not self._ctx:
            raise RskError(f"rsk_create failed: {lib().rsk_last_error().decode()}")
        self.set_tag_mode(tag_mode)

    def set_tag_mode(self, mode) -> None:
        """rsk_set_tag_mode: "md5" / "table" (or the RSK_TAG_* value)."""
        m = TAG_MODES[mode] if isinstance(mode, str) else int(mode)
        _check(lib().rsk_set_tag_mode(self._ctx, m), "rsk_set_tag_mode")

    @property
    def tag_mode(self) -> str:
        m = lib().rsk_get_tag_mode(self._ctx)
        return {v: k for k, v in TAG_MODES.items()}.get(m, str(m))

    def close(self) -> None:
        if self._ctx:
            lib().rsk_destroy(self._ctx)
            self._ctx = None

    def __del__(self):  # pragma: no cover - interpreter shutdown order
        try:
            self.close()
        except Exception:
            pass

    def set_encode_path(self, path: int) -> None:
        """rsk_set_encode_path for output_batch: 0 = chosen per call from the last sampled batch's mean
        payload (default), 1 = the per-set kernel k_encode, 2 = the two-pass form for long frames
        (k_encode_heads, then k_encode_copy: 1 / 2 / 4 packets per wave, set_copy_k), 3 = the short-frame
        kernel (k_encode with every set on the flat chunk list).  Every path gives identical bytes."""
        _check(lib().rsk_set_encode_path(self._ctx, path), "rsk_set_encode_path")

    @property
    def last_encode_path(self) -> int:
        """The path the last output_batch took (1 .. 3 as set_encode_path; 0 before any)."""
        fn = lib().rsk__last_encode_path
        fn.argtypes = [ctypes.c_void_p]
        return int(fn(self._ctx))

    @property
    def last_copy_k(self) -> int:
        """Packets per copy wave of the last two-pass output_batch (1, 2, 4; -1: the output-stationary copy;
        0 before any)."""
        fn = lib().rsk__last_copy_k
        fn.argtypes = [ctypes.c_void_p]
        return int(fn(self._ctx))

    def set_copy_k(self, k: int = 0) -> None:
        """Internal knob of the two-pass encode (rsk__set_copy_k): packets per copy wave (1, 2, 4), or -1 for the
        output-stationary copy (k_encode_os: waves own 1-KB blocks of the frame arena, for frames laid back to
        back); 0 = chosen from the last sampled statistic: output-stationary when the sampled frames lie back
        to back, else 4 below a mean payload of 880 B, 2 below 1160 B, 1 above (rsk_kernels.hip kAutoK*)."""
        fn = lib().rsk__set_copy_k
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _check(fn(self._ctx, k), "rsk__set_copy_k")

    def set_two_pass_chunk(self, packets: int = 0) -> None:
        """Internal knob of the two-pass encode (rsk__set_two_pass_chunk): header pass then copy per chunk
        of `packets` (0 = the whole batch)."""
        fn = lib().rsk__set_two_pass_chunk
        fn.argtypes = [ctypes.c_void_p, ctypes.c_uint32]
        _check(fn(self._ctx, packets), "rsk__set_two_pass_chunk")

    def set_send_seq_groupby(self, v: int) -> None:
        """Internal knob for rsk_tcp_send_seq_batch: 0 the per-tile table path when n_conn < 2048
        (default), 1 the demux group-by path for every n_conn, 2 the table path with the one-kernel
        column scan (parity tests and A/B)."""
        fn = lib().rsk__set_send_seq_groupby
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int]
        _check(fn(self._ctx, v), "rsk__set_send_seq_groupby")

    def check_device_errors(self) -> int:
        """rsk_check_device_errors: waits for the device, returns the sticky RSK_DEVERR_* flags (and
        clears them); raises RskError when any is set (that call's compaction / demux outputs were
        wrong; the look-back state is re-initialised at the next call)."""
        f = ctypes.c_uint32(0)
        rc = lib().rsk_check_device_errors(self._ctx, ctypes.byref(f))
        if rc != 0:
            raise RskError(f"device error flags 0x{f.value:x}: {lib().rsk_last_error().decode()}")
        return f.value

    def forget_captures(self) -> None:
        """rsk_forget_captures: the graphs that captured this context's calls are gone, so
        check_device_errors waits for the context's streams again, not the whole device."""
        _check(lib().rsk_forget_captures(self._ctx), "rsk_forget_captures")

    def release_stream(self, stream=None) -> None:
        """rsk_release_stream: wait for `stream` and free its scratch."""
        _check(lib().rsk_release_stream(self._ctx, _stream(stream)), "rsk_release_stream")

    def reserve(self, n_max: int, stream=None) -> None:
        """Pre-size the compaction and delivery scratch of `stream` (default: torch's current stream)."""
        _check(lib().rsk_reserve_stream(self._ctx, n_max, _stream(stream)), "rsk_reserve_stream")

    # ---- batch paths ---------------------------------------------------------------------
    def output_batch(self, payload, pay_off, pay_len, cmd, conv, conn_key, frame, frame_off, status,
                     id=None, id_uniform: bytes = b"\0" * 8, pad16: bool = False, pad128: bool = False,
                     stream=None) -> None:
        """RConn::Output framing for n packets (rsk_encode_batch).  pad16 / pad128 set
        RSK_ENC_ZERO_PAD16 / RSK_ENC_ZERO_PAD128."""
        n = pay_len.numel()
        ein = _abi.EncodeIn(_ptr(payload), _ptr(pay_off), _ptr(pay_len), _ptr(cmd), _ptr(conv),
                            _ptr(conn_key), _ptr(id),
                            (ctypes.c_uint8 * 8)(*bytes(id_uniform)[:8].ljust(8, b"\0")))
        eout = _abi.EncodeOut(_ptr(frame), _ptr(frame_off), _ptr(status),
                              (_abi.ENC_ZERO_PAD16 if pad16 else 0) | (_abi.ENC_ZERO_PAD128 if pad128 else 0))
        _check(lib().rsk_encode_batch(self._ctx, n, ctypes.byref(ein), ctypes.byref(eout),
                                      _stream(stream)), "rsk_encode_batch")

    def output_wire_batch(self, payload, pay_off, pay_len, cmd, conv, conn_key, src, dst, sp, dp, seq, ack, flag,
                          ip_id, wire, wire_off, status, eth: bytes | None = None, id=None,
                          id_uniform: bytes = b"\0" * 8, pad16: bool = False, pad128: bool = False,
                          stream=None) -> None:
        """RConn::Output + RawTcp::SendRawTcp (libnet IPv4/TCP build with checksums) for n packets
        (rsk_encode_wire_batch).  eth=None: LIBNET_RAW4 layout; else a 14-byte link header.  pad16 /
        pad128 set RSK_ENC_ZERO_PAD16 / RSK_ENC_ZERO_PAD128."""
        n = pay_len.numel()
        ein = _abi.EncodeIn(_ptr(payload), _ptr(pay_off), _ptr(pay_len), _ptr(cmd), _ptr(conv),
                            _ptr(conn_key), _ptr(id),
                            (ctypes.c_uint8 * 8)(*bytes(id_uniform)[:8].ljust(8, b"\0")))
        win = _abi.WireIn(_ptr(src), _ptr(dst), _ptr(sp), _ptr(dp), _ptr(seq), _ptr(ack), _ptr(flag), _ptr(ip_id),
                          (ctypes.c_uint8 * 14)(*(bytes(eth or b"")[:14].ljust(14, b"\0"))), 1 if eth else 0)
        eout = _abi.EncodeOut(_ptr(wire), _ptr(wire_off), _ptr(status),
                              (_abi.ENC_ZERO_PAD16 if pad16 else 0) | (_abi.ENC_ZERO_PAD128 if pad128 else 0))
        _check(lib().rsk_encode_wire_batch(self._ctx, n, ctypes.byref(ein), ctypes.byref(win), ctypes.byref(eout),
                                           _stream(stream)), "rsk_encode_wire_batch")

    def onrecv_batch(self, frame, frame_off, frame_len, out: DecodeBuffers, is_tcp_close=None,
                     compact: bool = True, stream=None) -> None:
        """RConn::OnRecv for n frames (rsk_decode_batch)."""
        n = frame_len.numel()
        dout = out.abi(compact)
        _check(lib().rsk_decode_batch(self._ctx, n, _ptr(frame), _ptr(frame_off), _ptr(frame_len),
                                      _ptr(is_tcp_close), ctypes.byref(dout), _stream(stream)),
               "rsk_decode_batch")

    def rawinput_batch(self, cap, cap_off, wire_len, cap_len, datalink: int, flags: int,
                       tcp: TcpInfoBuffers, out: DecodeBuffers, compact: bool = True,
                       stream=None) -> None:
        """RawTcp::RawInput -> cap2uv -> RConn::OnRecv for n captured packets."""
        n = wire_len.numel()
        tout = tcp.abi()
        dout = out.abi(compact)
        _check(lib().rsk_parse_decode_batch(self._ctx, n, _ptr(cap), _ptr(cap_off), _ptr(wire_len),
                                            _ptr(cap_len), datalink, flags, ctypes.byref(tout),
                                            ctypes.byref(dout), _stream(stream)),
               "rsk_parse_decode_batch")

    def syncinput_batch(self, rec, rec_off, nread, tcp: TcpInfoBuffers, out: DecodeBuffers, compact: bool = True,
                        stream=None) -> None:
        """RawTcp::syncInput -> TcpInfo::Decode -> RConn::OnRecv for n hand-off records (21-B TcpInfo
        + frame, nread[i] bytes at rec + rec_off[i])."""
        n = nread.numel()
        tout = tcp.abi()
        dout = out.abi(compact)
        _check(lib().rsk_syncinput_decode_batch(self._ctx, n, _ptr(rec), _ptr(rec_off), _ptr(nread),
                                                ctypes.byref(tout), ctypes.byref(dout), _stream(stream)),
               "rsk_syncinput_decode_batch")

    def rawinput_slots_batch(self, slots, slot: int, wire_len, cap_len, datalink: int, flags: int,
                             tcp: TcpInfoBuffers, out: DecodeBuffers, compact: bool = True, stream=None) -> None:
        """rawinput_batch on host-staged header slots (rsk_parse_decode_slots_batch): packet i's first
        min(cap_len, slot) bytes at slots[slot * i:]; RSK_PARSE_SLOT_SHORT marks packets to resubmit whole."""
        n = wire_len.numel()
        tout = tcp.abi()
        dout = out.abi(compact)
        _check(lib().rsk_parse_decode_slots_batch(self._ctx, n, _ptr(slots), slot, _ptr(wire_len), _ptr(cap_len),
                                                  datalink, flags, ctypes.byref(tout), ctypes.byref(dout),
                                                  _stream(stream)), "rsk_parse_decode_slots_batch")

    def tcp_send_seq_batch(self, conn, status, conn_seq, ip_id_next, seq, ip_id, stream=None) -> None:
        """FakeTcp::Output's seq advance + RawTcp::Output's mIpId++ for a batch sent in order
        (rsk_tcp_send_seq_batch); conn_seq / ip_id_next are device state updated in place."""
        n = conn.numel()
        _check(lib().rsk_tcp_send_seq_batch(self._ctx, n, _ptr(conn), _ptr(status), conn_seq.numel(), _ptr(conn_seq),
                                            _ptr(ip_id_next), _ptr(seq), _ptr(ip_id), _stream(stream)),
               "rsk_tcp_send_seq_batch")

    def tcp_recv_ack_batch(self, conn, delivered, seq, conn_ack, stream=None) -> None:
        """FakeTcp::OnRecv's ack update over a batch (rsk_tcp_recv_ack_batch)."""
        n = conn.numel()
        _check(lib().rsk_tcp_recv_ack_batch(self._ctx, n, _ptr(conn), _ptr(delivered), _ptr(seq), conn_ack.numel(),
                                            _ptr(conn_ack), _stream(stream)), "rsk_tcp_recv_ack_batch")

    def tcpinfo_encode_batch(self, src, dst, sp, dp, seq, ack, flag, rec, stream=None) -> None:
        n = src.numel()
        _check(lib().rsk_tcpinfo_encode_batch(self._ctx, n, _ptr(src), _ptr(dst), _ptr(sp), _ptr(dp),
                                              _ptr(seq), _ptr(ack), _ptr(flag), _ptr(rec),
                                              _stream(stream)), "rsk_tcpinfo_encode_batch")

    def output_headers_batch(self, first_byte, pay_len, cmd, conv, conn_key, hdr, status, id=None,
                             id_uniform: bytes = b"\0" * 8, stream=None) -> None:
        """Header-only RConn::Output (rsk_encode_headers_batch): hdr[32 i:32 i+32] = frame bytes [0, 32)."""
        n = pay_len.numel()
        ein = _abi.EncodeHdrIn(_ptr(first_byte), _ptr(pay_len), _ptr(cmd), _ptr(conv), _ptr(conn_key), _ptr(id),
                               (ctypes.c_uint8 * 8)(*bytes(id_uniform)[:8].ljust(8, b"\0")))
        _check(lib().rsk_encode_headers_batch(self._ctx, n, ctypes.byref(ein), _ptr(hdr), _ptr(status),
                                              _stream(stream)), "rsk_encode_headers_batch")

    def onrecv_headers_batch(self, hdr, frame_len, out: DecodeBuffers, is_tcp_close=None, stream=None) -> None:
        """Header-only RConn::OnRecv (rsk_decode_headers_batch) on 32-B slots (stage_decode_headers)."""
        n = frame_len.numel()
        _check(lib().rsk_decode_headers_batch(self._ctx, n, _ptr(hdr), _ptr(frame_len), _ptr(is_tcp_close),
                                              ctypes.byref(out.abi()), _stream(stream)),
               "rsk_decode_headers_batch")

    def filter_rawinput_batch(self, cap, cap_off, wire_len, cap_len, datalink: int, flags: int,
                              filt: "_abi.CaptureFilter", match, tcp: TcpInfoBuffers, out: DecodeBuffers,
                              compact: bool = True, stream=None) -> None:
        """Capture filter + RawTcp::RawInput + RConn::OnRecv in one pass (rsk_filter_parse_decode_batch)."""
        n = wire_len.numel()
        tout = tcp.abi()
        dout = out.abi(compact)
        _check(lib().rsk_filter_parse_decode_batch(self._ctx, n, _ptr(cap), _ptr(cap_off), _ptr(wire_len),
                                                   _ptr(cap_len), datalink, flags, ctypes.byref(filt), _ptr(match),
                                                   ctypes.byref(tout), ctypes.byref(dout), _stream(stream)),
               "rsk_filter_parse_decode_batch")

    def capture_filter_batch(self, cap, cap_off, cap_len, datalink: int, filt: "_abi.CaptureFilter", match,
                             match_idx=None, n_match=None, stream=None) -> None:
        """The capture filter RCap installs (rsk_capture_filter_batch) over a batch."""
        n = cap_off.numel()
        _check(lib().rsk_capture_filter_batch(self._ctx, n, _ptr(cap), _ptr(cap_off), _ptr(cap_len), datalink,
                                              ctypes.byref(filt), _ptr(match), _ptr(match_idx), _ptr(n_match),
                                              _stream(stream)), "rsk_capture_filter_batch")

    def demux_batch(self, status, cmd, fields: int, out: "DemuxBuffers", id=None, conv=None, conn_key=None,
                    dst=None, stream=None) -> None:
        """Stable group-by of the VALID packets on `fields` (rsk_demux_batch):
        segment s = out.perm[out.seg_off[s]:out.seg_off[s + 1]], keyed by packet out.seg_first[s]."""
        n = status.numel()
        din = _abi.DemuxIn(_ptr(status), _ptr(cmd), _ptr(id), _ptr(conv), _ptr(conn_key), _ptr(dst))
        _check(lib().rsk_demux_batch(self._ctx, n, ctypes.byref(din), fields, ctypes.byref(out.abi()),
                                     _stream(stream)), "rsk_demux_batch")

    def deliver_batch(self, arena, base_off, pay_off, pay_len, status, out: "DeliverBuffers", inner_off=None,
                      order=None, n_order=None, align: int = 1, plan_only: bool = False, stream=None) -> None:
        """The consumers' per-packet payload copy (SConn::OnRecv, server/SConn.cpp:77-89), batched
        (rsk_deliver_batch): the VALID payloads at arena + base_off + inner_off + pay_off packed into
        out.arena in `order` (a demux's perm with its n_valid, a decode's valid_idx with its n_valid, or
        None = packet order), payload k at out.out_off[k], each rounded up to `align`; out.total is the
        bytes needed, to compare with out.cap.  plan_only (or an `out` without an arena) writes the
        offsets and the total only."""
        n = status.numel()
        din = _abi.DeliverIn(_ptr(arena), _ptr(base_off), _ptr(inner_off), _ptr(pay_off), _ptr(pay_len),
                             _ptr(status), _ptr(order), _ptr(n_order))
        dout = out.abi(align, plan_only)
        _check(lib().rsk_deliver_batch(self._ctx, n, ctypes.byref(din), ctypes.byref(dout), _stream(stream)),
               "rsk_deliver_batch")

    def verify_wire_batch(self, cap, cap_off, cap_len, datalink: int, csum, status=None, status_out=None,
                          n_bad=None, stream=None) -> None:
        """IPv4 header and TCP checksum check of n captured packets (rsk_verify_wire_batch): csum[i]
        gets the CSUM_* bits of packet i (cap_len[i] bytes at cap + cap_off[i]; datalink DLT_EN10MB,
        DLT_NULL or DLT_RAW).  With `status` (a decode's status) only the RECV_VALID packets are
        examined; status_out (may be `status` itself) gets the status with the bad packets set to
        RECV_DROP, n_bad [1] their number."""
        n = cap_len.numel()
        vin = _abi.VerifyIn(_ptr(cap), _ptr(cap_off), _ptr(cap_len), _ptr(status))
        vout = _abi.VerifyOut(_ptr(csum), _ptr(status_out), _ptr(n_bad))
        _check(lib().rsk_verify_wire_batch(self._ctx, n, ctypes.byref(vin), datalink, ctypes.byref(vout),
                                           _stream(stream)), "rsk_verify_wire_batch")

    def conn_index_build(self, tab: "ConnTable", n_dup=None, stream=None) -> None:
        """rsk_conn_index_build: rebuild tab.index from its state, conn_key (and id) columns; n_dup [1]
        gets the LIVE rows that lost their key to a lower row."""
        _check(lib().rsk_conn_index_build(self._ctx, ctypes.byref(tab.abi()), _ptr(n_dup), _stream(stream)),
               "rsk_conn_index_build")

    def conn_pick_build(self, tab: "ConnTable", counts=None, stream=None) -> None:
        """rsk_conn_pick_build: rebuild tab.pick from its state (and id) columns; counts [2] gets the groups
        that have a candidate and the candidates."""
        _check(lib().rsk_conn_pick_build(self._ctx, ctypes.byref(tab.abi()), _ptr(tab.pick), _ptr(counts),
                                         _stream(stream)), "rsk_conn_pick_build")

    def conn_pick_batch(self, tab: "ConnTable", conn, len=None, id=None, avoid_key=None, draw=None, seed: int = 0,
                        n_none=None, used=None, stream=None) -> None:
        """INetGroup::doSend's pick for conn.numel() packets to send (rsk_conn_pick_batch): conn[i] = a
        LIVE | ALIVE row of packet i's group (all rows; with a by_id table the rows of id[i]) chosen by
        draw[i] (None: the splitmix64 stream of `seed`), never the row of avoid_key[i]; CONN_NONE for a
        packet with len[i] <= 0 and, counted in n_none [1], for one whose group has no such row.  used
        [capacity] gets 1 at every picked row.  The table is seen as rebuild_pick last saw it."""
        n = conn.numel()
        pin = _abi.ConnPickIn(_ptr(len), _ptr(id), _ptr(avoid_key), _ptr(draw), seed & 0xFFFFFFFFFFFFFFFF)
        pout = _abi.ConnPickOut(_ptr(conn), _ptr(n_none), _ptr(used))
        _check(lib().rsk_conn_pick_batch(self._ctx, ctypes.byref(tab.abi()), _ptr(tab.pick), n, ctypes.byref(pin),
                                         ctypes.byref(pout), _stream(stream)), "rsk_conn_pick_batch")

    def conn_resolve_batch(self, tab: "ConnTable", status, conn_key, conn, cmd=None, id=None, hit=None, miss=None,
                           n_miss=None, stream=None) -> None:
        """INetGroup::Input's lookup for n decoded packets (rsk_conn_resolve_batch): conn[i] = the row of
        packet i's connKey (with a by_id table: of its (IdBuf, connKey)) or CONN_NONE; looked up iff
        status[i] == RECV_VALID and cmd[i] == CMD_DATA (cmd None: all DATA).  hit[i] = 1 iff found (the
        `delivered` of tcp_recv_ack_batch); miss is a status column of the looked-up packets that were not
        found (feed it to demux_batch for the distinct missing keys), n_miss [1] their number."""
        n = status.numel()
        rin = _abi.ConnResolveIn(_ptr(status), _ptr(cmd), _ptr(id), _ptr(conn_key))
        rout = _abi.ConnResolveOut(_ptr(conn), _ptr(hit), _ptr(miss), _ptr(n_miss))
        _check(lib().rsk_conn_resolve_batch(self._ctx, ctypes.byref(tab.abi()), n, ctypes.byref(rin),
                                            ctypes.byref(rout), _stream(stream)), "rsk_conn_resolve_batch")

    def conn_expand_batch(self, tab: "ConnTable", conn, ok, src=None, dst=None, sp=None, dp=None, ack=None, flag=None,
                          conn_key=None, id=None, n_bad=None, stream=None) -> None:
        """INetConn::Output's TcpInfo for n packets to send (rsk_conn_expand_batch): every given column gets
        row conn[i]'s value -- the columns output_wire_batch takes -- or zero with ok[i] = 0 when the row is
        out of range or not LIVE | ALIVE; n_bad [1] counts those."""
        n = conn.numel()
        eout = _abi.ConnExpandOut(_ptr(src), _ptr(dst), _ptr(sp), _ptr(dp), _ptr(ack), _ptr(flag), _ptr(conn_key),
                                  _ptr(id), _ptr(ok), _ptr(n_bad))
        _check(lib().rsk_conn_expand_batch(self._ctx, ctypes.byref(tab.abi()), n, _ptr(conn), ctypes.byref(eout),
                                           _stream(stream)), "rsk_conn_expand_batch")

    def control_batch(self, tab: "ConnTable", status, cmd, pay_off, pay_len, arena, base_off, out: "ControlBuffers",
                      id=None, conn_key=None, inner_off=None, tcp_sp=None, tcp_dp=None, miss=None, ka_tries=None,
                      stream=None) -> None:
        """The control branches of IAppGroup::Input, ConnReset::Input, NetConnKeepAlive::Input and
        IAppGroup::ProcessTcpFinOrRst for n decoded packets (rsk_control_batch): out.kind[i] = CTL_*,
        out.arg[i] = the key (or conv) in the body at arena + base_off + inner_off + pay_off, out.conn[i]
        = its LIVE row in `tab` or CONN_NONE.  out.rst_first[r] = the first packet that resets row r;
        ka_tries[r] (the column keepalive_flush keeps) is cleared by a KEEP_ALIVE_RESP for r.  The
        messages to send -- a KEEP_ALIVE_RESP or a NETCONN_RST per KEEP_ALIVE_REQ and, with `miss` (the
        resolve's) and conn_key, a NETCONN_RST per missed DATA packet -- land in out.msg_* in packet
        order, out.n_msg of them.  tcp_sp / tcp_dp (the parse's ports) make the RECV_CLOSE packets of a
        table without by_id CTL_TCP_CLOSE.  Lookups see the table as last indexed."""
        cin = _control_in(status, cmd, pay_off, pay_len, arena, base_off, id, conn_key, inner_off, tcp_sp, tcp_dp, miss)
        _check(lib().rsk_control_batch(self._ctx, ctypes.byref(tab.abi()), status.numel(), ctypes.byref(cin),
                                       ctypes.byref(out.abi_control(ka_tries)), _stream(stream)), "rsk_control_batch")

    def keepalive_flush(self, tab: "ConnTable", ka_tries, established_ms, now_ms: int, out: "ControlBuffers",
                        request_delay_ms: int = _abi.KA_REQUEST_DELAY_MS, max_retry: int = _abi.KA_MAX_RETRY,
                        online: bool = True, stream=None) -> None:
        """NetConnKeepAlive::OnFlush as one pass over the rows of `tab` (rsk_keepalive_flush): ka_tries
        [capacity] (uint8, KA_NONE = no pending request) is advanced in place, the KEEP_ALIVE_REQ messages
        land in out.msg_* in row order (out.n_msg), the rows that timed out in out.dead_rows
        (out.n_dead).  established_ms [capacity] and now_ms are milliseconds; a row with CONN_NEW set, or
        younger than request_delay_ms, sends nothing; online False only purges the rows that are not LIVE."""
        ka = _abi.Keepalive(_addr(ka_tries), _addr(established_ms), now_ms, request_delay_ms, max_retry, int(online))
        _check(lib().rsk_keepalive_flush(self._ctx, ctypes.byref(tab.abi()), ctypes.byref(ka),
                                         ctypes.byref(out.abi_flush()), _stream(stream)), "rsk_keepalive_flush")

    def conv_index_build(self, tab: "ConvTable", n_dup=None, stream=None) -> None:
        """rsk_conv_index_build: rebuild tab.index from its state, conv (dst, id) columns; n_dup [1] gets
        the LIVE rows that lost their key to a lower row."""
        _check(lib().rsk_conv_index_build(self._ctx, ctypes.byref(tab.abi()), _ptr(n_dup), _stream(stream)),
               "rsk_conv_index_build")

    def conv_resolve_batch(self, tab: "ConvTable", status, conv, conv_row, cmd=None, hit=None, id=None, dst=None,
                           ctl_kind=None, ctl_arg=None, unknown=None, n_unknown=None, rst_first=None,
                           msgs: "ControlBuffers | None" = None, stream=None) -> None:
        """SubGroup::OnRecv's / ClientGroup::OnRecv's lookup for n decoded packets (rsk_conv_resolve_batch):
        conv_row[i] = the LIVE row of packet i's (id, dst, conv) -- each part only with the table's flag --
        or CONN_NONE; examined iff status[i] == RECV_VALID, cmd[i] == CMD_DATA (cmd None: all DATA) and
        hit[i] (the conn resolve's; None: all).  Every examined packet that found its row adds 1 to
        tab.cur_in[row], exactly, whatever the skew.  With ctl_kind / ctl_arg (control_batch's kind / arg)
        a CTL_CONV_RST packet is looked up by the conv in its body on a by_dst table; rst_first
        [capacity] gets the first such packet per row.  unknown is a status column of the examined
        packets that found no row (feed it to demux_batch for the distinct new keys), n_unknown [1]
        their number; with msgs (a ControlBuffers) one CONV_RST message per unknown packet lands in
        msgs.msg_* in packet order, msgs.n_msg of them.  Lookups see the table as last indexed."""
        cin, cout = _conv_resolve_structs(status, conv, conv_row, cmd, hit, id, dst, ctl_kind, ctl_arg, unknown,
                                          n_unknown, rst_first, msgs)
        _check(lib().rsk_conv_resolve_batch(self._ctx, ctypes.byref(tab.abi()), status.numel(), ctypes.byref(cin),
                                            ctypes.byref(cout), _stream(stream)), "rsk_conv_resolve_batch")

    def conv_create_batch(self, tab: "ConvTable", conv, conv_row, unknown, u_max: int, work, id=None, dst=None,
                          n_unknown=None, new_rows=None, new_first=None, n_new=None, n_full=None, stream=None) -> None:
        """SubGroup::newConn for the convs born in a batch, on the device table (rsk_conv_create_batch), after
        conv_resolve_batch left conv_row and unknown: the distinct keys of the first u_max unknown packets
        take the vacant rows in first-arrival order (new_rows[j], new_first[j], j < n_new; n_full keys got
        none), the rows go into tab.index in place, and every unknown packet whose key now resolves gets
        its conv_row, unknown = RECV_DROP and its count in cur_in.  work = tab.create_work(u_max)."""
        cin, cout = _conv_create_structs(conv, conv_row, unknown, u_max, work, id, dst, n_unknown, new_rows, new_first,
                                         n_new, n_full)
        _check(lib().rsk_conv_create_batch(self._ctx, ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()),
                                           conv_row.numel(), ctypes.byref(cin), ctypes.byref(cout), _stream(stream)),
               "rsk_conv_create_batch")

    def conn_close_batch(self, tab: "ConnTable", work, close_rows=None, n_close=None, m_max: int | None = None,
                         rst_first=None, remove: bool = False, sweep: bool = False, marked_rows=None, n_marked=None,
                         closed_rows=None, n_closed=None, pick: bool = False, pick_counts=None, stream=None) -> None:
        """INetConn::NotifyErr and INetGroup::RemoveConn on the device table (rsk_conn_close_batch).  The marks are
        a list (close_rows / n_close, e.g. keepalive_flush's dead_rows / n_dead; m_max defaults to
        len(close_rows)), a column (rst_first, control_batch's) or none (sweep alone).  A marked LIVE row loses
        CONN_ALIVE (marked_rows / n_marked); with remove it also leaves the table, with sweep every LIVE row
        without ALIVE does (closed_rows / n_closed), and the conn index is rebuilt over the rows that stay.
        pick=True keeps tab.pick current (it must be current for the state the call finds); pick_counts [2] as
        conn_pick_build's counts.  work = tab.close_work(), one per stream.  Captures into a graph after
        reserve(stream=...)."""
        cin, cout = _conn_close_structs(tab, close_rows, n_close, m_max, rst_first, work, remove, sweep, marked_rows,
                                        n_marked, closed_rows, n_closed, pick, pick_counts)
        _check(lib().rsk_conn_close_batch(self._ctx, ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()),
                                          ctypes.byref(cin), ctypes.byref(cout), _stream(stream)), "rsk_conn_close_batch")

    def conn_create_batch(self, tab: "ConnTable", offers: "ConnOffers", work, stream=None, **kw) -> None:
        """INetGroup::Input's miss path -> CreateNetConn -> AddNetConn on the device table (rsk_conn_create_batch).
        Column form, behind conn_resolve_batch: conn, hit, miss, n_miss (the resolve's, continued), the packets'
        conn_key, id (by_id), src, dst, sp, dp and u_max; the distinct keys of the first u_max missing packets
        whose first packet's 4-tuple has an offer take the vacant rows in first-arrival order.  List form
        (list_form=True): the offers carry conn_key (and id) themselves.  Outputs: new_rows / new_first /
        new_offer [min(m_max, capacity)], offer_row [m_max], n_new, n_full, n_refused; repeat=True makes
        offer_row in/out (a consumed offer refuses).  established_ms / ka_tries (with now_ms) are set for the new
        rows when given.  pick=True keeps tab.pick current; pick_counts [2].  work = tab.create_work(u_max,
        m_max), one per stream.  Captures into a graph after reserve(stream=...)."""
        if set(kw) - _CONN_CREATE_KW:
            raise TypeError(f"conn_create_batch: unknown arguments {sorted(set(kw) - _CONN_CREATE_KW)}")
        n, cin, cout = _conn_create_structs(tab, offers, work, kw)
        _check(lib().rsk_conn_create_batch(self._ctx, ctypes.byref(tab.abi()), ctypes.byref(tab.abi_create_rows()), n,
                                           ctypes.byref(cin), ctypes.byref(cout), _stream(stream)),
               "rsk_conn_create_batch")

    conn_create_host = staticmethod(conn_create_host)
    conn_create_bytes = staticmethod(conn_create_bytes)

    def conv_close_batch(self, tab: "ConvTable", close_rows=None, n_close=None, m_max: int | None = None, work=None,
                         rst_first=None, ctl_kind=None, conv_row=None, unknown=None, n_unknown=None, hold: bool = False,
                         closed_rows=None, closed_at=None, n_closed=None, n_reopened=None, n_rst_again=None,
                         stream=None) -> None:
        """IGroup::CloseConn on the device table (rsk_conv_close_batch), in one of two forms.  Timer: close_rows /
        n_close (conv_flush's dead_rows / n_dead; m_max defaults to len(close_rows)) and work = tab.close_work().
        Receive: rst_first and ctl_kind as conv_resolve_batch had them, conv_row (unknown, n_unknown) in/out: the
        rows a CONV_RST hit close, and the packets behind their row's reset go back to NONE -- the DATA ones as
        unknown = RECV_VALID for the next conv_create_batch.  closed_rows / closed_at [capacity] and n_closed list
        what closed; with hold the rows keep LIVE and only the index forgets them until the host clears them."""
        cin, cout = _conv_close_structs(close_rows, n_close, m_max, rst_first, ctl_kind, work, hold, conv_row, unknown,
                                        n_unknown, closed_rows, closed_at, n_closed, n_reopened, n_rst_again)
        n = 0 if conv_row is None else conv_row.numel()
        _check(lib().rsk_conv_close_batch(self._ctx, ctypes.byref(tab.abi()), ctypes.byref(tab.abi_rows()), n,
                                          ctypes.byref(cin), ctypes.byref(cout), _stream(stream)), "rsk_conv_close_batch")

    def conv_send_batch(self, tab: "ConvTable", conv_row, sent=None, conv=None, dst=None, id=None, ok=None, n_bad=None,
                        stream=None) -> None:
        """The send side of the conv table (rsk_conv_send_batch): the given columns conv / dst / id (an
        encode's) get row conv_row[i]'s values, or zero with ok[i] = 0 when the row is out of range or
        not LIVE; n_bad [1] counts those.  With sent (int32, the encode's status) every ok packet with
        sent[i] > 0 adds 1 to tab.cur_out[row].  Expand before the encode (sent None), count after it."""
        sout = _abi.ConvSendOut(_ptr(conv), _ptr(dst), _ptr(id), _ptr(ok), _ptr(n_bad))
        _check(lib().rsk_conv_send_batch(self._ctx, ctypes.byref(tab.abi()), conv_row.numel(), _ptr(conv_row), _ptr(sent),
                                         ctypes.byref(sout), _stream(stream)), "rsk_conv_send_batch")

    def conv_flush(self, tab: "ConvTable", dead_rows=None, n_dead=None, n_alive=None, stream=None) -> None:
        """IGroup::Flush as one pass over the rows of `tab` (rsk_conv_flush): a LIVE row whose alive is 0
        is listed in dead_rows (row order, n_dead [1]); every other LIVE row gets alive = (prev_in !=
        cur_in and prev_out != cur_out) and prev = cur.  n_alive [1] = the LIVE rows alive afterwards."""
        fout = _abi.ConvFlushOut(_ptr(dead_rows), _ptr(n_dead), _ptr(n_alive))
        _check(lib().rsk_conv_flush(self._ctx, ctypes.byref(tab.abi()), ctypes.byref(fout), _stream(stream)),
               "rsk_conv_flush")

    def pool_add_batch(self, pool: "PoolTable", src, dst, sp, dp, expiry: int, u_max: int, work, seq=None, ack=None,
                       parse_status=None, touch: bool = False, row=None, new_rows=None, new_first=None, n_new=None,
                       n_again=None, n_full=None, n_zero_port=None, stream=None) -> None:
        """TcpAckPool::AddInfoFromPeer / ServerNetManager::add2Pool on the device pool (rsk_pool_add_batch): the
        rows with parse_status == PARSE_SYN (every row without parse_status) and both ports, the first u_max of
        them; a tuple in the pool keeps its row (touch: its expiry moves), the new ones take the vacant rows in
        first-arrival order.  work: pool.add_work(u_max)."""
        cin, cout = _pool_add_structs(src, dst, sp, dp, expiry, u_max, work, seq, ack, parse_status, touch, row,
                                      new_rows, new_first, n_new, n_again, n_full, n_zero_port)
        _check(lib().rsk_pool_add_batch(self._ctx, ctypes.byref(pool.abi()), len(src), ctypes.byref(cin),
                                        ctypes.byref(cout), _stream(stream)), "rsk_pool_add_batch")

    def pool_offers(self, ack_pool: "PoolTable", sock_pool: "PoolTable", offers: "ConnOffers", offer_ack_row=None,
                    offer_sock_row=None, n_over=None, stream=None) -> None:
        """The join of the two pools into conn_create_batch's offers (rsk_pool_offers): one offer per record whose
        tuple has a socket, in row order; offers.conn_key, when given, receives key_for_tcp(sp, dp)."""
        out = _pool_offers_struct(offers, offer_ack_row, offer_sock_row, n_over)
        _check(lib().rsk_pool_offers(self._ctx, ctypes.byref(ack_pool.abi()), ctypes.byref(sock_pool.abi()),
                                     ctypes.byref(out), _stream(stream)), "rsk_pool_offers")

    def pool_settle_batch(self, ack_pool: "PoolTable", sock_pool: "PoolTable", work, new_offer=None, n_new=None,
                          offer_ack_row=None, offer_sock_row=None, m_max: int | None = None, miss=None, src=None,
                          dst=None, sp=None, dp=None, new_max: int | None = None, taken_sock_rows=None,
                          closed_sock_rows=None, n_closed=None, n_purged_ack=None, stream=None) -> None:
        """The pools behind a batch (rsk_pool_settle_batch): the rows of the offers that became conns leave, and so
        does what a still-missing packet's tuple has in one pool only.  work: ack_pool.settle_work(sock_pool)."""
        n, cin, cout = _pool_settle_structs(new_offer, n_new, offer_ack_row, offer_sock_row, m_max, miss, src, dst, sp,
                                            dp, work, new_max, taken_sock_rows, closed_sock_rows, n_closed, n_purged_ack)
        _check(lib().rsk_pool_settle_batch(self._ctx, ctypes.byref(ack_pool.abi()), ctypes.byref(sock_pool.abi()), n,
                                           ctypes.byref(cin), ctypes.byref(cout), _stream(stream)), "rsk_pool_settle_batch")

    def pool_flush(self, pool: "PoolTable", now_ms: int, dead_rows=None, n_dead=None, stream=None) -> None:
        """TcpAckPool::OnFlush / ServerNetManager::OnFlush (rsk_pool_flush): the LIVE rows with expiry <= now_ms
        leave; dead_rows [capacity] lists them in row order, n_dead [1] counts them."""
        fout = _abi.PoolFlushOut(_ptr(dead_rows), _ptr(n_dead))
        _check(lib().rsk_pool_flush(self._ctx, ctypes.byref(pool.abi()), int(now_ms) & 0xFFFFFFFFFFFFFFFF,
                                    ctypes.byref(fout), _stream(stream)), "rsk_pool_flush")

    # ---- reference single-call signatures (GPU round trip each) -----------------------------
    def compute_hash(self, data: bytes) -> bytes | None:
        tag = ctypes.create_string_buffer(8)
        r = lib().rsk_compute_hash(self._ctx, tag, bytes(data), len(data))
        return tag.raw if r else None

    def hash_equal(self, tag: bytes, data: bytes) -> bool:
        return bool(lib().rsk_hash_equal(self._ctx, bytes(tag), bytes(data), len(data)))

    def enc2buf(self, cmd: int, id: bytes, conv: int, conn_key: int, buf_len: int = 1492) -> bytes | None:
        buf = ctypes.create_string_buffer(max(buf_len, 23))
        r = lib().rsk_enchead_enc2buf(self._ctx, buf, buf_len, cmd, bytes(id)[:8].ljust(8, b"\0"),
                                      conv & 0xFFFFFFFF, conn_key & 0xFFFFFFFFFFFFFFFF)
        return buf.raw[:23] if r else None

    def decodebuf(self, buf: bytes, buf_len: int | None = None):
        """-> (len, cmd, id, conv, conn_key) or None (EncHead::DecodeBuf returned nullptr)."""
        if buf_len is None:
            buf_len = len(buf)
        b = bytes(buf).ljust(23, b"\0")
        ln, cmd = ctypes.c_uint8(), ctypes.c_uint8()
        idb = ctypes.create_string_buffer(8)
        conv, key = ctypes.c_uint32(), ctypes.c_uint64()
        r = lib().rsk_enchead_decodebuf(self._ctx, b, buf_len, ctypes.byref(ln), ctypes.byref(cmd),
                                        idb, ctypes.byref(conv), ctypes.byref(key))
        if not r:
            return None
        return ln.value, cmd.value, idb.raw, conv.value, key.value


def key_for_tcp(sp: int, dp: int) -> int:
    return lib().rsk_key_for_tcp(sp, dp)


def key_for_udp(sp: int, dp: int) -> int:
    return lib().rsk_key_for_udp(sp, dp)


def fill_splitmix(t: torch.Tensor, seed: int, stream=None) -> None:
    _check(lib().rsk_fill_splitmix(_ptr(t), t.numel() * t.element_size(), seed & (2**64 - 1),
                                   _stream(stream)), "rsk_fill_splitmix")
