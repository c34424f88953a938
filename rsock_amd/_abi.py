"""ctypes mirror of include/rsk_codec.h.

Loads the in-tree ``rsock_amd/librsk.so`` (built by ``__graft_entry__.build()`` /
``make -C rsock_amd``).  There is no fallback: if the library is missing or fails to load, importing
this module raises, so nothing can silently run a non-HIP path.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# RSK_LIB selects another in-tree build of the same library (tools: a saved copy of an earlier build,
# for an A/B between builds in separate processes)
LIB_PATH = os.path.join(_HERE, os.environ.get("RSK_LIB", "librsk.so"))

# ---- constants (include/rsk_codec.h) ------------------------------------------------------------
HASH_BUF_SIZE = 8
ID_BUF_SIZE = 8
ENC_HEAD_SIZE = 23
HEAD_SIZE = 31
MAX_PKT_SIZE = 1500
MAX_PAYLOAD = MAX_PKT_SIZE - HEAD_SIZE
TCPINFO_WIRE_SIZE = 21

CMD_DATA, CMD_CONV_RST, CMD_NETCONN_RST, CMD_KEEP_ALIVE_REQ, CMD_KEEP_ALIVE_RESP = 0, 1, 2, 3, 4
TH_FIN, TH_SYN, TH_RST, TH_PUSH, TH_ACK = 0x01, 0x02, 0x04, 0x08, 0x10
DLT_NULL, DLT_EN10MB = 0, 1
DLT_RAW = 12  # the packet starts at the IPv4 header; rsk_verify_wire_batch only

OK, EINVAL, ENOMEM, EDEVICE = 0, -22, -12, -5
SEND_OVERSIZE, SEND_RESET = -1, 0
MAX_BATCH = 0xFFFF0000
RECV_VALID, RECV_CLOSE, RECV_DROP = 1, 0, -1
PARSE_DROP, PARSE_DELIVER, PARSE_SYN, PARSE_MALFORMED, PARSE_SLOT_SHORT = 0, 1, 2, 3, 4
CAP_SLOT_MIN = 64
PARSE_HAS_ACK_POOL, PARSE_IS_SERVER = 0x1, 0x2
FILTER_MAX_PORTS = 64
TAG_MD5, TAG_TABLE = 0, 1
DEVERR_LOOKBACK = 0x1
DEVERR_TABLE = 0x2
DEMUX_ID, DEMUX_CONN_KEY, DEMUX_CONV, DEMUX_DST, DEMUX_CMD_BARRIER = 0x01, 0x02, 0x04, 0x08, 0x10
DEMUX_GROUP_BARRIER = 0x20
CSUM_IP_CHECKED, CSUM_IP_OK, CSUM_TCP_CHECKED, CSUM_TCP_OK, CSUM_TCP_TRUNC = 0x01, 0x02, 0x04, 0x08, 0x10
VERIFY_MAX_BATCH = 0x1FFFFFE0
CONN_NONE = 0xFFFFFFFF
CONN_MAX_ROWS = 1 << 20
CONN_BY_ID = 0x1
CONN_LIVE, CONN_ALIVE, CONN_NEW = 0x1, 0x2, 0x4
(CTL_NONE, CTL_CONV_RST, CTL_NETCONN_RST, CTL_KA_REQ, CTL_KA_RESP, CTL_TCP_CLOSE, CTL_SHORT,
 CTL_UNKNOWN) = range(8)
KA_NONE = 0xFF
KA_REQUEST_DELAY_MS = 15000
KA_MAX_RETRY = 3
CONV_BY_DST, CONV_BY_ID = 0x1, 0x2
CONV_CLOSE_HOLD = 0x1
CONN_CLOSE_REMOVE, CONN_CLOSE_SWEEP = 0x1, 0x2
CONN_CREATE_LIST, CONN_CREATE_REPEAT = 0x1, 0x2
POOL_LIVE = 0x1
POOL_TOUCH = 0x1

_vp = ctypes.c_void_p
_u8p = ctypes.c_void_p  # all arrays passed as raw addresses


class EncodeIn(ctypes.Structure):
    _fields_ = [
        ("payload_arena", _vp),
        ("pay_off", _vp),
        ("pay_len", _vp),
        ("cmd", _vp),
        ("conv", _vp),
        ("conn_key", _vp),
        ("id", _vp),
        ("id_uniform", ctypes.c_uint8 * 8),
    ]


class EncodeOut(ctypes.Structure):
    _fields_ = [("frame_arena", _vp), ("frame_off", _vp), ("status", _vp), ("flags", ctypes.c_uint32)]


ENC_ZERO_PAD16 = 0x1
ENC_ZERO_PAD128 = 0x2
ENC_PATH_AUTO, ENC_PATH_PER_SET, ENC_PATH_TWO_PASS, ENC_PATH_SHORT = 0, 1, 2, 3


class WireIn(ctypes.Structure):
    _fields_ = [
        ("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("seq", _vp), ("ack", _vp), ("flag", _vp),
        ("ip_id", _vp), ("eth", ctypes.c_uint8 * 14), ("with_eth", ctypes.c_uint8),
    ]


class DecodeOut(ctypes.Structure):
    _fields_ = [
        ("hlen", _vp),
        ("cmd", _vp),
        ("id", _vp),
        ("conv", _vp),
        ("conn_key", _vp),
        ("pay_off", _vp),
        ("pay_len", _vp),
        ("status", _vp),
        ("valid_idx", _vp),
        ("n_valid", _vp),
    ]


class TcpInfoOut(ctypes.Structure):
    _fields_ = [
        ("src", _vp),
        ("dst", _vp),
        ("sp", _vp),
        ("dp", _vp),
        ("seq", _vp),
        ("ack", _vp),
        ("flag", _vp),
        ("parse_status", _vp),
        ("cap_pay_off", _vp),
        ("cap_pay_len", _vp),
    ]


class EncodeHdrIn(ctypes.Structure):
    _fields_ = [("first_byte", _vp), ("pay_len", _vp), ("cmd", _vp), ("conv", _vp), ("conn_key", _vp), ("id", _vp),
                ("id_uniform", ctypes.c_uint8 * 8)]


class DemuxIn(ctypes.Structure):
    _fields_ = [("status", _vp), ("cmd", _vp), ("id", _vp), ("conv", _vp), ("conn_key", _vp), ("dst", _vp)]


class DemuxOut(ctypes.Structure):
    _fields_ = [("perm", _vp), ("seg_off", _vp), ("seg_first", _vp), ("n_seg", _vp), ("n_valid", _vp)]


class DeliverIn(ctypes.Structure):
    _fields_ = [("arena", _vp), ("base_off", _vp), ("inner_off", _vp), ("pay_off", _vp), ("pay_len", _vp),
                ("status", _vp), ("order", _vp), ("n_order", _vp)]


class DeliverOut(ctypes.Structure):
    _fields_ = [("out_arena", _vp), ("out_cap", ctypes.c_uint64), ("out_off", _vp), ("total", _vp),
                ("align", ctypes.c_uint32)]


class VerifyIn(ctypes.Structure):
    _fields_ = [("cap_arena", _vp), ("cap_off", _vp), ("cap_len", _vp), ("status", _vp)]


class VerifyOut(ctypes.Structure):
    _fields_ = [("csum", _vp), ("status_out", _vp), ("n_bad", _vp)]


class ConnTable(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("state", _vp), ("conn_key", _vp),
                ("id", _vp), ("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("seq", _vp), ("ack", _vp),
                ("flag", _vp), ("index", _vp)]


class ConnResolveIn(ctypes.Structure):
    _fields_ = [("status", _vp), ("cmd", _vp), ("id", _vp), ("conn_key", _vp)]


class ConnResolveOut(ctypes.Structure):
    _fields_ = [("conn", _vp), ("hit", _vp), ("miss", _vp), ("n_miss", _vp)]


class ConnExpandOut(ctypes.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("ack", _vp), ("flag", _vp), ("conn_key", _vp),
                ("id", _vp), ("ok", _vp), ("n_bad", _vp)]


class ConnPickIn(ctypes.Structure):
    _fields_ = [("len", _vp), ("id", _vp), ("avoid_key", _vp), ("draw", _vp), ("seed", ctypes.c_uint64)]


class ConnPickOut(ctypes.Structure):
    _fields_ = [("conn", _vp), ("n_none", _vp), ("used", _vp)]


class ControlIn(ctypes.Structure):
    _fields_ = [("status", _vp), ("cmd", _vp), ("id", _vp), ("conn_key", _vp), ("pay_off", _vp), ("pay_len", _vp),
                ("arena", _vp), ("base_off", _vp), ("inner_off", _vp), ("tcp_sp", _vp), ("tcp_dp", _vp), ("miss", _vp)]


class CtlMsgs(ctypes.Structure):
    _fields_ = [("cmd", _vp), ("body", _vp), ("id", _vp), ("src", _vp), ("avoid_key", _vp), ("pay_off", _vp),
                ("pay_len", _vp), ("n_msg", _vp)]


class ControlOut(ctypes.Structure):
    _fields_ = [("kind", _vp), ("arg", _vp), ("conn", _vp), ("n_ctl", _vp), ("rst_first", _vp), ("ka_tries", _vp),
                ("msgs", CtlMsgs)]


class Keepalive(ctypes.Structure):
    _fields_ = [("ka_tries", _vp), ("established_ms", _vp), ("now_ms", ctypes.c_uint64),
                ("request_delay_ms", ctypes.c_uint32), ("max_retry", ctypes.c_uint32), ("online", ctypes.c_uint32)]


class KeepaliveOut(ctypes.Structure):
    _fields_ = [("msgs", CtlMsgs), ("dead_rows", _vp), ("n_dead", _vp)]


class ConnRows(ctypes.Structure):
    _fields_ = [("state", _vp)]


class ConnCloseIn(ctypes.Structure):
    _fields_ = [("close_rows", _vp), ("n_close", _vp), ("m_max", ctypes.c_uint32), ("rst_first", _vp), ("work", _vp),
                ("flags", ctypes.c_uint32)]


class ConnCloseOut(ctypes.Structure):
    _fields_ = [("marked_rows", _vp), ("n_marked", _vp), ("closed_rows", _vp), ("n_closed", _vp), ("pick", _vp),
                ("pick_counts", _vp)]


class ConnCreateRows(ctypes.Structure):
    _fields_ = [("state", _vp), ("conn_key", _vp), ("id", _vp), ("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp),
                ("seq", _vp), ("ack", _vp), ("flag", _vp)]


class ConnOffers(ctypes.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("ack", _vp), ("flag", _vp), ("conn_key", _vp),
                ("id", _vp), ("n_offer", _vp), ("m_max", ctypes.c_uint32)]


class ConnCreateIn(ctypes.Structure):
    _fields_ = [("id", _vp), ("conn_key", _vp), ("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp),
                ("offers", ConnOffers), ("u_max", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("now_ms", ctypes.c_uint64), ("established_ms", _vp), ("ka_tries", _vp), ("work", _vp)]


class ConnCreateOut(ctypes.Structure):
    _fields_ = [("conn", _vp), ("hit", _vp), ("miss", _vp), ("n_miss", _vp), ("new_rows", _vp), ("new_first", _vp),
                ("new_offer", _vp), ("offer_row", _vp), ("n_new", _vp), ("n_full", _vp), ("n_refused", _vp),
                ("pick", _vp), ("pick_counts", _vp)]


class ConvTable(ctypes.Structure):
    _fields_ = [("capacity", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("state", _vp), ("conv", _vp), ("dst", _vp),
                ("id", _vp), ("cur_in", _vp), ("cur_out", _vp), ("prev_in", _vp), ("prev_out", _vp), ("alive", _vp),
                ("index", _vp)]


class ConvResolveIn(ctypes.Structure):
    _fields_ = [("status", _vp), ("cmd", _vp), ("hit", _vp), ("id", _vp), ("conv", _vp), ("dst", _vp),
                ("ctl_kind", _vp), ("ctl_arg", _vp)]


class ConvResolveOut(ctypes.Structure):
    _fields_ = [("conv_row", _vp), ("unknown", _vp), ("n_unknown", _vp), ("rst_first", _vp), ("msgs", CtlMsgs)]


class ConvRows(ctypes.Structure):
    _fields_ = [("state", _vp), ("conv", _vp), ("dst", _vp), ("id", _vp)]


class ConvCreateIn(ctypes.Structure):
    _fields_ = [("id", _vp), ("conv", _vp), ("dst", _vp), ("u_max", ctypes.c_uint32), ("work", _vp)]


class ConvCreateOut(ctypes.Structure):
    _fields_ = [("conv_row", _vp), ("unknown", _vp), ("n_unknown", _vp), ("new_rows", _vp), ("new_first", _vp),
                ("n_new", _vp), ("n_full", _vp)]


class ConvCloseIn(ctypes.Structure):
    _fields_ = [("close_rows", _vp), ("n_close", _vp), ("m_max", ctypes.c_uint32), ("rst_first", _vp), ("ctl_kind", _vp),
                ("work", _vp), ("flags", ctypes.c_uint32)]


class ConvCloseOut(ctypes.Structure):
    _fields_ = [("conv_row", _vp), ("unknown", _vp), ("n_unknown", _vp), ("closed_rows", _vp), ("closed_at", _vp),
                ("n_closed", _vp), ("n_reopened", _vp), ("n_rst_again", _vp)]


class ConvSendOut(ctypes.Structure):
    _fields_ = [("conv", _vp), ("dst", _vp), ("id", _vp), ("ok", _vp), ("n_bad", _vp)]


class ConvFlushOut(ctypes.Structure):
    _fields_ = [("dead_rows", _vp), ("n_dead", _vp), ("n_alive", _vp)]


class Pool(ctypes.Structure):
    _fields_ = [("state", _vp), ("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("seq", _vp), ("ack", _vp),
                ("expiry", _vp), ("index", _vp), ("capacity", ctypes.c_uint32)]


class PoolAddIn(ctypes.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("seq", _vp), ("ack", _vp), ("parse_status", _vp),
                ("expiry", ctypes.c_uint64), ("u_max", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("work", _vp)]


class PoolAddOut(ctypes.Structure):
    _fields_ = [("row", _vp), ("new_rows", _vp), ("new_first", _vp), ("n_new", _vp), ("n_again", _vp), ("n_full", _vp),
                ("n_zero_port", _vp)]


class PoolOffersOut(ctypes.Structure):
    _fields_ = [("src", _vp), ("dst", _vp), ("sp", _vp), ("dp", _vp), ("ack", _vp), ("flag", _vp), ("conn_key", _vp),
                ("n_offer", _vp), ("offer_ack_row", _vp), ("offer_sock_row", _vp), ("n_over", _vp),
                ("m_max", ctypes.c_uint32)]


class PoolSettleIn(ctypes.Structure):
    _fields_ = [("new_offer", _vp), ("n_new", _vp), ("offer_ack_row", _vp), ("offer_sock_row", _vp),
                ("new_max", ctypes.c_uint32), ("m_max", ctypes.c_uint32), ("miss", _vp), ("src", _vp), ("dst", _vp),
                ("sp", _vp), ("dp", _vp), ("work", _vp)]


class PoolSettleOut(ctypes.Structure):
    _fields_ = [("taken_sock_rows", _vp), ("closed_sock_rows", _vp), ("n_closed", _vp), ("n_purged_ack", _vp)]


class PoolFlushOut(ctypes.Structure):
    _fields_ = [("dead_rows", _vp), ("n_dead", _vp)]


class PortList(ctypes.Structure):
    _fields_ = [("n_single", ctypes.c_uint16), ("n_range", ctypes.c_uint16),
                ("single", ctypes.c_uint16 * FILTER_MAX_PORTS), ("range", (ctypes.c_uint16 * 2) * FILTER_MAX_PORTS)]


class CaptureFilter(ctypes.Structure):
    _fields_ = [("src_ip", ctypes.c_uint32), ("dst_ip", ctypes.c_uint32), ("has_src_ip", ctypes.c_uint8),
                ("has_dst_ip", ctypes.c_uint8), ("is_server", ctypes.c_uint8), ("reserved", ctypes.c_uint8),
                ("src_ports", PortList), ("dst_ports", PortList)]


# (name, restype, argtypes) for every symbol the header declares
SIGNATURES = [
    ("rsk_create", _vp, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int]),
    ("rsk_destroy", None, [_vp]),
    ("rsk_set_tag_mode", ctypes.c_int, [_vp, ctypes.c_int]),
    ("rsk_get_tag_mode", ctypes.c_int, [_vp]),
    ("rsk_set_encode_path", ctypes.c_int, [_vp, ctypes.c_int]),
    ("rsk_reserve", ctypes.c_int, [_vp, ctypes.c_uint32]),
    ("rsk_reserve_stream", ctypes.c_int, [_vp, ctypes.c_uint32, _vp]),
    ("rsk_release_stream", ctypes.c_int, [_vp, _vp]),
    ("rsk_check_device_errors", ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32)]),
    ("rsk_forget_captures", ctypes.c_int, [_vp]),
    ("rsk_last_error", ctypes.c_char_p, []),
    ("rsk_version", ctypes.c_char_p, []),
    ("rsk_encode_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, ctypes.POINTER(EncodeIn), ctypes.POINTER(EncodeOut), _vp]),
    ("rsk_encode_wire_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, ctypes.POINTER(EncodeIn), ctypes.POINTER(WireIn), ctypes.POINTER(EncodeOut), _vp]),
    ("rsk_encode_headers_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, ctypes.POINTER(EncodeHdrIn), _vp, _vp, _vp]),
    ("rsk_decode_headers_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.POINTER(DecodeOut), _vp]),
    ("rsk_stage_decode_header", None, [ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p]),
    ("rsk_stage_decode_headers", ctypes.c_int, [ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_int]),
    ("rsk_assemble_frames", ctypes.c_int, [ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, ctypes.c_int]),
    ("rsk_decode_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.POINTER(DecodeOut), _vp]),
    ("rsk_parse_decode_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int,
      ctypes.POINTER(TcpInfoOut), ctypes.POINTER(DecodeOut), _vp]),
    ("rsk_parse_decode_slots_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, ctypes.c_uint32, _vp, _vp, ctypes.c_int, ctypes.c_int,
      ctypes.POINTER(TcpInfoOut), ctypes.POINTER(DecodeOut), _vp]),
    ("rsk_stage_capture_slots", ctypes.c_int, [ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, _vp, ctypes.c_int]),
    ("rsk_tcpinfo_encode_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    ("rsk_syncinput_decode_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.POINTER(TcpInfoOut), ctypes.POINTER(DecodeOut), _vp]),
    ("rsk_capture_filter_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_int, ctypes.POINTER(CaptureFilter), _vp, _vp, _vp, _vp]),
    ("rsk_filter_str", ctypes.c_int, [ctypes.POINTER(CaptureFilter), ctypes.c_char_p, ctypes.c_size_t]),
    ("rsk_filter_parse_decode_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CaptureFilter), _vp,
      ctypes.POINTER(TcpInfoOut), ctypes.POINTER(DecodeOut), _vp]),
    ("rsk_tcp_send_seq_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, _vp, _vp, ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    ("rsk_tcp_recv_ack_batch", ctypes.c_int, [_vp, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint32, _vp, _vp]),
    ("rsk_demux_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, ctypes.POINTER(DemuxIn), ctypes.c_uint32, ctypes.POINTER(DemuxOut), _vp]),
    ("rsk_deliver_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, ctypes.POINTER(DeliverIn), ctypes.POINTER(DeliverOut), _vp]),
    ("rsk_deliver_host", ctypes.c_int,
     [ctypes.c_uint32, ctypes.POINTER(DeliverIn), ctypes.POINTER(DeliverOut), ctypes.c_int]),
    ("rsk_verify_wire_batch", ctypes.c_int,
     [_vp, ctypes.c_uint32, ctypes.POINTER(VerifyIn), ctypes.c_int, ctypes.POINTER(VerifyOut), _vp]),
    ("rsk_verify_wire_host", ctypes.c_int,
     [ctypes.c_uint32, ctypes.POINTER(VerifyIn), ctypes.c_int, ctypes.POINTER(VerifyOut), ctypes.c_int]),
    ("rsk_conn_index_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_conn_index_build", ctypes.c_int, [_vp, ctypes.POINTER(ConnTable), _vp, _vp]),
    ("rsk_conn_resolve_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), ctypes.c_uint32, ctypes.POINTER(ConnResolveIn), ctypes.POINTER(ConnResolveOut),
      _vp]),
    ("rsk_conn_expand_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), ctypes.c_uint32, _vp, ctypes.POINTER(ConnExpandOut), _vp]),
    ("rsk_conn_pick_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_conn_pick_build", ctypes.c_int, [_vp, ctypes.POINTER(ConnTable), _vp, _vp, _vp]),
    ("rsk_conn_pick_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), _vp, ctypes.c_uint32, ctypes.POINTER(ConnPickIn), ctypes.POINTER(ConnPickOut),
      _vp]),
    ("rsk_conn_pick_build_host", ctypes.c_int, [ctypes.POINTER(ConnTable), _vp, _vp, ctypes.c_int]),
    ("rsk_conn_pick_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), _vp, ctypes.c_uint32, ctypes.POINTER(ConnPickIn), ctypes.POINTER(ConnPickOut),
      ctypes.c_int]),
    ("rsk_conn_index_build_host", ctypes.c_int, [ctypes.POINTER(ConnTable), _vp, ctypes.c_int]),
    ("rsk_conn_resolve_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), ctypes.c_uint32, ctypes.POINTER(ConnResolveIn), ctypes.POINTER(ConnResolveOut),
      ctypes.c_int]),
    ("rsk_conn_expand_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), ctypes.c_uint32, _vp, ctypes.POINTER(ConnExpandOut), ctypes.c_int]),
    ("rsk_control_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), ctypes.c_uint32, ctypes.POINTER(ControlIn), ctypes.POINTER(ControlOut), _vp]),
    ("rsk_keepalive_flush", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), ctypes.POINTER(Keepalive), ctypes.POINTER(KeepaliveOut), _vp]),
    ("rsk_control_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), ctypes.c_uint32, ctypes.POINTER(ControlIn), ctypes.POINTER(ControlOut), ctypes.c_int]),
    ("rsk_keepalive_flush_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), ctypes.POINTER(Keepalive), ctypes.POINTER(KeepaliveOut), ctypes.c_int]),
    ("rsk_conv_index_build", ctypes.c_int, [_vp, ctypes.POINTER(ConvTable), _vp, _vp]),
    ("rsk_conv_resolve_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConvTable), ctypes.c_uint32, ctypes.POINTER(ConvResolveIn), ctypes.POINTER(ConvResolveOut),
      _vp]),
    ("rsk_conv_create_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_conv_create_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConvTable), ctypes.POINTER(ConvRows), ctypes.c_uint32, ctypes.POINTER(ConvCreateIn),
      ctypes.POINTER(ConvCreateOut), _vp]),
    ("rsk_conv_create_host", ctypes.c_int,
     [ctypes.POINTER(ConvTable), ctypes.POINTER(ConvRows), ctypes.c_uint32, ctypes.POINTER(ConvCreateIn),
      ctypes.POINTER(ConvCreateOut), ctypes.c_int]),
    ("rsk_conn_close_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_conn_close_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), ctypes.POINTER(ConnRows), ctypes.POINTER(ConnCloseIn),
      ctypes.POINTER(ConnCloseOut), _vp]),
    ("rsk_conn_close_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), ctypes.POINTER(ConnRows), ctypes.POINTER(ConnCloseIn), ctypes.POINTER(ConnCloseOut),
      ctypes.c_int]),
    ("rsk_conn_create_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_conn_create_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConnTable), ctypes.POINTER(ConnCreateRows), ctypes.c_uint32, ctypes.POINTER(ConnCreateIn),
      ctypes.POINTER(ConnCreateOut), _vp]),
    ("rsk_conn_create_host", ctypes.c_int,
     [ctypes.POINTER(ConnTable), ctypes.POINTER(ConnCreateRows), ctypes.c_uint32, ctypes.POINTER(ConnCreateIn),
      ctypes.POINTER(ConnCreateOut), ctypes.c_int]),
    ("rsk_conv_close_bytes", ctypes.c_uint64, [ctypes.c_uint32]),
    ("rsk_conv_close_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConvTable), ctypes.POINTER(ConvRows), ctypes.c_uint32, ctypes.POINTER(ConvCloseIn),
      ctypes.POINTER(ConvCloseOut), _vp]),
    ("rsk_conv_close_host", ctypes.c_int,
     [ctypes.POINTER(ConvTable), ctypes.POINTER(ConvRows), ctypes.c_uint32, ctypes.POINTER(ConvCloseIn),
      ctypes.POINTER(ConvCloseOut), ctypes.c_int]),
    ("rsk_conv_send_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(ConvTable), ctypes.c_uint32, _vp, _vp, ctypes.POINTER(ConvSendOut), _vp]),
    ("rsk_conv_flush", ctypes.c_int, [_vp, ctypes.POINTER(ConvTable), ctypes.POINTER(ConvFlushOut), _vp]),
    ("rsk_conv_index_build_host", ctypes.c_int, [ctypes.POINTER(ConvTable), _vp, ctypes.c_int]),
    ("rsk_conv_resolve_host", ctypes.c_int,
     [ctypes.POINTER(ConvTable), ctypes.c_uint32, ctypes.POINTER(ConvResolveIn), ctypes.POINTER(ConvResolveOut),
      ctypes.c_int]),
    ("rsk_conv_send_host", ctypes.c_int,
     [ctypes.POINTER(ConvTable), ctypes.c_uint32, _vp, _vp, ctypes.POINTER(ConvSendOut), ctypes.c_int]),
    ("rsk_conv_flush_host", ctypes.c_int, [ctypes.POINTER(ConvTable), ctypes.POINTER(ConvFlushOut), ctypes.c_int]),
    ("rsk_pool_index_build", ctypes.c_int, [_vp, ctypes.POINTER(Pool), _vp, _vp]),
    ("rsk_pool_index_build_host", ctypes.c_int, [ctypes.POINTER(Pool), _vp, ctypes.c_int]),
    ("rsk_pool_add_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_pool_add_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(Pool), ctypes.c_uint32, ctypes.POINTER(PoolAddIn), ctypes.POINTER(PoolAddOut), _vp]),
    ("rsk_pool_add_host", ctypes.c_int,
     [ctypes.POINTER(Pool), ctypes.c_uint32, ctypes.POINTER(PoolAddIn), ctypes.POINTER(PoolAddOut), ctypes.c_int]),
    ("rsk_pool_offers", ctypes.c_int, [_vp, ctypes.POINTER(Pool), ctypes.POINTER(Pool), ctypes.POINTER(PoolOffersOut), _vp]),
    ("rsk_pool_offers_host", ctypes.c_int,
     [ctypes.POINTER(Pool), ctypes.POINTER(Pool), ctypes.POINTER(PoolOffersOut), ctypes.c_int]),
    ("rsk_pool_settle_bytes", ctypes.c_uint64, [ctypes.c_uint32, ctypes.c_uint32]),
    ("rsk_pool_settle_batch", ctypes.c_int,
     [_vp, ctypes.POINTER(Pool), ctypes.POINTER(Pool), ctypes.c_uint32, ctypes.POINTER(PoolSettleIn),
      ctypes.POINTER(PoolSettleOut), _vp]),
    ("rsk_pool_settle_host", ctypes.c_int,
     [ctypes.POINTER(Pool), ctypes.POINTER(Pool), ctypes.c_uint32, ctypes.POINTER(PoolSettleIn),
      ctypes.POINTER(PoolSettleOut), ctypes.c_int]),
    ("rsk_pool_flush", ctypes.c_int, [_vp, ctypes.POINTER(Pool), ctypes.c_uint64, ctypes.POINTER(PoolFlushOut), _vp]),
    ("rsk_pool_flush_host", ctypes.c_int, [ctypes.POINTER(Pool), ctypes.c_uint64, ctypes.POINTER(PoolFlushOut), ctypes.c_int]),
    ("rsk_compute_hash", _vp, [_vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]),
    ("rsk_hash_equal", ctypes.c_int, [_vp, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int]),
    ("rsk_enchead_enc2buf", _vp,
     [_vp, ctypes.c_char_p, ctypes.c_int, ctypes.c_uint8, ctypes.c_char_p, ctypes.c_uint32,
      ctypes.c_uint64]),
    ("rsk_enchead_decodebuf", _vp,
     [_vp, ctypes.c_char_p, ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    ("rsk_key_for_tcp", ctypes.c_uint64, [ctypes.c_uint16, ctypes.c_uint16]),
    ("rsk_key_for_udp", ctypes.c_uint64, [ctypes.c_uint16, ctypes.c_uint16]),
    ("rsk_fill_splitmix", ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_uint64, _vp]),
    # include/rsk_rconn.h (RConn-shaped batching adapter)
    ("rsk_rconn_create", _vp, [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint32]),
    ("rsk_rconn_destroy", None, [_vp]),
    ("rsk_rconn_set_callbacks", None, [_vp, _vp, _vp, _vp, _vp]),
    ("rsk_rconn_output", ctypes.c_int,
     [_vp, ctypes.c_int64, ctypes.c_char_p, ctypes.c_uint8, ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint64, _vp]),
    ("rsk_rconn_onrecv", ctypes.c_int, [_vp, ctypes.c_int64, ctypes.c_char_p, ctypes.c_int, _vp]),
    ("rsk_rconn_flush", ctypes.c_int, [_vp]),
    ("rsk_rconn_callback_failures", ctypes.c_uint64, [_vp]),
]

SEND_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
RESET_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)
RECV_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_int, ctypes.c_uint8, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_uint32,
                           ctypes.c_uint64, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p)


def load(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise ImportError(
            f"rsock_amd: HIP library {path} not built; run `python -c 'import __graft_entry__ as g; g.build()'`"
        )
    lib = ctypes.CDLL(path)
    for name, res, args in SIGNATURES:
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    return lib


def demux_ws_layout(lib: ctypes.CDLL, n: int) -> tuple[int, int, int]:
    """rsk__demux_ws_layout (internal, host only, not in the header): (key table offset, key table
    bytes, total bytes) of the demux scratch for a batch of n packets."""
    fn = lib.rsk__demux_ws_layout
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint64)]
    out = (ctypes.c_uint64 * 3)()
    rc = fn(n, out)
    if rc != 0:
        raise ValueError(f"rsk__demux_ws_layout({n}) failed: rc={rc}")
    return int(out[0]), int(out[1]), int(out[2])


def header_symbols(header_paths: list[str] | None = None) -> list[str]:
    """Names of every function declared in include/rsk_codec.h and include/rsk_rconn.h."""
    import re

    if header_paths is None:
        inc = os.path.join(os.path.dirname(_HERE), "include")
        header_paths = [os.path.join(inc, "rsk_codec.h"), os.path.join(inc, "rsk_rconn.h")]
    names = set()
    for hp in header_paths:
        text = re.sub(r"/\*.*?\*/", "", open(hp).read(), flags=re.S)
        text = re.sub(r"typedef[^;]*;", "", text)  # callback typedefs are not exported symbols
        names |= set(re.findall(r"\b(rsk_[a-z0-9_]+)\s*\(", text))
    return sorted(names)
