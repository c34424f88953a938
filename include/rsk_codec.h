/*
 * rsk_codec.h — C ABI of the MI355X framing codec (drop-in for rsock's per-packet codec path).
 *
 * Every entry point is extern "C", takes plain pointers and sizes, and returns 0 or a negative
 * error code.  Batch entry points are stream-ordered (the `stream` argument is a hipStream_t,
 * passed as void* so this header needs no HIP include; NULL = the legacy default stream) and take
 * no ownership: the caller owns every device and host buffer.  All batch array pointers are
 * DEVICE pointers unless a comment says otherwise.  An empty batch (n == 0) is a no-op that may
 * pass null arrays (the ctx and the in/out structs must still be given); it zeroes a given
 * n_valid / n_match / n_seg count.
 *
 * Reference interfaces replaced (paths relative to the rsock tree):
 *   rsk_compute_hash      <- char* compute_hash(char*, const std::string&, const char*, int)   util/rhash.h:17, util/rhash.cpp:20-41
 *   rsk_hash_equal        <- bool hash_equal(const char*, const std::string&, const char*, int) util/rhash.h:13, util/rhash.cpp:71-92
 *   rsk_enchead_enc2buf   <- char* EncHead::Enc2Buf(char*, int)                               bean/EncHead.h:40, bean/EncHead.cpp:9-24
 *   rsk_enchead_decodebuf <- static const char* EncHead::DecodeBuf(EncHead&, const char*, int) bean/EncHead.h:38, bean/EncHead.cpp:39-55
 *   rsk_encode_batch      <- int RConn::Output(ssize_t, const rbuf_t&), framing part          conn/RConn.h:37, conn/RConn.cpp:87-105
 *   rsk_decode_batch      <- int RConn::OnRecv(ssize_t, const rbuf_t&)                        conn/RConn.h:34, conn/RConn.cpp:64-85
 *   rsk_parse_decode_batch<- int RawTcp::RawInput(u_char*, const pcap_pkthdr*, const u_char*) conn/RawTcp.h:38, conn/RawTcp.cpp:138-237
 *   rsk_parse_decode_slots_batch <- the same on host-staged header slots (payloads stay in the capture buffer)
 *                            + RawTcp::cap2uv size check (RawTcp.cpp:239-244) fused with RConn::OnRecv
 *   rsk_tcpinfo_encode_batch <- char* TcpInfo::Encode(char*, int) (21-B hand-off record)      bean/TcpInfo.cpp:20-32, bean/ConnInfo.cpp:12-20
 *   rsk_syncinput_decode_batch <- RawTcp::syncInput -> TcpInfo::Decode -> RConn::OnRecv     conn/RawTcp.cpp:262-276, bean/TcpInfo.cpp:35-47
 *   rsk_encode_wire_batch <- RConn::Output + RawTcp::SendRawTcp -> libnet_build_tcp/ipv4     conn/RawTcp.cpp:280-341
 *   rsk_key_for_tcp/udp   <- KeyGenerator::KeyForTcp / KeyForUdp                              src/util/KeyGenerator.cpp:16-36
 *   rsk_capture_filter_batch <- the pcap filter RCap installs: BuildFilterStr("tcp", srcIp, dstIp, srcPorts,
 *                            dstPorts, isServer) (cap/cap_util.cpp:67-144, cap/RCap.cpp:64-88) evaluated
 *                            per captured packet; rsk_filter_str renders the same string
 *   rsk_filter_parse_decode_batch <- that filter fused with RawTcp::RawInput + RConn::OnRecv (one pass)
 *   rsk_tcp_send_seq_batch <- FakeTcp::Output's seq advance + RawTcp::Output's mIpId++      conn/FakeTcp.cpp:43-49, conn/RawTcp.cpp:111-121
 *   rsk_tcp_recv_ack_batch <- FakeTcp::OnRecv's ack update                                  conn/FakeTcp.cpp:52-66
 *   rsk_demux_batch       <- the per-packet conn lookups of the receive path, batched:
 *                            INetGroup::Input by connKey (conn/INetGroup.cpp:57-83), IAppGroup::Input
 *                            by cmd (conn/IAppGroup.cpp:76-96), ServerGroup::OnRecv by IdBuf
 *                            (server/ServerGroup.cpp:44-60), SubGroup::OnRecv by (dst, conv)
 *                            (server/SubGroup.cpp:31-50), ClientGroup::OnRecv by conv (client/ClientGroup.cpp:66-80)
 *   rsk_deliver_batch     <- the per-packet payload copy of the consumers: SConn::OnRecv
 *                            (server/SConn.cpp:77-89), ClientGroup::send2Origin (client/ClientGroup.cpp:82-96)
 *   rsk_conn_resolve_batch <- INetGroup::Input's lookup of a packet's INetConn by connKey, ConnOfIntKey
 *                            (conn/INetGroup.cpp:57-83), below ServerGroup's per-IdBuf SNetGroup
 *                            (server/ServerGroup.cpp:44-60)
 *   rsk_conn_expand_batch <- INetConn::Output (conn/INetConn.cpp:30-39) handing FakeTcp's TcpInfo mInfo
 *                            (conn/FakeTcp.cpp:14-50) to RawTcp::Output as the packet's addresses, ports,
 *                            ack and flag
 *   rsk_conn_pick_batch   <- INetGroup::doSend's pick of an alive conn per outgoing packet, the conn to
 *                            reset excepted (conn/INetGroup.cpp:111-135)
 *   rsk_conn_table        <- INetGroup's mConnMap and the TcpInfo mInfo of each FakeTcp in it
 *   rsk_conn_create_batch <- INetGroup::Input's miss path (conn/INetGroup.cpp:57-83): SNetGroup::CreateNetConn
 *                            (server/SNetGroup.cpp:20-46), ServerNetManager::GetTcp
 *                            (server/ServerNetManager.cpp:52-75), FakeTcp::Init and AddNetConn; a client's
 *                            AddNetConn behind DialTcpSync / DialTcpAsync (client/CNetGroup.cpp:11-13)
 *   rsk_control_batch     <- IAppGroup::Input's control branches (conn/IAppGroup.cpp:76-96), ConnReset::Input
 *                            (callbacks/ConnReset.cpp:43-90), NetConnKeepAlive::Input
 *                            (callbacks/NetConnKeepAlive.cpp:37-98), IAppGroup::ProcessTcpFinOrRst
 *                            (conn/IAppGroup.cpp:103-116)
 *   rsk_keepalive_flush   <- NetConnKeepAlive::OnFlush / canSendRequest (callbacks/NetConnKeepAlive.cpp:110-145,
 *                            :168-178)
 *   rsk_conv_resolve_batch <- SubGroup::OnRecv's lookup of BuildConvKey(dst, conv) in the packet's SubGroup
 *                            (server/SubGroup.cpp:31-50, server/ServerGroup.cpp:44-60), ClientGroup::OnRecv's
 *                            lookup of conv in mConvMap and its SendConvRst (client/ClientGroup.cpp:65-80,
 *                            callbacks/ConnReset.cpp:34-41), ConnReset::OnRecvConvRst (:67-77) and the
 *                            curr_in++ of IConn::DataStat (conn/IConn.cpp:63-79)
 *   rsk_conv_send_batch   <- SubGroup::sconnSend / ClientGroup::cconSend setting the head's conv, and
 *                            IConn::Send -> afterSend's curr_out++ (conn/IConn.cpp:63-79)
 *   rsk_conv_flush        <- IGroup::Flush (conn/IGroup.cpp:81-107) with IConn::DataStat::Flush
 *   rsk_conv_table        <- a group's mConns at the app level (a server's SubGroups, a ClientGroup's
 *                            mConvMap) and the DataStat of every conv in it
 */
#ifndef RSK_CODEC_H
#define RSK_CODEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- wire constants (include/rstype.h:11-12, include/rscomm.h:19, conn/RConn.cpp:20) ---------- */
#define RSK_HASH_BUF_SIZE 8     /* tag bytes = last 8 bytes of the MD5 digest             */
#define RSK_ID_BUF_SIZE 8       /* IdBuf bytes                                            */
#define RSK_ENC_HEAD_SIZE 23    /* EncHead wire size: len,cmd,id[8],conv u32,key u64,rsvd */
#define RSK_HEAD_SIZE 31        /* RConn::HEAD_SIZE = 8 + 23                              */
#define RSK_MAX_PKT_SIZE 1500   /* OM_MAX_PKT_SIZE                                         */
#define RSK_MAX_PAYLOAD (RSK_MAX_PKT_SIZE - RSK_HEAD_SIZE) /* 1469                          */
#define RSK_TCPINFO_WIRE_SIZE 21 /* TcpInfo::Encode record: src,dst,sp,dp,seq,ack,flag      */

/* EncHead::TYPE (bean/EncHead.h:14-20) */
#define RSK_CMD_DATA 0
#define RSK_CMD_CONV_RST 1
#define RSK_CMD_NETCONN_RST 2
#define RSK_CMD_KEEP_ALIVE_REQ 3
#define RSK_CMD_KEEP_ALIVE_RESP 4

/* TCP flag bits as RawTcp reads them (tcp[13]) */
#define RSK_TH_FIN 0x01
#define RSK_TH_SYN 0x02
#define RSK_TH_RST 0x04
#define RSK_TH_PUSH 0x08
#define RSK_TH_ACK 0x10

/* pcap datalink types accepted by RawTcp::RawInput (RawTcp.cpp:144-165) */
#define RSK_DLT_NULL 0
#define RSK_DLT_EN10MB 1
/* The packet starts at the IPv4 header (pcap DLT_RAW; the LIBNET_RAW4 layout rsk_encode_wire_batch
 * writes with with_eth = 0).  rsk_verify_wire_batch only: the parse and filter entry points reject it. */
#define RSK_DLT_RAW 12

/* ---- error codes returned by every entry point --------------------------------------------- */
#define RSK_OK 0
#define RSK_EINVAL (-22)   /* bad argument (NULL where required, n too large, bad datalink)  */
#define RSK_ENOMEM (-12)   /* device/host allocation failed                                   */
#define RSK_EDEVICE (-5)   /* a HIP runtime call failed (see rsk_last_error())                */

/* ---- per-packet status codes ---------------------------------------------------------------- */
/* Encode (RConn::Output, RConn.cpp:87-128): status[i] = 31 + P (frame length) when the frame was
 * written; RSK_SEND_OVERSIZE (-1) when 31 + P > 1500 (RConn.cpp:94-98, nothing written);
 * RSK_SEND_RESET (0) when P == 0 (the reference calls RConnReset::SendReset instead of framing,
 * RConn.cpp:119-123; nothing written, the caller sends the reset). */
#define RSK_SEND_OVERSIZE (-1)
#define RSK_SEND_RESET 0

/* Decode (RConn::OnRecv, RConn.cpp:64-85): */
#define RSK_RECV_VALID 1   /* tag verified; payload forwarded to IGroup::OnRecv (:73-75)      */
#define RSK_RECV_CLOSE 0   /* nread <= 31 on TCP with FIN|RST: NotifyTcpFinOrRst, return 0    */
#define RSK_RECV_DROP (-1) /* everything else: return -1                                      */

/* Parse (RawTcp::RawInput, RawTcp.cpp:138-237 + cap2uv :239-244): */
#define RSK_PARSE_DROP 0      /* silently dropped (reference returns 0 before delivery)       */
#define RSK_PARSE_DELIVER 1   /* handed to cap2uv -> syncInput -> RConn::OnRecv               */
#define RSK_PARSE_SYN 2       /* SYN with an ack pool: TcpAckPool::AddInfoFromPeer, return 0   */
#define RSK_PARSE_MALFORMED 3 /* header runs past cap_len, or negative payload_len with FIN|RST
                                 (the reference memcpy's a negative length there: UB,
                                 RawTcp.cpp:251) — defined here as a drop                      */
#define RSK_PARSE_SLOT_SHORT 4 /* rsk_parse_decode_slots_batch only: a byte the parse or decode
                                  reads lies past the staged slot; resubmit the packet whole   */

/* parse flags */
#define RSK_PARSE_HAS_ACK_POOL 0x1 /* RawTcp::mTcpAckPool != nullptr                          */
#define RSK_PARSE_IS_SERVER 0x2    /* RawTcp::mIsServer: SYN info is Reverse()d (:222-224)     */

/* Largest n of any batch entry point (RSK_EINVAL above it): every launch has at most one work-item
 * per packet rounded up to its 256-thread blocks, and a grid holds at most 2^32 - 1 work-items (the
 * encode copy waves -- 64 work-items per packet -- run in several launches). */
#define RSK_MAX_BATCH 0xFFFF0000u

/* ---- context -------------------------------------------------------------------------------- */
typedef struct rsk_ctx rsk_ctx;

/* Create a codec context bound to HIP device `device` for hash key `key` (host pointer, key_len
 * bytes, any length; rsock's default is "hello135", bean/RConfig.h:44).  The tag is
 * MD5(key || payload[0])[8..15] (util/rhash.cpp:20-41).  The key's MD5 message schedule is
 * precomputed here (chaining state of the whole-key blocks, the constant words of the block that
 * carries the payload byte, the padding block when one is needed), and one GPU launch (k_tag_table)
 * compresses the key's 256 possible tags into a 2-KB device table for RSK_TAG_TABLE.  The context
 * starts in RSK_TAG_MD5.  Synchronous; returns NULL on failure (rsk_last_error). */
rsk_ctx *rsk_create(const uint8_t *key, uint32_t key_len, int device);
void rsk_destroy(rsk_ctx *ctx);

/* Tag mode of every later framing / verifying launch of this context (outputs are identical):
 *   RSK_TAG_MD5    (default) one MD5 compression per packet and lane, as the reference computes it
 *                  per packet (compute_hash / hash_equal, util/rhash.cpp:20-41, 71-92);
 *   RSK_TAG_TABLE  the tag is a function of payload[0] alone, so it is looked up in the key's
 *                  256-entry table (staged in LDS per block) instead of recomputed.
 * The mode is read when a call is issued (a hipGraph keeps the mode of its capture); do not change it
 * while another thread issues calls on the same context.  rsk_set_tag_mode returns RSK_EINVAL for an
 * unknown mode, rsk_get_tag_mode the current mode (or RSK_EINVAL for a NULL ctx). */
#define RSK_TAG_MD5 0
#define RSK_TAG_TABLE 1
int rsk_set_tag_mode(rsk_ctx *ctx, int mode);
int rsk_get_tag_mode(const rsk_ctx *ctx);

/* Encode path of this context's rsk_encode_batch calls (outputs are identical):
 *   RSK_ENC_PATH_AUTO     (default) chosen per call of >= 16384 packets from the mean payload of the
 *                         context's last sampled batch (table under rsk_encode_batch);
 *   RSK_ENC_PATH_PER_SET  one kernel, 64 packets per wave (every batch shape);
 *   RSK_ENC_PATH_TWO_PASS a header pass (MD5 tags 64 to a wave, 32-B records in the stream's scratch),
 *                         then copy waves of 1, 2 or 4 packets: 4 below a mean payload of 880 B, 2 below
 *                         1160 B, 1 above (batches of long frames); below 880 B, when the sampled frames
 *                         lie back to back sharing their boundary 16-B chunks (byte-packed, no pad),
 *                         an output-stationary copy instead (waves own 2-KB blocks of the frame arena
 *                         and write each shared chunk once; frames out of packet order or more than
 *                         32 KB apart are copied packet by packet by the same launch);
 *   RSK_ENC_PATH_SHORT    the per-set kernel with every set on the flat chunk list (batches of short
 *                         frames).
 * Read when a call is issued, as the tag mode; RSK_EINVAL for an unknown path. */
#define RSK_ENC_PATH_AUTO 0
#define RSK_ENC_PATH_PER_SET 1
#define RSK_ENC_PATH_TWO_PASS 2
#define RSK_ENC_PATH_SHORT 3
int rsk_set_encode_path(rsk_ctx *ctx, int path);

/* Streams: a context may be used from several streams at once.  Its device scratch (compaction
 * ballots and look-back state, demux and send-seq tables) is kept per stream, so calls on different streams
 * never share it; calls on ONE stream must be issued in the order the caller wants them to run
 * (from one host thread at a time, as with any hipStream_t).  The only per-context state the
 * kernels read is the immutable key schedule and tag table (and the tag mode, passed by value).
 *
 * Pre-size the scratch of `stream` (rsk_reserve: the legacy default stream, NULL) for batches of up
 * to n packets: the compaction state, the tile sums of rsk_deliver_batch and the tile counts of
 * rsk_control_batch / rsk_keepalive_flush (8 B per 1024 / 2048 packets), and, for n >= 16384, the header records of the two-pass encode
 * and wire build (max(40 n + 24, 96 min(n, 2^20)) bytes: 32-B records and the output-stationary
 * copy's block map) -- only for a context that encodes: one held to RSK_ENC_PATH_TWO_PASS, or an AUTO
 * context that has already run an rsk_encode_batch call (so a decode- or demux-only context pays
 * nothing for them; a failed records allocation is not an error: eager calls allocate them on demand,
 * a captured call then takes the per-set kernel).  Batch calls grow the scratch on demand, which waits
 * for that stream to drain and allocates; reserve first if batch calls will be captured into a hipGraph. */
int rsk_reserve(rsk_ctx *ctx, uint32_t n_max);
int rsk_reserve_stream(rsk_ctx *ctx, uint32_t n_max, void *stream);
/* Scratch stays allocated per stream until the context is destroyed or the stream is released:
 * rsk_release_stream waits for `stream` to drain and frees its scratch (call it before destroying a
 * stream whose handle value a later stream may reuse).  A batch call issued while `stream` is being
 * captured into a hipGraph cannot allocate, grow or initialise that scratch (RSK_EINVAL): reserve
 * the stream and run one eager call on it before the capture.  A graph's scratch is its capture
 * stream's: replay it on that stream, or on streams ordered with it.  Graphs captured on `stream`
 * point at that scratch: destroy them before rsk_release_stream (a replay afterwards would use freed
 * device memory). */
int rsk_release_stream(rsk_ctx *ctx, void *stream);

/* Device-side error flags, sticky per context.  RSK_DEVERR_LOOKBACK: a decoupled look-back (the
 * VALID-list compaction of the decode entry points, the demux) gave up waiting for a predecessor
 * tile after ~4M polls, so that call's valid_idx / n_valid / demux outputs are wrong (a compaction
 * that gave up anywhere writes n_valid = 0xFFFFFFFF); the spin limit exists so that such a stall can
 * never hang the GPU.  rsk_check_device_errors waits for the context's streams (those it has
 * scratch on, and its shim stream; not the whole device -- except for a context with a call captured
 * into a hipGraph, whose replays may run on streams it never saw: then the whole device, until
 * rsk_forget_captures), stores the flags in *flags (may be NULL) and clears them; when any flag was
 * set it returns RSK_EDEVICE and re-initialises the context's look-back state on every stream at its
 * next call there (graphs captured earlier must be captured again). */
#define RSK_DEVERR_LOOKBACK 0x1u
/* RSK_DEVERR_TABLE: a demux key probe walked the whole key table without finding its key or a free
 * slot (the table is kept all-ones between calls, each call clearing the slots it claimed; a table
 * left dirty -- which no completed call does -- would otherwise hang the probe): that call's demux
 * outputs are wrong, and the table is filled again at the next call. */
#define RSK_DEVERR_TABLE 0x2u
int rsk_check_device_errors(rsk_ctx *ctx, uint32_t *flags);
/* The caller has destroyed every graph that captured this context's calls (or replays them only on
 * streams this context has scratch on): rsk_check_device_errors waits for the context's streams
 * again instead of the whole device. */
int rsk_forget_captures(rsk_ctx *ctx);

/* Text of the last HIP error seen by this thread (static storage). */
const char *rsk_last_error(void);

/* Library version string, e.g. "rsk 0.1 gfx950". */
const char *rsk_version(void);

/* ---- batch encode (RConn::Output framing) --------------------------------------------------- */
typedef struct rsk_encode_in {
    const uint8_t *payload_arena; /* device bytes                                           */
    const uint64_t *pay_off;      /* [n] byte offset of packet i's payload in payload_arena  */
    const uint16_t *pay_len;      /* [n] P = nread                                           */
    const uint8_t *cmd;           /* [n] EncHead cmd                                         */
    const uint32_t *conv;         /* [n] EncHead conv                                        */
    const uint64_t *conn_key;     /* [n] EncHead connKey                                     */
    const uint8_t *id;            /* [n*8] per-packet IdBuf, or NULL to use id_uniform       */
    uint8_t id_uniform[8];        /* IdBuf used for every packet when id == NULL             */
} rsk_encode_in;

typedef struct rsk_encode_out {
    uint8_t *frame_arena;     /* device bytes                                              */
    const uint64_t *frame_off;/* [n] where frame (wire packet) i starts; any offset is correct
                                 and takes the vector path (16-B aligned: no partial head chunk) */
    int32_t *status;          /* [n] 31+P, RSK_SEND_OVERSIZE or RSK_SEND_RESET              */
    uint32_t flags;           /* RSK_ENC_* below; 0 = write exactly 31+P bytes per frame      */
} rsk_encode_out;

/* RSK_ENC_ZERO_PAD16: the encoder may also write zeros from each frame's end (31+P) up to the
 * next 16-byte boundary of the arena address.  The caller asserts those bytes belong to no other
 * frame (e.g. frames in 16-B-multiple slots).  This mirrors the reference, whose frames sit in a
 * zeroed 1500-B buffer (RConn.cpp:100), and lets every 16-B chunk of a slot be written whole —
 * no byte stores and no partially written cache lines, which the memory side otherwise services
 * with read-modify-write. */
#define RSK_ENC_ZERO_PAD16 0x1u
/* RSK_ENC_ZERO_PAD128: as RSK_ENC_ZERO_PAD16 but up to the next 128-byte (cache-line) boundary;
 * takes precedence over RSK_ENC_ZERO_PAD16. */
#define RSK_ENC_ZERO_PAD128 0x2u

/* frame_i = tag(8) | EncHead(23) | payload(P), written to frame_arena + frame_off[i].
 * Frames must not overlap each other or the payload arena.
 * Three device paths, identical bytes (rsk_set_encode_path): the per-set kernel (64 packets per wave),
 * the short-frame kernel (every set on the flat chunk list) and the two-pass form (a header pass: the
 * MD5 tags 64 to a wave into 32-B records in the stream's scratch; then copy waves of 1, 2 or 4
 * packets).  AUTO chooses per call of >= 16384 packets by the mean payload of the context's last
 * sampled batch: <= 96 B short-frame, < 224 B per-set, < 400 B short-frame, < 880 B two-pass with 4
 * packets per copy wave, < 1160 B 2, else 1; smaller batches take the per-set kernel.
 * The statistic is a host-mapped word the previous calls' kernels left (read without synchronisation:
 * calls issued back to back see it late, which only delays a switch of traffic mix); the first such call
 * on a context, which has no statistic yet, samples its own batch with one 64-thread launch on
 * `stream` and waits for an event recorded behind it -- i.e. for `stream`'s work up to that launch,
 * since a stream runs in order (with this thread's capture mode relaxed for the wait); a failed
 * wait returns RSK_EDEVICE.  A call being captured, or issued on the legacy NULL stream, does not
 * wait: it takes the per-set kernel, and the sample launched behind it decides the next calls.  A call
 * captured into a hipGraph keeps the path it was captured with, and one captured on a stream without
 * reserved records takes the per-set kernel.  rsk_set_encode_path fixes the path for a context
 * (e.g. one fed alternating long- and short-frame batches). */
int rsk_encode_batch(rsk_ctx *ctx, uint32_t n, const rsk_encode_in *in, const rsk_encode_out *out,
                     void *stream);

/* ---- batch encode straight to wire packets (RConn::Output + RawTcp::SendRawTcp) ---
 * RawTcp::SendRawTcp (conn/RawTcp.cpp:280-341) hands each frame to libnet 1.1.6:
 * libnet_build_tcp(sp, dp, seq, ack, flag, win 65535, sum auto, urg 0) and
 * libnet_build_ipv4(40 + frame, tos 0, id = mIpId++, IP_DF, TTL 64, IPPROTO_TCP, sum auto, src, dst).
 * This entry point frames AND builds the packet in one pass: out->frame_arena + frame_off[i] receives
 * [eth 14 if with_eth] | IPv4 20 | TCP 20 | tag 8 | EncHead 23 | payload, with the IPv4 header checksum
 * and the TCP checksum (RFC 793 pseudo-header, RFC 1071 sum over header + frame) filled in.
 * status[i] = wire length (14? + 40 + 31 + P), RSK_SEND_OVERSIZE or RSK_SEND_RESET as for
 * rsk_encode_batch; out->flags as there (padding counts from the end of the wire packet).  The value
 * RConn::Output returns for a sent frame is SendRawTcp's `payload_len` (RawTcp.cpp:340), i.e. the
 * frame length status[i] - 40 - (with_eth ? 14 : 0).  seq and ip_id are the caller's per-packet
 * values: the reference advances them per send (FakeTcp::Output: seq += 31 + nread, FakeTcp.cpp:43-49;
 * RawTcp::Output: mIpId++, RawTcp.cpp:118-120), so one connection's batch carries
 * seq[i] = seq0 + sum_{k<i} (31 + P_k) and ip_id[i] = id0 + i.
 * Two device paths, identical bytes: the per-set wire kernels (a flat half and a per-packet half),
 * and (round 6) the two-pass form -- a header pass writing each packet's header image (80 / 96 B,
 * RAW4 / Ethernet) into the stream's scratch, then copy waves of 4 / 2 / 1 packets that sum the
 * payload into the TCP checksum -- run per chunk of 2^20 packets.  The path follows the context's
 * rsk_set_encode_path (TWO_PASS: the two-pass form; any other forced path: the per-set kernels) or,
 * under AUTO, the sampled mean payload: per-set below 160 B and for Ethernet packets from 1300 B, the
 * two-pass form otherwise, 4 packets per copy wave, RAW4 from 1080 B 2. */
typedef struct rsk_wire_in {
    const uint32_t *src, *dst; /* [n] TcpInfo::src / dst: IPv4 addresses as stored (network order) */
    const uint16_t *sp, *dp;   /* [n] ports, host order                                           */
    const uint32_t *seq, *ack; /* [n] host order (TcpInfo seq / ack at send time)                 */
    const uint8_t *flag;       /* [n] TCP flags (TcpInfo::flag)                                   */
    const uint16_t *ip_id;     /* [n] IPv4 identification (RawTcp::mIpId++, host order)           */
    uint8_t eth[14];           /* link header written before the IPv4 header when with_eth       */
    uint8_t with_eth;          /* 0: LIBNET_RAW4 layout (IPv4 first); 1: Ethernet frame           */
} rsk_wire_in;
int rsk_encode_wire_batch(rsk_ctx *ctx, uint32_t n, const rsk_encode_in *in, const rsk_wire_in *wire,
                          const rsk_encode_out *out, void *stream);

/* ---- batch decode + verify (RConn::OnRecv) --------------------------------------------------- */
typedef struct rsk_decode_out {
    uint8_t *hlen;       /* [n] EncHead len byte as received (payload starts at 8 + hlen)      */
    uint8_t *cmd;        /* [n]                                                               */
    uint8_t *id;         /* [n*8]                                                             */
    uint32_t *conv;      /* [n]                                                               */
    uint64_t *conn_key;  /* [n]                                                               */
    uint16_t *pay_off;   /* [n] payload offset relative to the frame start (= 8 + hlen)       */
    uint16_t *pay_len;   /* [n] nread - 8 - hlen                                              */
    int8_t *status;      /* [n] RSK_RECV_*                                                    */
    uint32_t *valid_idx; /* [n] order-stable list of i with status == RSK_RECV_VALID (may be NULL) */
    uint32_t *n_valid;   /* [1] number of entries in valid_idx (device; may be NULL)            */
} rsk_decode_out;
/* For packets whose status is not RSK_RECV_VALID, hlen/cmd/id/conv/conn_key/pay_off/pay_len are
 * written as zero (the reference never exposes fields of a dropped frame). */

/* frame i = frame_len[i] bytes at frame_arena + frame_off[i]; is_tcp_close[i] != 0 marks a frame
 * that arrived on fake TCP with FIN or RST set (TcpInfo::HasCloseFlag, bean/TcpInfo.h:31); NULL
 * means "UDP / no close flag" for all packets. */
int rsk_decode_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *frame_arena, const uint64_t *frame_off,
                     const uint16_t *frame_len, const uint8_t *is_tcp_close, const rsk_decode_out *out,
                     void *stream);

/* ---- header-only batches (host-resident deployments) ------------------------------------------
 * The codec reads one payload byte per frame (payload[0] for the tag) and writes / verifies the
 * first 31 frame bytes: a caller whose payloads live in host memory ships only those bytes over PCIe
 * and keeps the payload where it is (assembling frame = header(31) | payload with an iovec, or the
 * memcpy RConn.cpp:104 does anyway).  Slots are 32 B, 16-B aligned, slot i at hdr + 32 i. */
typedef struct rsk_encode_hdr_in {
    const uint8_t *first_byte; /* [n] payload[0] (read only when 1 <= pay_len <= 1469)             */
    const uint16_t *pay_len;   /* [n]                                                              */
    const uint8_t *cmd;
    const uint32_t *conv;
    const uint64_t *conn_key;
    const uint8_t *id;         /* [n*8] 8-B aligned, or NULL (then id_uniform)                     */
    uint8_t id_uniform[8];
} rsk_encode_hdr_in;
/* slot i = frame bytes [0, 32): tag | EncHead | payload[0]; zero when status[i] <= 0.  status as
 * rsk_encode_batch. */
int rsk_encode_headers_batch(rsk_ctx *ctx, uint32_t n, const rsk_encode_hdr_in *in, uint8_t *hdr,
                             int32_t *status, void *stream);
/* slot i = frame bytes [0, 31) and, in byte 31, the byte OnRecv hashes: frame[8 + len] with
 * len = frame[8] (= frame[31] for a well-formed frame); rsk_stage_decode_header builds it.
 * frame_len[i] is the frame's full length; outputs exactly as rsk_decode_batch on the whole frame. */
int rsk_decode_headers_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *hdr, const uint16_t *frame_len,
                             const uint8_t *is_tcp_close, const rsk_decode_out *out, void *stream);
/* Host: the decode slot of one received frame (host pointers). */
void rsk_stage_decode_header(const uint8_t *frame, int nread, uint8_t *slot);
/* Host batch forms (host pointers; nthreads <= 1 runs on the caller's thread): stage the slots of n
 * frames at arena + frame_off[i]; assemble frame i = hdr slot bytes [0, 31) | payload (status[i] - 31
 * bytes at payload_arena + pay_off[i]) for status[i] > 0 — the copy RConn::Output makes
 * (RConn.cpp:100-104) when the sender needs one contiguous frame. */
int rsk_stage_decode_headers(uint32_t n, const uint8_t *arena, const uint64_t *frame_off,
                             const uint16_t *frame_len, uint8_t *slots, int nthreads);
int rsk_assemble_frames(uint32_t n, const uint8_t *hdr, const int32_t *status, const uint8_t *payload_arena,
                        const uint64_t *pay_off, uint8_t *frame_arena, const uint64_t *frame_off, int nthreads);

/* ---- fused pcap parse + decode (RawTcp::RawInput -> cap2uv -> RConn::OnRecv) ----------------- */
typedef struct rsk_tcpinfo_out {
    uint32_t *src;  /* [n] ip_dst as stored (network byte order bytes, read LE) — "self" view   */
    uint32_t *dst;  /* [n] ip_src as stored                                                    */
    uint16_t *sp;   /* [n] ntohs(th_dport)                                                     */
    uint16_t *dp;   /* [n] ntohs(th_sport)                                                     */
    uint32_t *seq;  /* [n] ntohl(th_seq) (+ payload_len when delivered)                        */
    uint32_t *ack;  /* [n] ntohl(th_ack)                                                       */
    uint8_t *flag;  /* [n] th_flags                                                            */
    int8_t *parse_status; /* [n] RSK_PARSE_*                                                   */
    uint16_t *cap_pay_off; /* [n] payload (= frame) offset inside the captured packet          */
    uint16_t *cap_pay_len; /* [n] payload_len (0 unless delivered)                             */
} rsk_tcpinfo_out;
/* TcpInfo fields are written for RSK_PARSE_DELIVER and RSK_PARSE_SYN, zero otherwise.  The decode
 * outputs (`dec`) follow rsk_decode_batch on the delivered payload with is_tcp_close = flag &
 * (FIN|RST); packets that were not delivered get dec->status = RSK_RECV_DROP and zero fields. */
int rsk_parse_decode_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *cap_arena, const uint64_t *cap_off,
                           const uint32_t *wire_len, const uint32_t *cap_len, int datalink, int flags,
                           const rsk_tcpinfo_out *tcp, const rsk_decode_out *dec, void *stream);

/* Host-resident capture (copy only the first ~86 B of each captured packet, keep the
 * payloads host-side): packet i's first min(cap_len[i], slot) bytes at slots + slot * i (slot a
 * multiple of 16, >= RSK_CAP_SLOT_MIN; slots 16-B aligned), staged by rsk_stage_capture_slots.  Same
 * outputs as rsk_parse_decode_batch on the whole capture (decisions use the real cap_len), except
 * that a packet whose parse or decode must read a byte past its slot (IP/TCP options, an EncHead
 * len byte that moves the hashed byte) gets parse_status RSK_PARSE_SLOT_SHORT with zero outputs
 * and dec->status RSK_RECV_DROP: resubmit those through rsk_parse_decode_batch.  With slot = 96 a
 * rsock packet (IHL 5, data offset 5, len 23) needs 86 B (EN10MB) or 76 B (NULL). */
#define RSK_CAP_SLOT_MIN 64
int rsk_parse_decode_slots_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *slots, uint32_t slot,
                                 const uint32_t *wire_len, const uint32_t *cap_len, int datalink, int flags,
                                 const rsk_tcpinfo_out *tcp, const rsk_decode_out *dec, void *stream);
/* Host: stage the slots of n captured packets at arena + cap_off[i] (first min(cap_len[i], slot)
 * bytes, the rest of the slot zeroed). */
int rsk_stage_capture_slots(uint32_t n, const uint8_t *arena, const uint64_t *cap_off, const uint32_t *cap_len,
                            uint32_t slot, uint8_t *slots, int nthreads);

/* ---- TcpInfo hand-off records (cap2uv's 21-B TcpInfo::Encode) ---------------- */
/* rec[21*i ..] = src LE32 | dst LE32 | sp LE16 | dp LE16 | seq LE32 | ack LE32 | flag. */
int rsk_tcpinfo_encode_batch(rsk_ctx *ctx, uint32_t n, const uint32_t *src, const uint32_t *dst,
                             const uint16_t *sp, const uint16_t *dp, const uint32_t *seq,
                             const uint32_t *ack, const uint8_t *flag, uint8_t *rec, void *stream);
/* The consumer side (RawTcp::syncInput, conn/RawTcp.cpp:262-276 -> TcpInfo::Decode,
 * bean/TcpInfo.cpp:35-47 -> RConn::OnRecv): record i = nread[i] bytes at rec_arena + rec_off[i], a
 * 21-B TcpInfo record followed by the frame (what cap2uv sends, RawTcp.cpp:239-260).  A record of
 * nread >= 21 bytes gets parse_status RSK_PARSE_DELIVER, its TcpInfo fields, cap_pay_off 21,
 * cap_pay_len nread - 21, and dec = rsk_decode_batch on the frame with is_tcp_close = flag &
 * (FIN|RST).  nread < 21: RSK_PARSE_DROP, zero TcpInfo, dec->status RSK_RECV_DROP (syncInput
 * returns before Input for nread <= 0 and for a failed Decode; for 12 <= nread < 21 the reference's
 * Decode does not fail but reads its receive buffer past nread — TcpInfo.cpp:40 compares the
 * bytes consumed, not those left — so this is the one deliberate deviation, on malformed input). */
int rsk_syncinput_decode_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *rec_arena, const uint64_t *rec_off,
                               const int32_t *nread, const rsk_tcpinfo_out *tcp, const rsk_decode_out *dec,
                               void *stream);

/* ---- fake-TCP connection state on either side of the codec --------------------------------------- */
/* Send: FakeTcp::Output (conn/FakeTcp.cpp:43-49) advances its connection's seq by
 * RConn::HEAD_SIZE + nread after every frame RConn::Output produced, and RawTcp::Output
 * (conn/RawTcp.cpp:111-121) stamps every packet it sends with mIpId++.  For a batch sent in order,
 * packet i of connection conn[i] with rsk_encode_batch's status[i] (31 + P when framed):
 *   framed (status > 0): ip_id[i] = *ip_id_next, then ++*ip_id_next (wraps at 2^16); and when
 *       conn[i] < n_conn: seq[i] = conn_seq[conn[i]], then conn_seq[conn[i]] += status[i] (mod 2^32)
 *   otherwise, or conn[i] >= n_conn: seq[i] = 0 (ip_id[i] = 0 when not framed)
 * conn_seq [n_conn] and ip_id_next [1] are device state updated in place; seq / ip_id are what
 * rsk_encode_wire_batch takes.  n <= 2^30.  Workspace: n_conn < 2048 takes a per-tile connection table
 * (<= 4 B per packet); wider n_conn the demux group-by (its workspace plus ~35 B per packet). */
int rsk_tcp_send_seq_batch(rsk_ctx *ctx, uint32_t n, const uint32_t *conn, const int32_t *status,
                           uint32_t n_conn, uint32_t *conn_seq, uint16_t *ip_id_next, uint32_t *seq,
                           uint16_t *ip_id, void *stream);
/* Receive: FakeTcp::OnRecv (conn/FakeTcp.cpp:52-66) raises its connection's ack to a delivered
 * packet's TcpInfo seq (rsk_parse_decode_batch's tcp->seq) when that is larger (unsigned compare,
 * as the reference), so over a batch conn_ack[c] = max(conn_ack[c], seq[i] of every packet i with
 * delivered[i] != 0 and conn[i] == c) — independent of order; conn[i] >= n_conn is skipped.
 * n <= 2^30 (RSK_EINVAL above). */
int rsk_tcp_recv_ack_batch(rsk_ctx *ctx, uint32_t n, const uint32_t *conn, const uint8_t *delivered,
                           const uint32_t *seq, uint32_t n_conn, uint32_t *conn_ack, void *stream);

/* ---- receive demux: stable group-by of the VALID packets on decoded fields --- */
/* The reference routes every VALID packet on its own: a map lookup per packet on the fields below,
 * packets delivered in arrival order.  rsk_demux_batch groups a decoded batch so the host does one
 * lookup per segment and hands each conn its packets as one run:
 *   - the key is the tuple of the fields selected in `fields` (unselected fields are ignored);
 *   - with RSK_DEMUX_CMD_BARRIER, a packet whose cmd != RSK_CMD_DATA (RST / keepalive, handled by
 *     IAppGroup outside the conn maps) is a segment of its own and an ordering barrier: DATA
 *     packets on either side of it never share a segment;
 *   - with RSK_DEMUX_GROUP_BARRIER instead (requires RSK_DEMUX_ID, excludes CMD_BARRIER), a control
 *     packet is a segment of its own and a barrier for the packets of its own IdBuf only: DATA
 *     packets of one IdBuf on either side of it never share a segment, packets of other IdBufs
 *     are not split by it.  That is the server's routing: ServerGroup::OnRecv (server/
 *     ServerGroup.cpp:44-60) hands each packet to its IdBuf's SubGroup, whose conns and control
 *     handling never see another IdBuf's packets, so only the order inside one IdBuf is
 *     observable.  A server batch then has about one segment per conn and epoch of its own group
 *     instead of one per conn and epoch of the whole batch;
 *   - segments are ordered by their first packet, packets inside a segment by arrival.
 * Delivering segment by segment therefore hands every conn the same packet sequence as the
 * reference's per-packet loop, and creates new conns in the same order (first occurrence). */
#define RSK_DEMUX_ID            0x01u /* EncHead IdBuf (8 B)                                      */
#define RSK_DEMUX_CONN_KEY      0x02u /* EncHead connKey                                          */
#define RSK_DEMUX_CONV          0x04u /* EncHead conv                                             */
#define RSK_DEMUX_DST           0x08u /* TcpInfo dst (SubGroup keys on BuildConvKey(dst, conv))   */
#define RSK_DEMUX_CMD_BARRIER   0x10u
#define RSK_DEMUX_GROUP_BARRIER 0x20u
typedef struct rsk_demux_in {
    const int8_t *status;      /* [n] packet i takes part iff status[i] == RSK_RECV_VALID       */
    const uint8_t *cmd;        /* [n]                                                           */
    const uint8_t *id;         /* [n*8] (8-B aligned); may be NULL unless RSK_DEMUX_ID           */
    const uint32_t *conv;      /* [n]; may be NULL unless RSK_DEMUX_CONV                         */
    const uint64_t *conn_key;  /* [n]; may be NULL unless RSK_DEMUX_CONN_KEY                     */
    const uint32_t *dst;       /* [n]; may be NULL unless RSK_DEMUX_DST                          */
} rsk_demux_in;
typedef struct rsk_demux_out {
    uint32_t *perm;      /* [n] packet indices, segment by segment (first n_valid entries used)   */
    uint32_t *seg_off;   /* [n+1] segment s = perm[seg_off[s] .. seg_off[s+1]) (first n_seg+1)   */
    uint32_t *seg_first; /* [n] first packet of segment s (its key representative), increasing    */
    uint32_t *n_seg;     /* [1]                                                                   */
    uint32_t *n_valid;   /* [1]                                                                   */
} rsk_demux_out;
/* n <= 2^30.  Workspace (per stream, grown on demand): about 75 B per packet.  Its key table is kept
 * all-ones between calls at a place that depends on the table size alone, so calls of any batch
 * sizes may follow each other on a stream.  A call captured into a hipGraph needs the stream's
 * workspace to exist at the largest size that will run on that stream (rsk_reserve_stream does not
 * size it: run one eager call of that size first); growing it later frees what the graph points at.
 * GROUP_BARRIER runs
 * two group-bys (the control packets by IdBuf, then every packet by the key with each DATA packet's
 * epoch inside its IdBuf), writing
 * the first one's result to `out` before the second overwrites it. */
int rsk_demux_batch(rsk_ctx *ctx, uint32_t n, const rsk_demux_in *in, uint32_t fields,
                    const rsk_demux_out *out, void *stream);

/* ---- payload delivery: the VALID payloads packed in delivery order ------------------------------ */
/* The reference's consumers copy every delivered payload on its own: SConn::OnRecv
 * (server/SConn.cpp:77-89) and ClientGroup::send2Origin (client/ClientGroup.cpp:82-96) malloc +
 * memcpy(base, rbuf.base, nread) and uv_udp_send it, where rbuf.base is the pointer RConn::OnRecv
 * computed (conn/RConn.cpp:64-85: p = base + 8 + len, length nread - (p - base)).  rsk_deliver_batch is
 * that copy for a batch: the payloads of the VALID packets gathered into one dense arena in delivery
 * order, with the byte offset of every payload -- what completes "hands each conn its packets as one
 * run" above: with order = the demux's perm, segment s is the bytes
 * [out_off[seg_off[s]], out_off[seg_off[s + 1]]) of out_arena, so the host makes one contiguous D2H
 * (or hands the arena to a next device stage) and one sendmmsg per segment with iovecs from out_off.
 *
 * Let m = n when order == NULL, else min(*n_order, n).  Position k < m stands for packet i = order[k]
 * (k itself without an order) and has length L_k = pay_len[i] when i < n and status[i] ==
 * RSK_RECV_VALID, else L_k = 0: a stray index, a packet that is not VALID, and every position of a
 * poisoned n_valid of 0xFFFFFFFF (a look-back timeout, RSK_DEVERR_LOOKBACK) whose entry is stray, is
 * skipped and its packet fields are never read (`order` must be readable for n entries, as perm and
 * valid_idx are).
 *   out_off[0] = 0, out_off[k + 1] = out_off[k] + roundup(L_k, align); every entry from m to n equals
 *   the total, and *total = out_off[m].
 *   Payload k is the L_k bytes at arena + base_off[i] + inner_off[i] + pay_off[i]; it lands at
 *   out_arena + out_off[k], followed by zeros up to the rounded length.
 * A payload whose rounded end exceeds out_cap is not written at all, and no byte at or past out_cap is
 * written; *total still reports the need, so the caller compares it with out_cap (no device error bit).
 * Every destination byte is written at most once, and nothing outside the rounded ranges is written.
 * arena and out_arena must not overlap.  n <= 2^30.  RSK_EINVAL: a NULL in, out, out_off, base_off,
 * pay_off, pay_len or status (the arrays may be NULL when n == 0), an align that is not a power of two
 * in [1, 128], an out_arena that is not 16-B aligned, order / n_order not both set or both NULL.
 * n == 0 writes out_off[0] = 0 and *total = 0.
 * Scratch: 8 B per 1024 packets per stream (rsk_reserve_stream sizes it, so a call captured into a
 * hipGraph after a reserve replays correctly: the launches are a linear chain and keep no host state). */
typedef struct rsk_deliver_in {
    const uint8_t  *arena;     /* device bytes the frames lie in: rsk_decode_batch's frame_arena,
                                  rsk_parse_decode_batch's cap_arena, rsk_syncinput_decode_batch's rec_arena */
    const uint64_t *base_off;  /* [n] frame_off / cap_off / rec_off                                  */
    const uint16_t *inner_off; /* [n] tcp->cap_pay_off (frame start inside the capture / record), or NULL = 0 */
    const uint16_t *pay_off;   /* [n] dec->pay_off                                                    */
    const uint16_t *pay_len;   /* [n] dec->pay_len                                                    */
    const int8_t   *status;    /* [n] dec->status; only RSK_RECV_VALID packets carry bytes            */
    const uint32_t *order;     /* [*n_order] packet indices in delivery order: demux perm, or a decode's
                                  valid_idx; NULL = 0..n-1                                            */
    const uint32_t *n_order;   /* [1] device count (demux / decode n_valid); must be NULL iff order is */
} rsk_deliver_in;
typedef struct rsk_deliver_out {
    uint8_t  *out_arena; /* device, 16-B aligned; NULL = plan only (offsets and total, no copy)       */
    uint64_t  out_cap;   /* bytes available at out_arena                                              */
    uint64_t *out_off;   /* [n+1] out_off[k] = start of the k-th delivered payload                    */
    uint64_t *total;     /* [1] bytes needed (may be NULL)                                            */
    uint32_t  align;     /* power of two in [1,128]: every payload starts at a multiple of it          */
} rsk_deliver_out;
int rsk_deliver_batch(rsk_ctx *ctx, uint32_t n, const rsk_deliver_in *in, const rsk_deliver_out *out,
                      void *stream);
/* Host twin (host pointers throughout; nthreads <= 1 runs on the caller's thread): the same offsets
 * and bytes for host-resident deployments whose payloads never left host memory (the header-only
 * batches above). */
int rsk_deliver_host(uint32_t n, const rsk_deliver_in *in, const rsk_deliver_out *out, int nthreads);

/* ---- checksum verification of captured packets --------------------------------------------------- */
/* rsock's fake-TCP segments reach RawTcp::RawInput (conn/RawTcp.cpp:138-237) through libpcap, before
 * the kernel's TCP input path has verified or dropped them, and the frame's tag covers payload[0]
 * only.  rsk_verify_wire_batch checks the IPv4 header checksum and the TCP checksum of every captured
 * packet -- the other half of rsk_encode_wire_batch, which fills both in.  It belongs behind the
 * capture filter and the parse: parse_decode -> verify(status = dec->status, status_out =
 * dec->status) -> demux -> deliver.  (Packets a host sends itself with checksum offload are captured
 * with unfinished checksums and fail the check.)
 *
 * Packet i is the c = cap_len[i] bytes at p = cap_arena + cap_off[i]; L = 14 (RSK_DLT_EN10MB), 4
 * (RSK_DLT_NULL) or 0 (RSK_DLT_RAW); integers big-endian unless stated.
 *   0. in->status given and status[i] != RSK_RECV_VALID: csum[i] = 0, no byte of the packet is read.
 *   1. Link: EN10MB needs c >= 14 and p[12..13] == 08 00; NULL needs c >= 4 and the little-endian
 *      u32 at p == 2; RAW has no link check.  Otherwise csum[i] = 0.
 *   2. Header: c >= L + 20, p[L] >> 4 == 4, ihl = p[L] & 15 >= 5, H = 4 * ihl, c >= L + H.
 *      Otherwise csum[i] = 0.
 *   3. IP_CHECKED is set; IP_OK iff the ones'-complement sum of the header's H / 2 halfwords folds
 *      to 0xFFFF.
 *   4. TCP is attempted iff p[L + 9] == 6, (u16 at p + L + 6) & 0x3FFF == 0 (MF clear, fragment
 *      offset 0) and tot = u16 at p + L + 2 >= H + 20; otherwise no TCP bit is set.
 *   5. L + tot > c: TCP_TRUNC is set and neither other TCP bit.
 *   6. Otherwise, with T = tot - H: TCP_CHECKED is set; TCP_OK iff the source and destination address
 *      halfwords + 6 + T + the halfwords of the T segment bytes (an odd last byte taken as the high
 *      byte) fold to 0xFFFF.  The data offset is not consulted: the checksum covers the whole segment.
 *      The TCP check runs whether or not IP_OK is set.
 * Bytes at or past p + L + tot (Ethernet trailer padding, the next packet) are never summed, and
 * cap_len bounds every read: no 16-B aligned chunk without a byte of [p, p + c) is loaded, so the arena
 * may end at the last packet's last byte.  A field that holds 0xFFFF where 0x0000 is correct still
 * folds to 0xFFFF and is accepted, as Linux accepts it.
 * A packet is bad iff (IP_CHECKED && !IP_OK) || (TCP_CHECKED && !TCP_OK); "not checkable" is never
 * bad (the caller reads csum to be stricter).  status_out[i] = RSK_RECV_DROP when status[i] ==
 * RSK_RECV_VALID and the packet is bad, else status[i]; *n_bad = the number of bad packets (written,
 * not accumulated).
 * RSK_EINVAL: a NULL ctx, in or out; a NULL csum, cap_arena, cap_off or cap_len with n > 0; status_out
 * without in->status; a datalink outside {RSK_DLT_NULL, RSK_DLT_EN10MB, RSK_DLT_RAW}; n >
 * RSK_VERIFY_MAX_BATCH (8 work-items per packet in blocks of 256: a grid holds at most 2^32 - 1,
 * DESIGN.md §4.10).  n == 0 is a no-op that zeroes a given n_bad.
 * No scratch: one memset node (n_bad, when given) and one kernel, a linear chain that a hipGraph
 * captures without a reserve; no device-error bit is set. */
#define RSK_CSUM_IP_CHECKED  0x01u
#define RSK_CSUM_IP_OK       0x02u
#define RSK_CSUM_TCP_CHECKED 0x04u
#define RSK_CSUM_TCP_OK      0x08u
#define RSK_CSUM_TCP_TRUNC   0x10u /* the TCP segment runs past cap_len (snaplen): not checkable */
#define RSK_VERIFY_MAX_BATCH 0x1FFFFFE0u /* 2^29 - 32 */
typedef struct rsk_verify_in {
    const uint8_t  *cap_arena;  /* as rsk_parse_decode_batch                                          */
    const uint64_t *cap_off;    /* [n]                                                                */
    const uint32_t *cap_len;    /* [n]                                                                */
    const int8_t   *status;     /* [n] optional (dec->status): when set, only RSK_RECV_VALID packets are examined */
} rsk_verify_in;
typedef struct rsk_verify_out {
    uint8_t  *csum;        /* [n] RSK_CSUM_* bits, 0 = not examined / not IPv4                        */
    int8_t   *status_out;  /* [n] optional; requires in->status; may be the SAME pointer as in->status */
    uint32_t *n_bad;       /* [1] optional device count of bad packets (written, not accumulated)     */
} rsk_verify_out;
int rsk_verify_wire_batch(rsk_ctx *ctx, uint32_t n, const rsk_verify_in *in, int datalink,
                          const rsk_verify_out *out, void *stream);
/* Host twin (host pointers throughout; the same rule and outputs; nthreads as rsk_deliver_host; no
 * upper limit on n). */
int rsk_verify_wire_host(uint32_t n, const rsk_verify_in *in, int datalink, const rsk_verify_out *out, int nthreads);

/* ---- fake-TCP connection table: a packet's connection, a connection's TcpInfo -------------------- */
/* The level the reference keeps between the codec and the leaves: INetGroup's map from connKey to
 * INetConn (mConnMap, conn/INetGroup.cpp:57-83; one INetGroup per IdBuf on a server,
 * server/ServerGroup.cpp:44-60) and the TcpInfo mInfo of every FakeTcp in it (conn/FakeTcp.cpp:14-50,
 * conn/INetConn.cpp:30-39).  Here it is a table of `capacity` rows in caller-owned device columns plus
 * one opaque index, so a batch carries connection indices only:
 *   receive  parse_decode -> verify -> rsk_conn_resolve_batch -> conn[i], the conn / delivered columns of
 *            rsk_tcp_recv_ack_batch(conn, hit, tcp->seq, capacity, tab.ack)
 *   send     rsk_conn_pick_batch -> conn[i]; rsk_conn_expand_batch(conn) -> src, dst, sp, dp, ack, flag
 *            (rsk_wire_in) and conn_key, id (rsk_encode_in); seq and ip_id from rsk_tcp_send_seq_batch(conn, status, capacity, tab.seq, ...)
 * The host edits rows with ordinary copies on its streams and calls rsk_conn_index_build after any
 * change to state, conn_key or id (one rebuild over the capacity; this table's insert is rsk_conn_create_batch,
 * which makes the conns of a receive batch or a client's dials on the device, its erase rsk_conn_close_batch,
 * which kills and removes rows there; both keep both indexes current; the conv table has
 * rsk_conv_create_batch and rsk_conv_close_batch); an index that was not rebuilt after such a change gives lookups of
 * the changed keys an unspecified row or RSK_CONN_NONE, never an access outside the table.  The other
 * columns need no rebuild.  The arrays are the caller's and do not move, so a call captured into a
 * hipGraph sees later row edits and rebuilds.
 * The key of a row is its conn_key, or with RSK_CONN_BY_ID the pair (id, conn_key).  When two LIVE rows
 * hold one key the lowest row is the key's connection, whatever order the device ran them in. */
#define RSK_CONN_NONE     0xFFFFFFFFu
#define RSK_CONN_MAX_ROWS 0x100000u /* 2^20 */
#define RSK_CONN_BY_ID    0x1u   /* key = (IdBuf, connKey): a server, whose SNetGroup is per IdBuf
                                    (server/ServerGroup.cpp:44-60); without it connKey alone: a client */
#define RSK_CONN_LIVE     0x1u   /* state bit: the row holds a connection (it is in mConnMap)        */
#define RSK_CONN_ALIVE    0x2u   /* state bit: INetConn::Alive()                                     */

typedef struct rsk_conn_table {  /* device pointers, caller-owned, `capacity` rows */
    uint32_t capacity, flags;    /* capacity in [1, RSK_CONN_MAX_ROWS]; flags: RSK_CONN_BY_ID or 0   */
    const uint8_t  *state;       /* [C] RSK_CONN_LIVE | RSK_CONN_ALIVE | RSK_CONN_NEW bits */
    const uint64_t *conn_key;    /* [C] INetConn::mIntKey */
    const uint8_t  *id;          /* [C*8], 8-B aligned; BY_ID only, else may be NULL */
    const uint32_t *src, *dst;   /* [C] TcpInfo as stored */
    const uint16_t *sp, *dp;     /* [C] */
    uint32_t *seq, *ack;         /* [C] the conn_seq / conn_ack of rsk_tcp_send_seq_batch /
                                    rsk_tcp_recv_ack_batch with n_conn = capacity */
    const uint8_t  *flag;        /* [C] TcpInfo::flag used when sending */
    uint32_t *index;             /* opaque, rsk_conn_index_bytes(capacity, flags) bytes, 16-B aligned */
} rsk_conn_table;

/* Bytes of the index of a table (8 per row rounded up to a power of two, at least 16: an
 * open-addressing table over the LIVE rows that always keeps half of its entries free, so a lookup of
 * an absent key ends even when every row is LIVE); 0 for a capacity outside [1, RSK_CONN_MAX_ROWS] or
 * unknown flags. */
uint64_t rsk_conn_index_bytes(uint32_t capacity, uint32_t flags);
/* Rebuilds tab->index from state, conn_key (and id): two launches of one kernel on `stream`, the first
 * clearing the index, the second inserting the LIVE rows; *n_dup (device, may be NULL; written, not
 * accumulated) = the LIVE rows that lost their key to a lower row.  No scratch.  RSK_EINVAL: a NULL
 * ctx, tab, state, conn_key or index, id missing with BY_ID, unknown flags, a capacity outside
 * [1, RSK_CONN_MAX_ROWS], an index that is not 16-B aligned, an id column that is not 8-B aligned. */
int rsk_conn_index_build(rsk_ctx *ctx, const rsk_conn_table *tab, uint32_t *n_dup, void *stream);

/* Receive: INetGroup::Input's lookup, once per batch.  Packet i is looked up iff status[i] ==
 * RSK_RECV_VALID and cmd[i] == RSK_CMD_DATA (control packets never reach INetGroup::Input,
 * conn/IAppGroup.cpp:80-95): conn[i] = the LIVE row with its key (whether or not RSK_CONN_ALIVE is set:
 * Input does not ask Alive()), or RSK_CONN_NONE.  A packet that is not looked up gets conn NONE, hit 0,
 * miss DROP, and its key fields are not read.
 * `miss` is a status column of the looked-up packets whose key is unknown -- the ones the reference
 * answers with ERR_NO_CONN and a SendNetConnRst (conn/IAppGroup.cpp:80-87) on a client, with
 * CreateNetConn (server/SNetGroup.cpp:20-46) on a server: rsk_demux_batch(status = miss, ...,
 * RSK_DEMUX_ID | RSK_DEMUX_CONN_KEY) -- RSK_DEMUX_CONN_KEY alone on a client -- lists the distinct
 * missing keys in first-arrival order in seg_first, i.e. one reset per key, or the conns in the order
 * CreateNetConn would make them.
 * No scratch: one memset node (n_miss, when given) and one kernel, a linear chain that a hipGraph
 * captures without a reserve.  n == 0 zeroes a given n_miss.  RSK_EINVAL: a NULL ctx, tab, in or out;
 * a NULL status, conn_key or conn with n > 0; a NULL tab->conn_key or tab->index; id missing (in the
 * table or in `in`) with BY_ID, or one that is not 8-B aligned; unknown flags; a capacity outside
 * [1, RSK_CONN_MAX_ROWS]; n > RSK_MAX_BATCH. */
typedef struct rsk_conn_resolve_in {
    const int8_t   *status;    /* [n] dec->status */
    const uint8_t  *cmd;       /* [n] dec->cmd, or NULL = all DATA */
    const uint8_t  *id;        /* [n*8] dec->id (8-B aligned); required with BY_ID */
    const uint64_t *conn_key;  /* [n] dec->conn_key */
} rsk_conn_resolve_in;
typedef struct rsk_conn_resolve_out {
    uint32_t *conn;    /* [n] row, or RSK_CONN_NONE */
    uint8_t  *hit;     /* [n] optional: 1 iff conn[i] != NONE (the `delivered` of rsk_tcp_recv_ack_batch) */
    int8_t   *miss;    /* [n] optional: RSK_RECV_VALID iff looked up and not found, else RSK_RECV_DROP */
    uint32_t *n_miss;  /* [1] optional, written not accumulated */
} rsk_conn_resolve_out;
int rsk_conn_resolve_batch(rsk_ctx *ctx, const rsk_conn_table *tab, uint32_t n, const rsk_conn_resolve_in *in,
                           const rsk_conn_resolve_out *out, void *stream);

/* Send: what INetConn::Output and RawTcp::Output take from the connection the sender picked.  ok[i] = 1
 * iff conn[i] < capacity and the row is LIVE and ALIVE; then every given column receives the row's
 * value (ack as it is when the kernel runs: stream-ordered behind an earlier rsk_tcp_recv_ack_batch).
 * Otherwise ok[i] = 0 and every given column receives zero: the caller picked a dead conn, which the
 * reference's doSend drops before picking again (conn/INetGroup.cpp:111-135; the pick itself is
 * rsk_conn_pick_batch below, whose conn column never names such a row).  *n_bad = the packets with ok == 0 (written, not
 * accumulated).  No scratch, one memset node and one kernel, as the resolve.
 * RSK_EINVAL: a NULL ctx, tab, out or tab->state; a NULL conn or ok with n > 0; an output column whose
 * table column is NULL; an id column (the table's or out->id) that is not 8-B aligned when out->id is
 * given; unknown flags; a capacity outside [1, RSK_CONN_MAX_ROWS]; n > RSK_MAX_BATCH. */
typedef struct rsk_conn_expand_out {   /* every array optional except ok */
    uint32_t *src, *dst; uint16_t *sp, *dp; uint32_t *ack; uint8_t *flag;
    uint64_t *conn_key; uint8_t *id /*[n*8], 8-B aligned*/;
    uint8_t *ok;       /* [n] 1 iff conn[i] < capacity and the row is LIVE|ALIVE */
    uint32_t *n_bad;   /* [1] optional: packets with ok == 0 */
} rsk_conn_expand_out;
int rsk_conn_expand_batch(rsk_ctx *ctx, const rsk_conn_table *tab, uint32_t n, const uint32_t *conn,
                          const rsk_conn_expand_out *out, void *stream);

/* Host twins (host pointers throughout, the table's included; the same rules and outputs; nthreads as
 * rsk_deliver_host; the build takes it for symmetry and runs on the caller's thread).  The index has
 * one layout on both sides: one built here and copied to the device is valid there, and the reverse.
 * The host twins read the IdBuf columns bytewise and accept any alignment of them. */
int rsk_conn_index_build_host(const rsk_conn_table *tab, uint32_t *n_dup, int nthreads);
int rsk_conn_resolve_host(const rsk_conn_table *tab, uint32_t n, const rsk_conn_resolve_in *in,
                          const rsk_conn_resolve_out *out, int nthreads);
int rsk_conn_expand_host(const rsk_conn_table *tab, uint32_t n, const uint32_t *conn,
                         const rsk_conn_expand_out *out, int nthreads);

/* ---- the send pick: INetGroup::doSend's choice of a connection per outgoing packet ------------------ */
/* Between rsk_conv_send_batch (the head's conv, dst, id) and rsk_conn_expand_batch (the picked conn's
 * TcpInfo) the reference runs INetGroup::doSend (conn/INetGroup.cpp:111-135): per packet it draws
 * rand() % mConns.size(), walks to that conn and takes it if it is Alive(), and for a reset also if it is
 * not the conn named by keyOfConnToReset.  Here the draw is a column, so the pick is a pure function of
 * the table, the pick index and the batch.
 *   Groups.      On a table without RSK_CONN_BY_ID (a client) all rows form one group.  With it (a
 *                server) a group is the set of rows with one 8-byte id, one SNetGroup per IdBuf.  An id of
 *                eight zero bytes is an ordinary id.
 *   Candidates.  A group's rows with both RSK_CONN_LIVE and RSK_CONN_ALIVE, in ascending row order; m is
 *                their number.
 *   Packet i:
 *   1. It is taken iff len == NULL || len[i] > 0 (doSend's nread > 0).  A packet that is not taken gets
 *      conn[i] = RSK_CONN_NONE, is not counted, and none of its other fields are read.
 *   2. g = the group of id[i]; without BY_ID the one group, and id is not read.  No group with that id, or
 *      m == 0: conn[i] = RSK_CONN_NONE and the packet is counted in *n_none (the reference's ERR_NO_CONN).
 *   3. d = draw[i]; with draw == NULL, d = the upper 32 bits of word i of the splitmix64 stream of `seed`
 *      (the words rsk_fill_splitmix(seed) writes).
 *   4. a = avoid_key ? avoid_key[i] : 0.  If a != 0, let r be the row the table's conn index names for
 *      (id[i], a) -- the resolve's rule; a alone without BY_ID.  If r is a candidate of g, at position p,
 *      the pick runs over the other m - 1 candidates: m - 1 == 0 gives NONE, counted; otherwise
 *      k = d % (m - 1), k += (k >= p).  In every other case (a == 0, a key not in the index, a row that is
 *      no candidate, with BY_ID a key that exists only under another id) k = d % m.
 *   5. conn[i] = candidate k of g.  With `used` given ([capacity] bytes, zeroed by the caller when it wants)
 *      used[conn[i]] = 1: plain stores of one value, which tell the host where to clear RSK_CONN_NEW as
 *      INetConn::Output clears mNew.
 * Relation to the reference.  With every conn of a group alive and no avoid key (or one that names no conn
 * of the group) the reference takes element rand() % size of mConns: a table whose rows of a group stand in
 * mConns order, with draw[i] the i-th rand(), gives the reference's pick exactly.  mConns is a
 * std::map<std::string, IConn *> keyed by KeyGenerator::StrForIntKey(key) = std::to_string(key), so its
 * order is the lexicographic order of the keys' decimal strings ("10" < "100" < "9"), not their numeric
 * order: exactness is the caller's row layout, and with rows in any other order the picks are the same
 * distribution over other conns.  With dead conns the reference removes the dead one
 * and draws again: a rejection sampler, uniform over the same candidates, with the same modulo bias of
 * `%`; the distribution is the same, the number of draws consumed is not (a deliberate deviation, of the
 * kind of rsk_control_batch's snapshot semantics).  When the only alive conn is the one to avoid the
 * reference's loop never ends (`continue` at :122 without a removal); here the packet gets NONE and is
 * counted.  The table is seen as the pick index was last built (a snapshot): which rows are dead is the
 * host's knowledge already, because it edits `state`.  The reference learns it inside the walk: a conn that a
 * NETCONN_RST of the same batch marked dead is still a candidate here until rsk_conn_close_batch (behind the control
 * pass in the chain) or the host clears RSK_CONN_ALIVE and brings the pick index up to date, where the reference's
 * doSend would draw it, remove it and draw again.
 *
 * The pick index is a separate caller-owned buffer of rsk_conn_pick_bytes(capacity, flags) bytes, 16-B
 * aligned, rebuilt by the caller after any host change to state or id (as rsk_conn_index_build after its
 * columns; rsk_conn_close_batch keeps it current on the device when conns die); avoid keys also go through tab->index.  A stale or never-built pick index gives an unspecified
 * row of the table or RSK_CONN_NONE, never an access outside the table or the index.  It has one layout
 * on host and device: one built on either side and copied to the other is valid there. */
uint64_t rsk_conn_pick_bytes(uint32_t capacity, uint32_t flags);      /* 0 for a bad capacity / flags */
/* Builds `pick` from tab->state (and tab->id): a handful of launches on `stream`, set-up rate (one of
 * them walks the rows in order on a single block).  counts (device [2], may be NULL) receives the groups
 * that have a candidate and the candidates of the whole table.  No scratch and no host state, but it is
 * not meant for capture.  RSK_EINVAL: a NULL ctx, tab, tab->state or pick; id missing with BY_ID or not
 * 8-B aligned; unknown flags; a capacity outside [1, RSK_CONN_MAX_ROWS]; a pick index that is not 16-B
 * aligned. */
int rsk_conn_pick_build(rsk_ctx *ctx, const rsk_conn_table *tab, uint32_t *pick, uint32_t *counts, void *stream);
typedef struct rsk_conn_pick_in {
    const int32_t  *len;        /* [n] optional: the packet is taken iff len[i] > 0; NULL = all taken */
    const uint8_t  *id;         /* [n*8] the packet's IdBuf (8-B aligned); required with BY_ID, else not read */
    const uint64_t *avoid_key;  /* [n] optional: keyOfConnToReset, 0 = none (rsk_ctl_msgs.avoid_key) */
    const uint32_t *draw;       /* [n] optional: the draws; NULL = the splitmix64 stream of `seed` */
    uint64_t seed;
} rsk_conn_pick_in;
typedef struct rsk_conn_pick_out {
    uint32_t *conn;    /* [n] row, or RSK_CONN_NONE */
    uint32_t *n_none;  /* [1] optional, written not accumulated: taken packets without a conn */
    uint8_t  *used;    /* [capacity] optional: used[conn[i]] = 1 */
} rsk_conn_pick_out;
/* No scratch and no host state: one one-thread kernel (n_none, when given) and one kernel, a linear chain that a
 * hipGraph captures without a reserve.  n == 0 zeroes a given n_none.  RSK_EINVAL: a NULL ctx, tab, pick,
 * in or out; a NULL conn with n > 0; id missing (in the table, or in `in` with n > 0) with BY_ID, or one
 * that is not 8-B aligned; avoid_key given on a table whose conn_key or index is NULL; unknown flags; a
 * capacity outside [1, RSK_CONN_MAX_ROWS]; a pick index that is not 16-B aligned; n > RSK_MAX_BATCH. */
int rsk_conn_pick_batch(rsk_ctx *ctx, const rsk_conn_table *tab, const uint32_t *pick, uint32_t n,
                        const rsk_conn_pick_in *in, const rsk_conn_pick_out *out, void *stream);
/* Host twins (host pointers throughout; the same rule, outputs and index layout; the id columns at any
 * alignment; nthreads as rsk_deliver_host, the build runs on the caller's thread; no upper limit on n). */
int rsk_conn_pick_build_host(const rsk_conn_table *tab, uint32_t *pick, uint32_t *counts, int nthreads);
int rsk_conn_pick_host(const rsk_conn_table *tab, const uint32_t *pick, uint32_t n, const rsk_conn_pick_in *in,
                       const rsk_conn_pick_out *out, int nthreads);

/* ---- control packets and the keepalive timer on the connection table ------------------------------ */
/* Every packet that is not DATA is the reference's per packet: IAppGroup::Input branches on cmd
 * (conn/IAppGroup.cpp:76-96), ConnReset::Input (callbacks/ConnReset.cpp:43-90) and
 * NetConnKeepAlive::Input (callbacks/NetConnKeepAlive.cpp:37-98) read a 4- or 8-byte body, look the
 * body's key up in mConnMap and answer, report the conn or clear a pending request; a FIN / RST packet
 * (RSK_RECV_CLOSE) reaches IAppGroup::ProcessTcpFinOrRst (conn/IAppGroup.cpp:103-116).  The state they
 * touch is the table above, and NetConnKeepAlive::OnFlush (:110-145) is a pass over its rows.
 *   receive  parse_decode -> verify -> resolve -> rsk_control_batch -> rsk_conn_close_batch (the conns the batch
 *            killed) -> rsk_conn_pick_batch (a conn per message, with the messages' id and avoid_key) -> expand ->
 *            send_seq -> rsk_encode_wire_batch
 *   timer    rsk_keepalive_flush -> the same message columns, and the rows that timed out -> rsk_conn_close_batch
 *
 * rsk_control_batch classifies packet i, reads the body of a control packet at
 * arena + base_off[i] + inner_off[i] + pay_off[i], and looks its key up by the resolve's rule: the LIVE
 * row found by the index, whether or not ALIVE; with RSK_CONN_BY_ID the key is the pair (id[i], arg).
 *   kind              when                                         arg                      conn
 *   RSK_CTL_NONE      not VALID (and no examined CLOSE), cmd DATA  0                        NONE
 *   RSK_CTL_CONV_RST  cmd 1, pay_len >= 4                          LE32 of body[0..4)       NONE (the lookup by
 *                                             BuildConvKey(dst, conv), ConnReset.cpp:67-77, stays above this level)
 *   RSK_CTL_NETCONN_RST cmd 2, pay_len >= 8                        LE64 of body[0..8)       row (OnRecvNetConnRst ->
 *                                             NotifyErr(ERR_FIN_RST), :79-90) or NONE
 *   RSK_CTL_KA_REQ    cmd 3, pay_len >= 8                          LE64                     row: answered with
 *                                             KEEP_ALIVE_RESP; NONE: answered with NETCONN_RST (:41-48)
 *   RSK_CTL_KA_RESP   cmd 4, pay_len >= 8                          LE64                     row: RemoveRequest; NONE
 *   RSK_CTL_TCP_CLOSE status RSK_RECV_CLOSE, tcp_sp / tcp_dp       rsk_key_for_tcp(sp, dp)  row or NONE
 *                     given, table without BY_ID                   (KeyForConnInfo)
 *   RSK_CTL_SHORT     cmd 1-4, body shorter than above (the reference returns -1)   0       NONE
 *   RSK_CTL_UNKNOWN   VALID, cmd > 4                               0                        NONE
 * A CLOSE packet on a BY_ID table, or without the port columns, is RSK_CTL_NONE
 * (ServerGroup::OnTcpFinOrRst walks every SubGroup in map order: the host's).  Only the body bytes
 * [0, 4) / [0, 8) are read: no 16-B aligned chunk that holds none of them is loaded, and a packet of
 * kind NONE, SHORT, UNKNOWN or TCP_CLOSE has no frame byte read at all.
 *
 * Per-row effects, on caller-owned columns of `capacity` rows (both optional):
 *   rst_first[r]  the smallest packet index whose kind is NETCONN_RST or TCP_CLOSE and whose conn is r,
 *                 0xFFFFFFFF when there is none (the call fills the column on the stream, then takes
 *                 atomicMin);
 *   ka_tries[r]   (in/out, shared with rsk_keepalive_flush) set to RSK_KA_NONE by any KA_RESP whose conn is r.
 * SNAPSHOT SEMANTICS -- a deliberate deviation.  Every lookup of a call sees the table as last indexed.
 * The reference walks the packets one at a time.  A NETCONN_RST of key K that hit only marks the conn dead
 * (INetConn::NotifyErr, conn/INetConn.cpp:49-52): K stays in mConnMap and its later packets still find it --
 * a KEEP_ALIVE_REQ for K is answered with a RESP, a second reset notifies again -- until a doSend draws the
 * dead conn and removes it (conn/INetGroup.cpp:129-130) or the group's Flush does; from then on they see K
 * gone.  So in a batch that sends nothing (no message of this call, no other send of the group meanwhile)
 * every packet gets what the reference gives it; with sends, a packet at or before its row's rst_first
 * always does, and a later packet of that row does as long as no send has drawn the row.  rst_first is what
 * lets a caller redo the tail for the few rows concerned, and what rsk_conn_close_batch takes to kill those rows
 * before the answers are picked.  (tests/golden/control.npz holds the reference's
 * own walk, removals included.)
 *
 * Messages to send (rsk_ctl_msgs): an order-stable compacted list, in packet order, of
 *   - one message per KA_REQ: cmd KEEP_ALIVE_RESP, avoid_key 0 when it hit; cmd NETCONN_RST,
 *     avoid_key = arg when it missed; body = arg in both;
 *   - with in->miss given (the resolve's miss column), one NETCONN_RST with body = avoid_key =
 *     conn_key[i] for every other packet with miss[i] == RSK_RECV_VALID: the per-packet SendNetConnRst
 *     of conn/IAppGroup.cpp:84-86 (the demux-based "one reset per key" recipe above stays available).
 * Entry k: cmd[k]; body[k] (to be sent as 8 LE bytes); id[8k .. 8k+8) the packet's IdBuf (zeros without an
 * id column); src[k] the packet index; avoid_key[k] doSend's keyOfConnToReset, the conn the reset must
 * not travel on (0 = none, as the reference); pay_off[k] = 8k and pay_len[k] = 8 -- so the columns are an
 * rsk_encode_in as they stand with `body` as the payload arena; the conn the caller picks supplies
 * conn_key through rsk_conn_expand_batch, and conv is the caller's (the receiver branches on cmd before
 * it reads conv).  Every array holds n entries and is optional; n_msg is required when any array is
 * given.  *n_msg and *n_ctl (the packets whose kind is not NONE) are written, not accumulated.
 *
 * Three launches on `stream` behind the fill of a given rst_first (a kernel, so that a captured chain replays
 * it), a linear chain: per-tile counts, one block that scans them, and the pass
 * that classifies, gathers, probes and writes; no block waits on another.  Scratch: 8 B per 2048 packets
 * per stream, sized by rsk_reserve_stream, so a captured call replays.  n == 0 zeroes the given counts
 * and fills a given rst_first.  RSK_EINVAL: a NULL ctx, tab, in or out; a table a lookup cannot use (as
 * rsk_conn_resolve_batch); with n > 0 a NULL status, cmd, arena, base_off, pay_off or pay_len; id
 * missing with BY_ID; an id column (the table's with BY_ID, or in->id) that is not 8-B aligned; tcp_sp
 * and tcp_dp not both set or both NULL; miss without conn_key; a message array without n_msg;
 * n > RSK_MAX_BATCH. */
#define RSK_CONN_NEW 0x4u /* state bit: INetConn::mNew, set at creation and cleared by the host at the
                             conn's first send (rsk_keepalive_flush skips such a row) */
#define RSK_CTL_NONE        0
#define RSK_CTL_CONV_RST    1
#define RSK_CTL_NETCONN_RST 2
#define RSK_CTL_KA_REQ      3
#define RSK_CTL_KA_RESP     4
#define RSK_CTL_TCP_CLOSE   5
#define RSK_CTL_SHORT       6
#define RSK_CTL_UNKNOWN     7
#define RSK_KA_NONE 0xFFu               /* ka_tries: the row has no entry in mReqMap */
#define RSK_KA_REQUEST_DELAY_MS 15000u  /* NetConnKeepAlive::REQUEST_DELAY */
#define RSK_KA_MAX_RETRY 3u             /* NetConnKeepAlive::MAX_RETRY */

typedef struct rsk_control_in {
    const int8_t   *status;    /* [n] dec->status */
    const uint8_t  *cmd;       /* [n] dec->cmd */
    const uint8_t  *id;        /* [n*8] dec->id, 8-B aligned; required with BY_ID, else only copied to the messages */
    const uint64_t *conn_key;  /* [n] dec->conn_key (EncHead's); only read for the miss option */
    const uint16_t *pay_off;   /* [n] dec->pay_off */
    const uint16_t *pay_len;   /* [n] dec->pay_len */
    const uint8_t  *arena;     /* the bytes the frames lie in, as rsk_deliver_in */
    const uint64_t *base_off;  /* [n] */
    const uint16_t *inner_off; /* [n] or NULL = 0 */
    const uint16_t *tcp_sp, *tcp_dp; /* [n] the parse's TcpInfo ports, or both NULL */
    const int8_t   *miss;      /* [n] the resolve's miss column, or NULL */
} rsk_control_in;
typedef struct rsk_ctl_msgs {  /* every array optional; n_msg required when any is given */
    uint8_t  *cmd;        /* [m] */
    uint64_t *body;       /* [m] */
    uint8_t  *id;         /* [m*8], 8-B aligned */
    uint32_t *src;        /* [m] packet index (rsk_control_batch) or row (rsk_keepalive_flush) */
    uint64_t *avoid_key;  /* [m] */
    uint64_t *pay_off;    /* [m] 8k */
    uint16_t *pay_len;    /* [m] 8 (4 from rsk_conv_resolve_batch) */
    uint32_t *n_msg;      /* [1] */
} rsk_ctl_msgs;
typedef struct rsk_control_out {  /* every output optional */
    uint8_t  *kind;      /* [n] RSK_CTL_* */
    uint64_t *arg;       /* [n] */
    uint32_t *conn;      /* [n] row, or RSK_CONN_NONE */
    uint32_t *n_ctl;     /* [1] */
    uint32_t *rst_first; /* [capacity] */
    uint8_t  *ka_tries;  /* [capacity] in/out */
    rsk_ctl_msgs msgs;   /* m = n */
} rsk_control_out;
int rsk_control_batch(rsk_ctx *ctx, const rsk_conn_table *tab, uint32_t n, const rsk_control_in *in,
                      const rsk_control_out *out, void *stream);

/* NetConnKeepAlive::OnFlush (callbacks/NetConnKeepAlive.cpp:110-145) as one pass over the rows.
 * ka_tries[r] is the row's entry of mReqMap, RSK_KA_NONE when it has none.  Per row r, in this order:
 *   1. r is not LIVE: ka_tries[r] = RSK_KA_NONE (removeInvalidRequest); done with r.  With online == 0
 *      (mRouteObserver->Online() false, :111-114) nothing else runs for any row.
 *   2. can = !(state & RSK_CONN_NEW) && now_ms > est && (int32_t)(uint32_t)(now_ms - est) >=
 *      (int32_t)request_delay_ms, est = established_ms[r]: canSendRequest's `int df` (:168-178), its
 *      truncation of the 64-bit difference included, reproduced as-is.
 *   3. If can: had = tries != NONE; tries = had ? tries + 1 : 0; a KEEP_ALIVE_REQ is emitted iff !had or
 *      tries < max_retry.
 *   4. If tries != NONE and tries >= max_retry: tries = NONE and r is appended to dead_rows
 *      (onNetConnDead -> NotifyErr(ERR_TIMEOUT)).
 * Both lists are in row order, their counts written, not accumulated.  A message has cmd
 * KEEP_ALIVE_REQ, body = the row's conn_key, id = the row's IdBuf (zeros for a table without an id
 * column), src = r, avoid_key 0, pay_off 8k, pay_len 8; the arrays hold `capacity` entries.  The table's
 * state stays read-only: rsk_conn_close_batch(close_rows = dead_rows, n_close = n_dead) kills (and removes) the
 * dead rows on the device, or the host clears ALIVE for them and rebuilds when it removes them.  No
 * index is read.  The launches and the scratch are rsk_control_batch's (8 B per 1024 rows).
 * Against the reference's own OnFlush (tests/golden/control.npz) the requests, the timeouts and mReqMap
 * are the same per flush; the reference emits in mConns order (the keys' decimal strings), this pass in row
 * order.  One deviation, of the snapshot kind: the reference's requests travel through doSend while it
 * iterates, so a request carried by a conn that is still new clears that conn's mNew
 * (INetConn::Output) and, when the iteration reaches it later in the same flush, it is asked already;
 * here state is read as the call found it and that row is asked one flush later.
 * RSK_EINVAL: a NULL ctx, tab, ka, out, tab->state, tab->conn_key, ka_tries or established_ms; unknown
 * table flags or a capacity outside [1, RSK_CONN_MAX_ROWS]; max_retry outside [1, 254]; a message array
 * without n_msg, dead_rows without n_dead; an id column (the table's or msgs.id) that is not 8-B aligned
 * when msgs.id is given. */
typedef struct rsk_keepalive {
    uint8_t        *ka_tries;        /* [C] in/out */
    const uint64_t *established_ms;  /* [C] INetConn::EstablishedTimeStampMs() */
    uint64_t        now_ms;          /* OnFlush's timestamp */
    uint32_t        request_delay_ms;/* RSK_KA_REQUEST_DELAY_MS */
    uint32_t        max_retry;       /* RSK_KA_MAX_RETRY */
    uint32_t        online;          /* 0: only step 1 runs */
} rsk_keepalive;
typedef struct rsk_keepalive_out {
    rsk_ctl_msgs msgs;     /* m = capacity */
    uint32_t *dead_rows;   /* [C] optional */
    uint32_t *n_dead;      /* [1] required with dead_rows */
} rsk_keepalive_out;
int rsk_keepalive_flush(rsk_ctx *ctx, const rsk_conn_table *tab, const rsk_keepalive *ka,
                        const rsk_keepalive_out *out, void *stream);

/* Host twins (host pointers, the same rules and outputs, nthreads as rsk_deliver_host; the IdBuf
 * columns are read bytewise at any alignment). */
int rsk_control_host(const rsk_conn_table *tab, uint32_t n, const rsk_control_in *in, const rsk_control_out *out,
                     int nthreads);
int rsk_keepalive_flush_host(const rsk_conn_table *tab, const rsk_keepalive *ka, const rsk_keepalive_out *out,
                             int nthreads);

/* ---- conn close: fake-TCP conns killed and removed on the device table ------------------------------ */
/* The two steps the reference takes when a conn dies, on the connection table, so that neither chain goes
 * through the host:
 *   receive  resolve -> rsk_control_batch (rst_first) -> rsk_conn_close_batch (column form) -> rsk_conn_pick_batch -> ...
 *   timer    rsk_keepalive_flush (dead_rows, n_dead) -> rsk_conn_close_batch (list form) -> rsk_conn_pick_batch -> ...
 * KILL.  INetConn::NotifyErr sets mAlive = false (conn/INetConn.cpp:49-52; from ConnReset::OnRecvNetConnRst,
 * callbacks/ConnReset.cpp:79-90, IAppGroup::ProcessTcpFinOrRst, and the keepalive timeout,
 * callbacks/NetConnKeepAlive.cpp:110-145).  The conn stays in mConnMap: lookups still find it.
 * REMOVE.  INetGroup::childConnErrCb -> RemoveConn erases it from mConns and mConnMap
 * (conn/INetGroup.cpp:94-101, :138-146), reached from IGroup::Flush for every conn that is not alive
 * (conn/IGroup.cpp:81-111) and from doSend for the dead conn it drew (conn/INetGroup.cpp:129-130).
 *
 * Marks.  At most one of close_rows and rst_first is given; with neither, RSK_CONN_CLOSE_SWEEP is required (that
 * call is IGroup::Flush alone).  List form: the marked rows are the first min(*n_close, m_max) entries of
 * close_rows (*n_close is a device word the host need not read); entries >= capacity, entries naming a row that
 * is not LIVE and repeats mark nothing extra.  Column form: row r is marked iff rst_first[r] != 0xFFFFFFFF.  No
 * packet column is read or written in either form: the call takes no n.
 * Kill.  A marked row that is LIVE loses RSK_CONN_ALIVE; it is counted in *n_marked and listed in marked_rows
 * iff it had the bit.
 * Remove.  With RSK_CONN_CLOSE_REMOVE every marked LIVE row is removed; with RSK_CONN_CLOSE_SWEEP also every
 * LIVE row without ALIVE, the rows killed by an earlier call or by the host included.  A removed row loses
 * LIVE, ALIVE and RSK_CONN_NEW; its other state bits and every other column stay bytewise untouched.  It is
 * listed once in closed_rows (the host closes the socket, and on a client redials).  ka_tries of a removed row
 * is left to the next rsk_keepalive_flush, whose step 1 is removeInvalidRequest.
 * Both lists are in row order; their counts are written, not accumulated, and nothing behind them is written.
 * State is written through rows->state, which must alias tab->state.
 * Conn index.  After a call that removed something every lookup gives what rsk_conn_index_build over the new
 * state gives: the index is rebuilt over the rows that stay (open addressing without tombstones has no erase
 * in place).  After a call that removed nothing no byte of tab->index is written: a kill alone never touches
 * it, as the reference's lookups still find a dead conn.
 * Pick index (out->pick, optional).  Precondition: it was current for the state the call found (built by
 * rsk_conn_pick_build, or kept by earlier calls of this function).  Afterwards every rsk_conn_pick_batch result
 * equals the result on an index freshly built over the new state, for any id, draw and avoid key, and so do
 * the header words and pick_counts (written by every call that has `pick`; not looked at without it).  The bytes may differ: a group that lost every
 * candidate keeps its entry, with an offset that the pick's bounds turn into NONE, and `lead` keeps what the
 * build left.  When no row lost ALIVE or LIVE no byte of it is written.  The update is a parallel, order-stable
 * compaction of the candidates (a close only takes candidates away).  Every value read from the pick index is
 * bounded before it is used as an offset: a stale or garbage index gives an unspecified index again, and never
 * an access outside the index, work or the table.
 * work: rsk_conn_close_bytes(capacity, table flags) bytes, 16-B aligned, caller-owned, contents do not matter;
 * one per stream that runs the call.
 * Launches: a linear chain of kernels on `stream` and no memset node (list form: clear and scatter the marks;
 * per 1024-row tile the counts of the rows that lose ALIVE, of those that lose LIVE and of the candidates
 * that stay; two one-block scans of the tile counts; one launch for the two lists, the clear of the conn index
 * and the scatter of the staying candidates into work; one for the rows' state and their insertion, the copy
 * back into the pick index and its group entries).  The last two leave at once when no row lost ALIVE or LIVE.
 * No launch walks the rows on one block, no block waits on another, nothing spins, no block reads a region of
 * an index that another block of the same launch writes, and every probe loop is bounded by its table's size.
 * The per-tile counts live in the control path's per-stream scratch (rsk_reserve_stream before a capture); the
 * chain captures into a hipGraph and replays on edited columns.  A row's state byte is written by the one lane
 * that owns the row.
 * RSK_EINVAL: a NULL ctx, tab, rows, in, out or work; a table a lookup cannot use, or without state;
 * rows->state != tab->state; both mark sources given, or none without SWEEP; unknown flags; list form without
 * n_close; marked_rows without n_marked, closed_rows without n_closed; a work, index or pick that is not 16-B
 * aligned; an id column (BY_ID) that is not 8-B aligned; a capacity outside [1, RSK_CONN_MAX_ROWS]. */
#define RSK_CONN_CLOSE_REMOVE 0x1u  /* the marked rows are also removed (RemoveConn of named conns)   */
#define RSK_CONN_CLOSE_SWEEP  0x2u  /* every LIVE row without ALIVE is removed (IGroup::Flush)        */
uint64_t rsk_conn_close_bytes(uint32_t capacity, uint32_t table_flags); /* 0 for a bad capacity / flags */

typedef struct rsk_conn_rows { uint8_t *state; } rsk_conn_rows;   /* writable alias of tab->state */

typedef struct rsk_conn_close_in {
    const uint32_t *close_rows; /* [m_max] list form: e.g. rsk_keepalive_flush's dead_rows            */
    const uint32_t *n_close;    /* [1] list form: device word, e.g. its n_dead                        */
    uint32_t m_max;
    const uint32_t *rst_first;  /* [capacity] column form: rsk_control_batch's, as it left it         */
    void *work;                 /* rsk_conn_close_bytes(...) bytes, 16-B aligned, caller-owned        */
    uint32_t flags;             /* RSK_CONN_CLOSE_*                                                    */
} rsk_conn_close_in;

typedef struct rsk_conn_close_out {
    uint32_t *marked_rows, *n_marked;  /* rows that lost ALIVE in this call, row order; count written */
    uint32_t *closed_rows, *n_closed;  /* rows that lost LIVE in this call, row order; count written  */
    uint32_t *pick;                    /* optional: the table's pick index, kept current              */
    uint32_t *pick_counts;             /* [2] optional, as rsk_conn_pick_build's counts               */
} rsk_conn_close_out;

int rsk_conn_close_batch(rsk_ctx *ctx, const rsk_conn_table *tab, const rsk_conn_rows *rows,
                         const rsk_conn_close_in *in, const rsk_conn_close_out *out, void *stream);
/* The twin: host pointers, the same rules, outputs, work buffer and index layouts (a table closed on one side
 * and copied to the other is valid there); sequential on the caller's thread; the IdBuf column at any alignment. */
int rsk_conn_close_host(const rsk_conn_table *tab, const rsk_conn_rows *rows, const rsk_conn_close_in *in,
                        const rsk_conn_close_out *out, int nthreads);

/* ---- conn create: fake-TCP conns made on the device table ------------------------------------------- */
/* INetGroup::Input's miss path (conn/INetGroup.cpp:57-83): ConnOfIntKey fails, SNetGroup::CreateNetConn
 * (server/SNetGroup.cpp:20-46) asks ServerNetManager::GetTcp (server/ServerNetManager.cpp:52-75) for the accepted
 * socket and the TcpAckPool record of the packet's 4-tuple, builds a FakeTcp from them, Init()s it, and AddNetConn
 * puts it into mConns and mConnMap; the packet that caused it, and every later packet of the key, is input to the
 * new conn.  A client never creates from a packet (client/CNetGroup.cpp:11-13 returns nullptr): its conns come
 * from DialTcpSync / DialTcpAsync followed by AddNetConn -- the list form.
 *   receive  resolve -> rsk_conn_create_batch -> rsk_tcp_recv_ack_batch -> rsk_control_batch ->
 *            rsk_conn_close_batch -> rsk_conn_pick_batch -> ...
 * Offers.  The host's join of the accepted sockets (ServerNetManager::mPool) and the harvested handshakes
 * (TcpAckPool): a caller-owned device list of m_max entries, the first min(*n_offer, m_max) in use (*n_offer is a
 * device word).  An offer has src, dst, sp, dp in the orientation of the parse's TcpInfo of a DATA packet of the
 * connection (the one FakeTcp is constructed with and the row stores), ack (the info.ack Wait2TransferInfo
 * leaves: the ack of the pooled record, which on a server is the th_seq of its own SYN|ACK, RawTcp.cpp:221-227)
 * and flag; no seq (FakeTcp::Init never reads it).  flag is the flag the conn SENDS with, not
 * the handshake's: the reference builds the conn's TcpInfo from the DATA packet's ConnInfo (server/SNetGroup.cpp:25,
 * bean/TcpInfo.cpp:55-58), Wait2TransferInfo transfers seq and ack only (net/TcpAckPool.cpp:45-53), so it is the
 * member default TH_ACK (bean/TcpInfo.h:15); an offer that carried the SYN row's flag would put SYN on every
 * packet of the conn.  It is matched by its 4-tuple alone
 * (TcpCmpFn keys both pools by src, sp, dst, dp); of two offers with one tuple the lower index is the tuple's.
 * What the host keeps around the call (the first handshake of a tuple wins, a refusal empties the tuple's pool
 * entries) is INTEGRATION.md's; tests/golden/conncreate.npz holds call and procedure to the reference's classes.
 * COLUMN FORM (flags without RSK_CONN_CREATE_LIST), behind rsk_conn_resolve_batch whose conn / hit / miss / n_miss
 * it continues; miss must be the resolve's (or an earlier call's) for the table as it is:
 *   1. The considered packets are the first u_max packets with miss[i] == RSK_RECV_VALID, in packet order; no
 *      other packet's key or tuple is read before step 8.
 *   2. K_0 .. K_{k-1} = their distinct keys (conn_key, or (id, conn_key) with BY_ID) in first-arrival order,
 *      f_j = the first considered packet of K_j.
 *   3. K_j is offered iff the tuple of packet f_j (src, dst, sp, dp columns) has an offer that no key with a lower
 *      f took and that was not consumed before (below).  Every other key is refused: it creates nothing, its
 *      packets stay in miss, it is counted in *n_refused (CreateNetConn returning nullptr; the reference hands
 *      such packets to mDefaultFakeConn).  DEVIATION: the reference retries CreateNetConn at every later packet
 *      of the key; this call looks at f_j only.  A key's packets share their ports, so the tuples agree unless a
 *      packet is forged.
 *   4. The offered keys, in first-arrival order, take the vacant rows (RSK_CONN_LIVE clear) v_0 < v_1 < ...:
 *      n_new = min(offered, vacant), n_full = the rest, whose offers are not consumed.
 *   5. A new row: state = LIVE | ALIVE | RSK_CONN_NEW (INetConn's mAlive, mNew); conn_key and id from packet f_j
 *      (the EncHead's key, never one made from the tuple: server/SNetGroup.cpp:29 records that bug); src, dst, sp,
 *      dp, flag from the offer; seq = offer.ack + 1 and ack = offer.ack + 2 modulo 2^32 (tests/golden/tcpstate.npz);
 *      with in->established_ms / in->ka_tries given, established_ms = now_ms and ka_tries = RSK_KA_NONE.  Every
 *      column of every other row stays bytewise untouched.
 *   6. Conn index: the new rows are inserted in place by rsk_conn_index_build's rule (compare-and-swap on a free
 *      entry, the lowest row of a key wins) in a later launch than the one that writes the rows; no rebuild.
 *      Bytes may differ from a rebuilt index, no lookup's result does.  A call that creates nothing writes no
 *      byte of tab->index.
 *   7. Pick index (out->pick, optional; precondition as rsk_conn_close_batch: current for the state found).
 *      Afterwards every rsk_conn_pick_batch result equals the result on an index freshly built over the new
 *      state, and so do the header words and pick_counts (written by every call that has `pick`).  A new row is
 *      a candidate of its group at its place in ascending row order.  A group without candidates (no entry, or
 *      one the close emptied) takes the first entry of its IdBuf's probe chain that is free or emptied, whichever
 *      IdBuf the emptied one held: entries are reused, so a table may see any number of IdBufs in its life and a
 *      group always finds an entry.  Probe chains only shorten again with rsk_conn_pick_build: once every entry
 *      has been used, a lookup of an IdBuf without candidates walks all of `group`; a server with heavy IdBuf
 *      churn rebuilds now and then.  The bytes may differ from a fresh
 *      build's (groups that had no candidate stand behind the others in cand).  When nothing was created no byte
 *      of it is written.  Every value read from it is bounded before use.
 *   8. Every packet of the batch with miss[i] == VALID whose key now resolves gets conn[i] = row, hit[i] = 1
 *      (when given) and miss[i] = RSK_RECV_DROP; *n_miss = the packets still missing; every other packet's
 *      columns stay untouched.  rsk_tcp_recv_ack_batch(conn, hit, ...) then advances the new rows' ack as
 *      FakeTcp::OnRecv does for the packet that created the conn.
 *   9. new_rows[j], new_first[j], new_offer[j] = the j-th new conn's row, first packet and offer;
 *      offer_row[o] = the row offer o became or RSK_CONN_NONE, over the first min(*n_offer, m_max) offers;
 *      *n_new, *n_full, *n_refused are written, not accumulated; nothing behind the lists' ends is written.
 *  10. Repeat calls.  With u_max below the missing packets the caller repeats while n_miss > 0 && n_full == 0 &&
 *      n_new > 0.  The consumed offers are LEFT IN PLACE and the later calls carry RSK_CONN_CREATE_REPEAT: then an
 *      offer whose offer_row entry is not RSK_CONN_NONE on entry was consumed, it still is its tuple's offer and
 *      refuses every key, and its entry is kept.  The sequence gives the rows and the conn column of one call
 *      with u_max >= n as long as each call's considered packets hold an offered key: packets of refused keys
 *      stay missing and are considered again, so u_max should exceed what a batch can hold of those.
 * LIST FORM (RSK_CONN_CREATE_LIST, n == 0, no packet columns): a client's dials and redials (AddNetConn after
 * DialTcpSync, the redial behind rsk_conn_close_batch's closed_rows), or a host that does the matching itself.
 * Every offer also has conn_key and, with BY_ID, id.  The first min(*n_offer, m_max) offers, in list order, that
 * carry a key not LIVE in the table and not carried by a lower offer take the vacant rows by 4-7 with the key
 * from the offer; the others are counted in *n_refused.  Outputs: offer_row, new_rows, new_offer, the counts.
 * work: rsk_conn_create_bytes(u_max, m_max, capacity, table flags) bytes, 16-B aligned, caller-owned, contents do
 * not matter, one per stream that runs the call.  With UI = max(u_max, m_max), M = min(m_max, capacity),
 * S(x) = the power of two >= 2 x (at least 4) and every term rounded up to 4, it is 4 * (16 + 2 * ceil(UI / 64) +
 * S(UI) + 2 UI + S(m_max) + 2 m_max + 10 M + S(M) + 2 * capacity) bytes: it depends on these values only.
 * Launches: a linear chain of kernels on `stream`, no host state and no memset node; it captures into a hipGraph
 * and replays on edited columns and offers.  Per-tile counts live in the control path's per-stream scratch
 * (rsk_reserve_stream before a capture).  No block waits on another, nothing spins, every probe loop is bounded
 * by its table's size, a row's state byte is written by the one lane that owns the row, no block reads a region
 * of an index that another block of the same launch writes.  When nothing is missing, or no missing packet
 * matches an offer, the later launches leave at once.  The order of the new candidates among the groups is a
 * rank over the new conns of the call computed by all blocks; no pass walks the capacity or n
 * on one block.  COST: on a RSK_CONN_BY_ID table with a pick index that rank takes n_new^2 key comparisons (spread
 * over the device): it grows with the square of the conns born in ONE call, 4.5 ms at 210 K on an MI355X against
 * 0.16 ms without BY_ID; a caller that bears more splits the call (u_max / m_max).
 * RSK_EINVAL: a NULL ctx, tab, rows, in, out or work; a table a lookup cannot use or without state, src, dst, sp,
 * dp, seq, ack or flag; a writable alias that is not the table's pointer; u_max 0 (column form) or above 2^24,
 * m_max 0 or above 2^21; unknown flags; column form with n > 0 and a NULL miss, conn, conn_key or tuple column, or
 * id missing with BY_ID; list form with n != 0, without the offers' conn_key, or without their id with BY_ID; a
 * NULL offer column or n_offer; new_rows, new_first or new_offer without n_new; REPEAT without offer_row; work,
 * index or pick not 16-B aligned, an id column not 8-B aligned; a capacity outside [1, RSK_CONN_MAX_ROWS];
 * n > RSK_MAX_BATCH. */
#define RSK_CONN_CREATE_LIST   0x1u  /* list form: the offers carry the keys, no packet columns            */
#define RSK_CONN_CREATE_REPEAT 0x2u  /* offer_row is in/out: an entry that names a row marks a consumed offer */
uint64_t rsk_conn_create_bytes(uint32_t u_max, uint32_t m_max, uint32_t capacity, uint32_t table_flags); /* 0: bad */

typedef struct rsk_conn_create_rows {  /* writable aliases of the table's columns */
    uint8_t *state; uint64_t *conn_key; uint8_t *id; uint32_t *src, *dst; uint16_t *sp, *dp;
    uint32_t *seq, *ack; uint8_t *flag;
} rsk_conn_create_rows;

typedef struct rsk_conn_offers {
    const uint32_t *src, *dst;   /* [m_max] */
    const uint16_t *sp, *dp;     /* [m_max] */
    const uint32_t *ack;         /* [m_max] info.ack behind Wait2TransferInfo */
    const uint8_t  *flag;        /* [m_max] */
    const uint64_t *conn_key;    /* [m_max] list form only */
    const uint8_t  *id;          /* [m_max*8], 8-B aligned; list form with BY_ID only */
    const uint32_t *n_offer;     /* [1] device word */
    uint32_t m_max;
} rsk_conn_offers;

typedef struct rsk_conn_create_in {
    const uint8_t  *id;          /* [n*8] dec->id, 8-B aligned; BY_ID */
    const uint64_t *conn_key;    /* [n] dec->conn_key */
    const uint32_t *src, *dst;   /* [n] the parse's TcpInfo */
    const uint16_t *sp, *dp;     /* [n] */
    rsk_conn_offers offers;
    uint32_t u_max;              /* considered packets per call */
    uint32_t flags;              /* RSK_CONN_CREATE_* */
    uint64_t now_ms;
    uint64_t *established_ms;    /* [capacity] optional */
    uint8_t  *ka_tries;          /* [capacity] optional */
    void *work;
} rsk_conn_create_in;

typedef struct rsk_conn_create_out {
    uint32_t *conn;  uint8_t *hit;  int8_t *miss;  uint32_t *n_miss;  /* the resolve's, continued (column form) */
    uint32_t *new_rows, *new_first, *new_offer;   /* [min(m_max, capacity)] optional; new_first column form only */
    uint32_t *offer_row;                          /* [m_max] optional */
    uint32_t *n_new, *n_full, *n_refused;         /* [1] optional */
    uint32_t *pick, *pick_counts;                 /* as rsk_conn_close_out */
} rsk_conn_create_out;

int rsk_conn_create_batch(rsk_ctx *ctx, const rsk_conn_table *tab, const rsk_conn_create_rows *rows, uint32_t n,
                          const rsk_conn_create_in *in, const rsk_conn_create_out *out, void *stream);
/* The twin: host pointers, the same rules and outputs, the same work size (it need not use it) and index
 * layouts: a table created on one side and copied to the other is valid there; sequential on the caller's
 * thread; the id columns bytewise at any alignment. */
int rsk_conn_create_host(const rsk_conn_table *tab, const rsk_conn_create_rows *rows, uint32_t n,
                         const rsk_conn_create_in *in, const rsk_conn_create_out *out, int nthreads);

/* ---- tuple pool: TcpAckPool and the accepted-socket pool kept on the device ------------------------- */
/* What feeds rsk_conn_create_batch's offers on a server: TcpAckPool::mInfoPool (net/TcpAckPool.cpp), the handshakes
 * RawInput harvested, and ServerNetManager::mPool (server/ServerNetManager.cpp), the accepted sockets nobody has
 * asked for yet; both std::maps keyed by the 4-tuple (TcpCmpFn: src, sp, dst, dp).  One type serves both: caller-
 * owned device columns of `capacity` rows (capacity in [1, RSK_CONN_MAX_ROWS]) and an index of
 * rsk_conn_index_bytes(capacity, RSK_CONN_BY_ID) bytes, 16-B aligned, with the layout, hash and probe rule of the
 * conn index, keyed by (src << 32 | dst, sp << 16 | dp) as the create's offers are hashed: an index built on either
 * side is valid on the other.  A row is in the pool iff state has RSK_POOL_LIVE.  The ack pool holds its tuples in
 * the orientation of a DATA packet's TcpInfo (the parse with RSK_PARSE_IS_SERVER reverses a SYN's, RawTcp.cpp:
 * 221-227) with the stored seq / ack; the socket pool has no use for seq / ack (both may be NULL there).  expiry is
 * the reference's `now + PersistMs` of the entry, in the caller's clock.
 *   receive  parse -> rsk_pool_add_batch (ack pool, TOUCH) ; accepted sockets -> rsk_pool_add_batch (socket pool)
 *            rsk_pool_offers -> resolve -> rsk_conn_create_batch -> rsk_tcp_recv_ack_batch -> rsk_pool_settle_batch
 *   timer    rsk_pool_flush on either pool
 * The host reads counts and row lists behind the batch (to bind sockets to the new conns and to close sockets);
 * the socket objects themselves stay the host's, one per socket-pool row.  Every call is a linear chain of kernels
 * on `stream` without host state or memset nodes; per-tile counts live in the control path's per-stream scratch
 * (rsk_reserve_stream before a capture); every call captures into a hipGraph and replays on edited columns.  No
 * block waits on another, nothing spins, every probe loop is bounded by its table's size, every value read from an
 * index or a list is bounded before use, a row's state byte is written by the one lane that owns the row, no pass
 * walks n or a capacity on one block.  Counts are written, not accumulated; nothing behind a list's end is written.
 *
 * rsk_pool_index_build / _host: the index over the LIVE rows, after host edits (as rsk_conn_index_build; *n_dup
 * optional: LIVE rows whose tuple a lower LIVE row holds).  RSK_EINVAL: a NULL ctx or pool, a NULL state, tuple
 * column, expiry or index, an index not 16-B or an expiry not 8-B aligned, a capacity out of range.
 *
 * rsk_pool_add_batch: TcpAckPool::AddInfoFromPeer (net/TcpAckPool.cpp:17-33) for the parse's SYN rows, and
 * ServerNetManager::add2Pool (server/ServerNetManager.cpp:105-117) for a list of accepted tuples.
 *   1. Considered: with parse_status given the rows with parse_status[i] == RSK_PARSE_SYN (the columns are the
 *      parse's rsk_tcpinfo_out as they lie on the device), without it every row (the list form).
 *   2. A considered row with sp == 0 or dp == 0 is dropped and counted in *n_zero_port (the pool refuses it,
 *      although the parse reports it).
 *   3. Of the first u_max remaining rows: a tuple that is LIVE in the pool keeps its row and its seq / ack -- the
 *      first handshake wins; with RSK_POOL_TOUCH (the ack pool: every AddInfoFromPeer moves the expiry) its expiry
 *      becomes in->expiry, without it (the socket pool, whose emplace changes nothing) it stays.
 *   4. The distinct tuples that are not LIVE take the vacant rows, lowest first, in first-arrival order, each with
 *      the columns of its first arrival (seq / ack where the pool has them), expiry = in->expiry, state = LIVE.
 *      n_new = min(distinct, vacant); *n_full = the rest (DEVIATION: the reference's map is unbounded);
 *      *n_again = the rows of step 3 whose tuple was LIVE already or arrived earlier in the call.
 *   5. The new rows go into the index by compare-and-swap in a later launch than the one that writes the rows; the
 *      index is never rebuilt, and a call that adds nothing writes no byte of it.
 *   6. row[i] (optional, [n]) = the row the tuple of input i has after the call for a row that passed step 2
 *      (whether or not it was among the first u_max), RSK_CONN_NONE for every other and for a tuple without a row;
 *      new_rows[j] / new_first[j] (optional, [min(u_max, capacity)]) = the j-th new row and its first arrival.
 * work: rsk_pool_add_bytes(u_max, capacity) bytes, 16-B aligned, caller-owned, contents do not matter, one per
 * stream that runs the call.  RSK_EINVAL: a NULL ctx, in, out or work; a pool as for rsk_pool_index_build; flags
 * other than RSK_POOL_TOUCH; u_max 0 or above 2^24; n > 0 with a NULL tuple column, or a NULL seq / ack where the
 * pool has that column; new_rows or new_first without n_new; work not 16-B aligned; n > RSK_MAX_BATCH.
 *
 * rsk_pool_offers: the join GetTcp (server/ServerNetManager.cpp:52-75) and Wait2TransferInfo (net/TcpAckPool.cpp:
 * 35-60) make per miss, ahead of time.  Every LIVE row of the ack pool whose tuple is LIVE in the socket pool makes
 * one offer, in ascending ack-pool row order, into columns laid out as rsk_conn_offers (m_max entries): src, dst,
 * sp, dp of the record; ack = the record's ack, never its seq; flag = RSK_TH_ACK, never the handshake's; conn_key
 * (optional) = rsk_key_for_tcp(sp, dp), for a client, which harvests without RSK_PARSE_IS_SERVER, adds its dialled
 * tuples to the socket pool and hands the offers to the create's list form.  offer_ack_row[o] / offer_sock_row[o]
 * (optional, [m_max]) = the two rows of offer o; *n_offer = min(matches, m_max); *n_over (optional) = the matches
 * beyond m_max, which are not offered.  expiry is not consulted: neither GetTcp nor Wait2TransferInfo looks at it,
 * an entry lives until a flush removes it.  RSK_EINVAL: a NULL ctx, pool or out; pools as above, the ack pool also
 * without seq or ack; m_max 0 or above 2^21; a NULL src, dst, sp, dp, ack, flag or n_offer; conn_key not 8-B aligned.
 *
 * rsk_pool_settle_batch: what becomes of the pools behind the batch.
 *   (a) For j < min(*n_new, new_max): both rows of offer new_offer[j] (the create's output; offer_ack_row /
 *       offer_sock_row are rsk_pool_offers', m_max entries) leave their pools; taken_sock_rows[j] (optional,
 *       [new_max]) = the socket row, whose socket the host binds to the create's new_rows[j].
 *   (b) Then every packet with miss[i] == RSK_RECV_VALID (the create's miss: a packet CreateNetConn refused) is
 *       taken by its tuple as the pools stand after (a).  LIVE in both pools: nothing happens, a whole offer this
 *       call did not consume stays (a full table, or the create's documented deviation).  Otherwise whichever entry
 *       exists is removed (GetTcp erases the socket it finds, Wait2TransferInfo the record).  Removed socket rows
 *       are listed once each in row order in closed_sock_rows ([capacity of the socket pool], optional) /
 *       *n_closed, for the host to close; *n_purged_ack = the ack-pool rows (b) removed.
 *   The outcome does not depend on packet order: (b) decides from state and the marks of (a) alone, equal lanes
 *   write equal marks, and LIVE is cleared by the lane that owns the row in a later launch.  Afterwards every
 *   lookup gives what a rebuild over the new state gives: each pool that lost a row is rebuilt over the rows that
 *   stay; a pool that lost none has no byte of its index written.
 * work: rsk_pool_settle_bytes(capacity of the ack pool, of the socket pool) bytes, 16-B aligned, contents do not
 * matter.  RSK_EINVAL: a NULL ctx, pool, in, out or work; pools as above; m_max 0 or above 2^21, new_max above 2^21;
 * new_max > 0 with a NULL new_offer, n_new, offer_ack_row or offer_sock_row; n > 0 with a NULL miss or tuple column;
 * closed_sock_rows without n_closed; work not 16-B aligned; n > RSK_MAX_BATCH.
 *
 * rsk_pool_flush: TcpAckPool::OnFlush (net/TcpAckPool.cpp:85-95) and ServerNetManager::OnFlush
 * (server/ServerNetManager.cpp:82-103), both of which compare expiry <= now: the LIVE rows with expiry <= now_ms
 * leave the pool; dead_rows ([capacity], optional) lists them in row order, *n_dead counts them (the host closes
 * the sockets of a socket pool's); the index is rebuilt over the rows that stay only when a row left.  RSK_EINVAL:
 * a NULL ctx, pool or out; a pool as above; dead_rows without n_dead.
 *
 * The host twins take host pointers and the same rules, outputs, work sizes and index layouts; sequential. */
#define RSK_POOL_LIVE  0x1u  /* state bit: the row holds an entry of the pool                                  */
#define RSK_POOL_TOUCH 0x1u  /* add flag: a considered row of a LIVE tuple moves its expiry (the ack pool)     */
typedef struct rsk_pool {    /* device pointers, caller-owned, `capacity` rows */
    uint8_t  *state;         /* [C] RSK_POOL_LIVE */
    uint32_t *src, *dst;     /* [C] */
    uint16_t *sp, *dp;       /* [C] */
    uint32_t *seq, *ack;     /* [C] the record's; NULL in a socket pool */
    uint64_t *expiry;        /* [C] */
    uint32_t *index;         /* rsk_conn_index_bytes(capacity, RSK_CONN_BY_ID) bytes, 16-B aligned */
    uint32_t capacity;
} rsk_pool;
int rsk_pool_index_build(rsk_ctx *ctx, const rsk_pool *pool, uint32_t *n_dup, void *stream);
int rsk_pool_index_build_host(const rsk_pool *pool, uint32_t *n_dup, int nthreads);

uint64_t rsk_pool_add_bytes(uint32_t u_max, uint32_t capacity);  /* 0 for a bad u_max / capacity */
typedef struct rsk_pool_add_in {
    const uint32_t *src, *dst;   /* [n] */
    const uint16_t *sp, *dp;     /* [n] */
    const uint32_t *seq, *ack;   /* [n] where the pool has the column */
    const int8_t *parse_status;  /* [n] optional */
    uint64_t expiry;             /* now + PersistMs */
    uint32_t u_max;
    uint32_t flags;              /* RSK_POOL_TOUCH */
    void *work;
} rsk_pool_add_in;
typedef struct rsk_pool_add_out {  /* every field optional */
    uint32_t *row;                        /* [n] */
    uint32_t *new_rows, *new_first;       /* [min(u_max, capacity)] */
    uint32_t *n_new, *n_again, *n_full, *n_zero_port;  /* [1] */
} rsk_pool_add_out;
int rsk_pool_add_batch(rsk_ctx *ctx, const rsk_pool *pool, uint32_t n, const rsk_pool_add_in *in,
                       const rsk_pool_add_out *out, void *stream);
int rsk_pool_add_host(const rsk_pool *pool, uint32_t n, const rsk_pool_add_in *in, const rsk_pool_add_out *out,
                      int nthreads);

typedef struct rsk_pool_offers_out {
    uint32_t *src, *dst;         /* [m_max] */
    uint16_t *sp, *dp;           /* [m_max] */
    uint32_t *ack;               /* [m_max] */
    uint8_t  *flag;              /* [m_max] */
    uint64_t *conn_key;          /* [m_max] optional */
    uint32_t *n_offer;           /* [1] */
    uint32_t *offer_ack_row, *offer_sock_row;  /* [m_max] optional */
    uint32_t *n_over;            /* [1] optional */
    uint32_t m_max;
} rsk_pool_offers_out;
int rsk_pool_offers(rsk_ctx *ctx, const rsk_pool *ack_pool, const rsk_pool *sock_pool, const rsk_pool_offers_out *out,
                    void *stream);
int rsk_pool_offers_host(const rsk_pool *ack_pool, const rsk_pool *sock_pool, const rsk_pool_offers_out *out,
                         int nthreads);

uint64_t rsk_pool_settle_bytes(uint32_t cap_ack, uint32_t cap_sock);  /* 0 for a bad capacity */
typedef struct rsk_pool_settle_in {
    const uint32_t *new_offer;   /* [new_max] the create's */
    const uint32_t *n_new;       /* [1] the create's */
    const uint32_t *offer_ack_row, *offer_sock_row;  /* [m_max] rsk_pool_offers' */
    uint32_t new_max, m_max;
    const int8_t *miss;          /* [n] the create's */
    const uint32_t *src, *dst;   /* [n] the parse's TcpInfo */
    const uint16_t *sp, *dp;     /* [n] */
    void *work;
} rsk_pool_settle_in;
typedef struct rsk_pool_settle_out {  /* every field optional */
    uint32_t *taken_sock_rows;   /* [new_max] */
    uint32_t *closed_sock_rows;  /* [capacity of the socket pool] */
    uint32_t *n_closed, *n_purged_ack;  /* [1] */
} rsk_pool_settle_out;
int rsk_pool_settle_batch(rsk_ctx *ctx, const rsk_pool *ack_pool, const rsk_pool *sock_pool, uint32_t n,
                          const rsk_pool_settle_in *in, const rsk_pool_settle_out *out, void *stream);
int rsk_pool_settle_host(const rsk_pool *ack_pool, const rsk_pool *sock_pool, uint32_t n, const rsk_pool_settle_in *in,
                         const rsk_pool_settle_out *out, int nthreads);

typedef struct rsk_pool_flush_out {
    uint32_t *dead_rows;         /* [capacity] optional */
    uint32_t *n_dead;            /* [1] optional */
} rsk_pool_flush_out;
int rsk_pool_flush(rsk_ctx *ctx, const rsk_pool *pool, uint64_t now_ms, const rsk_pool_flush_out *out, void *stream);
int rsk_pool_flush_host(const rsk_pool *pool, uint64_t now_ms, const rsk_pool_flush_out *out, int nthreads);

/* ---- conv table: a DATA packet's conv, the convs' activity counts and their flush ------------------ */
/* The reference's last lookup before a payload reaches anybody: on a server SubGroup::OnRecv looks
 * BuildConvKey(info->dst, head->Conv()) up in the SubGroup of the packet's IdBuf (server/SubGroup.cpp:31-50,
 * server/ServerGroup.cpp:44-60); on a client ClientGroup::OnRecv looks head->Conv() up in mConvMap
 * (client/ClientGroup.cpp:65-80) and answers an unknown conv with SendConvRst (callbacks/ConnReset.cpp:34-41).
 * Each conv counts its packets (IConn::DataStat, conn/IConn.cpp:63-79: curr_in++ / curr_out++), and
 * IGroup::Flush (conn/IGroup.cpp:81-107) closes the convs that went quiet.  Here that level is a second
 * table of `capacity` rows in caller-owned device columns, with the rules of the connection table above:
 * the host edits rows with ordinary copies and calls rsk_conv_index_build after any change to state,
 * conv, dst or id; the counter columns need no rebuild.  The two exceptions are rsk_conv_create_batch below,
 * which writes the rows of the convs born in a batch and inserts them into the index in place, and
 * rsk_conv_close_batch, which clears LIVE for the convs that a reset or the timer closes and leaves the index
 * without them; the host's clear LIVE and rebuild stays available for any other edit.
 *   receive  ... -> rsk_conn_resolve_batch (hit) -> rsk_control_batch (kind, arg) -> rsk_conv_resolve_batch
 *            -> conv_row[i] (-> rsk_conv_create_batch -> rsk_conv_close_batch -> rsk_conv_create_batch on a
 *            server); rsk_demux_batch / rsk_deliver_batch hand the bytes to the rows
 *   send     rsk_conv_send_batch(conv_row) -> conv, dst, id (rsk_encode_in) -> ... encode ... ->
 *            rsk_conv_send_batch(conv_row, sent = the encode's status) counts what was sent
 *   timer    rsk_conv_flush -> the rows to close -> rsk_conv_close_batch
 * The key of a row is the 64-bit word ((uint64_t)dst << 32) | conv with RSK_CONV_BY_DST, else conv; with
 * RSK_CONV_BY_ID it is paired with the row's IdBuf word (injective, as the reference's "conv:ip:conv"
 * string inside one SubGroup is).  A client is flags 0, a server both; any combination is valid.  The
 * index has the layout, hash and probe rule of the connection table's: rsk_conn_index_bytes(capacity, 0)
 * sizes it, one built on the host is valid on the device and the reverse, the lowest LIVE row of a key
 * wins. */
#define RSK_CONV_BY_DST 0x1u /* the key includes the TcpInfo dst: a server's SubGroup               */
#define RSK_CONV_BY_ID  0x2u /* one key space per IdBuf: a server's SubGroups                        */

typedef struct rsk_conv_table {  /* device pointers, caller-owned, `capacity` rows */
    uint32_t capacity, flags;    /* capacity in [1, RSK_CONN_MAX_ROWS]; RSK_CONV_BY_DST | RSK_CONV_BY_ID */
    const uint8_t  *state;       /* [C] RSK_CONN_LIVE = the row is in mConns */
    const uint32_t *conv;        /* [C] */
    const uint32_t *dst;         /* [C] BY_DST only (also what rsk_conv_send_batch hands out) */
    const uint8_t  *id;          /* [C*8], 8-B aligned; BY_ID only (also for rsk_conv_send_batch) */
    uint32_t *cur_in, *cur_out;  /* [C] DataStat::curr_in / curr_out; wrap mod 2^32 as the reference's uint32_t */
    uint32_t *prev_in, *prev_out;/* [C] DataStat::prev_in / prev_out */
    uint8_t  *alive;             /* [C] DataStat::mAlive; the host sets 1 when it creates a row */
    uint32_t *index;             /* opaque, rsk_conn_index_bytes(capacity, 0) bytes, 16-B aligned */
} rsk_conv_table;

/* As rsk_conn_index_build: two launches of the same kernel (clear, insert the LIVE rows), no scratch, no
 * incremental insert (that is rsk_conv_create_batch); *n_dup (device, optional, written) = the LIVE rows that lost their key to a lower
 * row.  RSK_EINVAL: a NULL ctx, tab, state, conv or index; dst / id missing with their flag; unknown
 * flags; a capacity outside [1, RSK_CONN_MAX_ROWS]; an index that is not 16-B aligned; an id column
 * that is not 8-B aligned. */
int rsk_conv_index_build(rsk_ctx *ctx, const rsk_conv_table *tab, uint32_t *n_dup, void *stream);

/* Receive.  Per packet i:
 *   DATA      examined iff status[i] == RSK_RECV_VALID && cmd[i] == RSK_CMD_DATA && (hit == NULL || hit[i])
 *             (a client packet of an unknown connKey never reaches ClientGroup::OnRecv: INetGroup::Input
 *             returns ERR_NO_CONN first).  conv_row[i] = the LIVE row of (id[i], dst[i], conv[i]) -- each
 *             part only with its flag -- or RSK_CONN_NONE.  With tab->cur_in given, every examined packet
 *             that found row r adds 1 to cur_in[r] (IConn::Input -> afterInput(n > 0); a VALID packet has
 *             pay_len >= 1).  The sums are exact whatever the skew -- all of a batch on one row, or every
 *             packet on another row -- and equal rows are combined on chip: no global atomic per packet.
 *   CONV_RST  with ctl_kind / ctl_arg given (rsk_control_batch's kind / arg; both or neither), a packet
 *             that is not examined and whose kind is RSK_CTL_CONV_RST is looked up as (id[i], dst[i],
 *             (uint32_t)ctl_arg[i]) on a table with RSK_CONV_BY_DST: conv_row[i] = the row or NONE, and
 *             rst_first[r] (optional, [capacity]; filled with 0xFFFFFFFF on the stream, then atomicMin) =
 *             the smallest such packet index that hit r: OnRecvConvRst -> CloseConn.  It adds nothing to
 *             cur_in.  On a table WITHOUT RSK_CONV_BY_DST (a client) a CONV_RST never hits: conv_row
 *             NONE, no rst_first.  Reproduced as-is from the reference, where ClientGroup keys mConns by
 *             CConn::BuildKey(addr) (a decimal number or a socket path) while OnRecvConvRst asks for
 *             "conv:..." (callbacks/ConnReset.cpp:67-77; the reference's own todo at server/SubGroup.cpp:38
 *             names the mismatch).
 *   else      conv_row NONE.  The key fields (conv, dst, id, ctl_arg) of a packet that is not looked up
 *             are never read.
 * unknown[i] (optional status column) = RSK_RECV_VALID iff examined and not found, else RSK_RECV_DROP;
 * *n_unknown is written, not accumulated.  rsk_demux_batch(status = unknown, ..., RSK_DEMUX_ID |
 * RSK_DEMUX_DST | RSK_DEMUX_CONV) lists the distinct new keys in first-arrival order in seg_first: the
 * order SubGroup::newConn makes them on a server.
 * Messages (out->msgs; n_msg required with any array, arrays of n entries): one per unknown packet,
 * order-stable, in packet order: cmd RSK_CMD_CONV_RST, body = conv, pay_len 4 (encode_uint32), pay_off 8k,
 * id = the packet's IdBuf (zeros without an id column), src = i, avoid_key 0 (doSendCmd -> Send ->
 * doSend(..., 0)) -- an rsk_encode_in as they stand.  This is the client's per-packet SendConvRst; a
 * server, which creates a conv instead, leaves the messages out.  *n_msg = *n_unknown.
 * SNAPSHOT SEMANTICS, as rsk_control_batch: every lookup sees the table as last indexed; a packet at or
 * before its row's rst_first gets what the reference gives it, and rst_first lets the caller redo the
 * tail; a conv the host creates from `unknown` exists from the next rebuild on.
 * Launches: without a list or a count, memset nodes, the fill of a given rst_first (a kernel, so that a captured
 * chain that reads rst_first again replays exactly) and one kernel.  With msgs / n_unknown the kernel
 * also leaves its tile's number of unknown packets in the control path's per-stream scratch (sized by
 * rsk_reserve_stream), one block scans them, and a third launch writes the list from conv_row's verdicts
 * (the probes run once; the count cannot precede them as in rsk_control_batch, since a message here
 * depends on a lookup).  A linear chain; no block waits on another.  n == 0 zeroes the given counts and
 * fills a given rst_first.
 * RSK_EINVAL: a NULL ctx, tab, in or out; a table a lookup cannot use (NULL state, conv or index; dst or
 * id missing with its flag; unknown flags; bad capacity); with n > 0 a NULL status, conv or conv_row, or
 * dst / id missing in `in` with the flag; an id column (the table's with BY_ID, in->id, msgs.id) that is
 * not 8-B aligned; ctl_kind and ctl_arg not both set or both NULL; a message array without n_msg;
 * n > RSK_MAX_BATCH. */
typedef struct rsk_conv_resolve_in {
    const int8_t   *status;   /* [n] dec->status */
    const uint8_t  *cmd;      /* [n] dec->cmd, or NULL = all DATA */
    const uint8_t  *hit;      /* [n] rsk_conn_resolve_batch's hit, or NULL = every packet reached its group */
    const uint8_t  *id;       /* [n*8] dec->id, 8-B aligned; required with BY_ID, else only copied to the messages */
    const uint32_t *conv;     /* [n] dec->conv */
    const uint32_t *dst;      /* [n] the parse's TcpInfo dst; required with BY_DST */
    const uint8_t  *ctl_kind; /* [n] rsk_control_batch's kind, or NULL */
    const uint64_t *ctl_arg;  /* [n] rsk_control_batch's arg, or NULL */
} rsk_conv_resolve_in;
typedef struct rsk_conv_resolve_out {
    uint32_t *conv_row;   /* [n] row, or RSK_CONN_NONE */
    int8_t   *unknown;    /* [n] optional */
    uint32_t *n_unknown;  /* [1] optional, written */
    uint32_t *rst_first;  /* [capacity] optional */
    rsk_ctl_msgs msgs;    /* m = n; optional */
} rsk_conv_resolve_out;
int rsk_conv_resolve_batch(rsk_ctx *ctx, const rsk_conv_table *tab, uint32_t n, const rsk_conv_resolve_in *in,
                           const rsk_conv_resolve_out *out, void *stream);

/* Create: the convs born in a batch, made on the device table (SubGroup::OnRecv -> newConn inside the packet
 * walk, server/SubGroup.cpp:31-68), so that a receive batch ends in conv rows with no host step:
 *   rsk_conv_resolve_batch (conv_row, unknown) -> rsk_conv_create_batch -> rsk_demux_batch / rsk_deliver_batch
 * and the host reads n_new, new_rows and n_full after the batch to open the new convs' UDP sockets.  It is
 * the documented host procedure (list the distinct unknown keys, write rows, rsk_conv_index_build, resolve
 * the unknown packets again) done in place:
 *   1. considered: the first u_max packets with unknown[i] == RSK_RECV_VALID, in packet order.  The key
 *      fields of other packets are never read.
 *   2. K_0 .. K_{k-1}: the distinct keys (id, dst, conv -- each part only with its flag) among them, in
 *      first-arrival order.
 *   3. v_0 < v_1 < ...: the vacant rows (LIVE bit clear).  K_j gets row v_j for j < n_new = min(k, number of
 *      vacant rows); n_full = k - n_new.
 *   4. a new row: state = RSK_CONN_LIVE; conv, dst, id of its first packet; where the table has the column
 *      cur_in = cur_out = prev_in = prev_out = 0 and alive = 1 (a fresh IConn::DataStat, conn/IConn.h:80-84).
 *      It is inserted into tab->index with rsk_conv_index_build's rule (compare-and-swap on a free entry,
 *      the lowest row of a key wins) and no rebuild; the insert is the launch after the one that writes the
 *      rows.  The index bytes may differ from a rebuilt index (probe positions depend on the insertion
 *      order); every lookup's result is the same.
 *   5. every packet of the batch -- considered or not -- with unknown[i] == VALID whose key now resolves gets
 *      conv_row[i] = row, unknown[i] = RSK_RECV_DROP and adds 1 to cur_in[row] when the column is given
 *      (exact under any skew, combined on chip as the resolve's).  Every other packet's conv_row / unknown
 *      and every row that was not created stay bytewise untouched.
 *   6. new_rows[j] = v_j, new_first[j] = the first packet of K_j, for j < n_new; nothing behind them is
 *      written.  *n_unknown = the packets still unknown; *n_new, *n_full: written, not accumulated.
 * With u_max below the number of unknown packets the caller calls again while n_unknown > 0 && n_full == 0:
 * the sequence gives the rows, conv_row and counters of one call with u_max >= n.
 * CONV_RST packets are not looked at: one that names a conv born in this call keeps conv_row NONE, as under
 * the snapshot rule above.  The index must be current, as for every lookup: otherwise the results for the
 * affected keys are unspecified, but no access leaves the table, work or the columns.  n == 0 writes the
 * given counts (0) and nothing else.
 * `rows` holds writable aliases of the table's key columns (the table struct's are const): each must equal
 * the table's pointer, dst / id only with their flag.
 * work: rsk_conv_create_bytes(u_max, capacity) bytes, 16-B aligned, caller-owned, contents do not matter;
 * calls that may run concurrently (two streams) need one each.  With m = min(u_max, capacity), P = the
 * smallest power of two >= max(4, 2 u_max) and M = 2 * ceil(u_max / 64) rounded up to a multiple of 4:
 * bytes = 4 * (16 + M + P + u_max + 2 m), rounded up to 16.  It depends on u_max and capacity only, never
 * on n; 0 for u_max == 0, u_max > 2^24 or a bad capacity.
 * Launches: a linear chain of kernels, the first of which zeroes *n_unknown (list the considered packets; deduplicate them in
 * work; rank first arrivals and vacant rows; write rows; insert; assign); no block waits on another, nothing
 * spins, every probe loop is bounded by its table's size.  The per-tile counts live in the control path's
 * per-stream scratch as the resolve's (rsk_reserve_stream before a capture), everything else in work.
 * RSK_EINVAL: a NULL ctx, tab, rows, in, out or work; a table a lookup cannot use; rows not aliasing the
 * table; u_max 0 or > 2^24; with n > 0 a NULL conv_row, unknown or conv, or dst / id missing with their
 * flag; an id column (in->id, the table's with BY_ID) that is not 8-B aligned or a work that is not 16-B
 * aligned; n > RSK_MAX_BATCH. */
uint64_t rsk_conv_create_bytes(uint32_t u_max, uint32_t capacity);

typedef struct rsk_conv_rows {   /* writable aliases of the table's key columns */
    uint8_t *state; uint32_t *conv; uint32_t *dst; uint8_t *id;
} rsk_conv_rows;

typedef struct rsk_conv_create_in {
    const uint8_t  *id;    /* [n*8] the resolve's key columns; each required with its flag, 8-B aligned id */
    const uint32_t *conv;  /* [n] */
    const uint32_t *dst;   /* [n] */
    uint32_t u_max;        /* unknown packets considered per call, in packet order */
    void *work;            /* rsk_conv_create_bytes(u_max, tab->capacity) bytes */
} rsk_conv_create_in;

typedef struct rsk_conv_create_out {
    uint32_t *conv_row;    /* [n] in/out: rsk_conv_resolve_batch's */
    int8_t   *unknown;     /* [n] in/out: rsk_conv_resolve_batch's */
    uint32_t *n_unknown;   /* [1] optional, written: packets still unknown afterwards */
    uint32_t *new_rows;    /* [min(u_max, capacity)] optional: row of the j-th new conv */
    uint32_t *new_first;   /* [min(u_max, capacity)] optional: packet that created it */
    uint32_t *n_new;       /* [1] optional, written */
    uint32_t *n_full;      /* [1] optional, written: distinct considered keys that got no row */
} rsk_conv_create_out;

int rsk_conv_create_batch(rsk_ctx *ctx, const rsk_conv_table *tab, const rsk_conv_rows *rows, uint32_t n,
                          const rsk_conv_create_in *in, const rsk_conv_create_out *out, void *stream);

/* Close: convs closed on the device table, where the reference calls IGroup::CloseConn (conn/IGroup.cpp:126-137):
 * from IGroup::Flush for the convs that went quiet (conn/IGroup.cpp:81-107), and from ConnReset::OnRecvConvRst
 * inside the packet walk (callbacks/ConnReset.cpp:67-77), behind which a DATA packet of the same key gets a new
 * SConn (SubGroup::OnRecv -> newConn, server/SubGroup.cpp:31-68).  A call has exactly one of two forms; in both a
 * row is closed iff it is LIVE and marked.
 * TIMER FORM (in->close_rows, n_close, m_max, work; n == 0):
 *   timer    rsk_conv_flush (dead_rows, n_dead) -> rsk_conv_close_batch(close_rows = dead_rows, n_close = n_dead)
 *   The marked rows are the first min(*n_close, m_max) entries of close_rows; *n_close is a device word that
 *   the host need not read.  Entries >= capacity, entries naming a row that is not LIVE and repeated entries
 *   close nothing extra: a row is closed once.  work: rsk_conv_close_bytes(capacity) bytes (one mark per row,
 *   rounded up to 16), 16-B aligned, caller-owned, contents do not matter; one per stream that runs the call.
 *   The packet columns of `out` are not looked at.
 * RECEIVE FORM (in->rst_first [capacity] and in->ctl_kind [n] as rsk_conv_resolve_batch read and left them;
 * out->conv_row in/out):
 *   receive  rsk_conv_resolve_batch -> rsk_conv_create_batch -> rsk_conv_close_batch (HOLD) ->
 *            rsk_conv_create_batch -> rsk_demux_batch / rsk_deliver_batch
 *   Row r is marked iff rst_first[r] != 0xFFFFFFFF.  For each packet i whose conv_row[i] is a closed row r, with
 *   a = rst_first[r]:
 *     i <= a                                   nothing changes; the reset packet itself keeps conv_row == r;
 *     i > a, ctl_kind[i] != RSK_CTL_CONV_RST   (a DATA packet that had found the conv) conv_row[i] = NONE,
 *                                              unknown[i] = RSK_RECV_VALID where the column is given; counted in
 *                                              n_reopened: the next create makes the reborn conv and routes it;
 *     i > a, ctl_kind[i] == RSK_CTL_CONV_RST   conv_row[i] = NONE (the reference's lookup finds nothing and
 *                                              returns -1); counted in n_rst_again.
 *   *n_unknown is in/out and grows by the reopened packets; n_reopened and n_rst_again are written, not
 *   accumulated.  No other packet is touched, and ctl_kind[i] of a packet whose conv_row is not a closed row is
 *   never read.  On a table without RSK_CONV_BY_DST (a client) the resolve never sets rst_first: the call closes
 *   nothing.  n == 0 closes the marked rows and looks at no packet column.
 * BOTH FORMS: closed_rows[j] = the j-th closed row in row order (as dead_rows, and as the create takes the
 * vacant rows), closed_at[j] = its reset's packet index, or 0xFFFFFFFF in the timer form; *n_closed is written,
 * not accumulated, and nothing behind entry n_closed is written.  state[r] of a closed row loses RSK_CONN_LIVE,
 * written through rows->state (`rows` aliases the table as in the create).  The key columns, alive and the four
 * counters of every row stay bytewise untouched (the create resets them when the row is reused): cur_in of a
 * closed row keeps the counts of its reopened packets.  After the call every lookup gives what
 * rsk_conv_index_build over the new state gives: the index is rebuilt over the rows that stay (open addressing
 * without tombstones has no erase in place), by launches that leave at once when nothing closed -- then no byte
 * of the index, of state or of the packet columns is written.
 * RSK_CONV_CLOSE_HOLD (receive form only): state keeps LIVE and only the index forgets the closed rows, as if
 * they were not LIVE.  A create later in the same chain then cannot hand a vacated row to another key, so within
 * a batch a row names one conv (the old conv's packets up to its reset and a new conv's from its birth on could
 * otherwise overlap under one row).  After the batch the host clears LIVE for closed_rows; no rebuild is needed,
 * the index already lacks them.  Until then a held row is LIVE to every other call: rsk_conv_send_batch gives
 * ok = 1 for it, rsk_conv_flush flushes or lists it, and a rebuild (rsk_conv_index_build, or the next close that
 * closes something) would insert it again.
 * DEVIATIONS from the reference's walk that remain: a CONV_RST naming a conv born in the same batch keeps NONE
 * (the resolve ran before the create); a row's second reset is only counted: n_rst_again > 0 is the conservative
 * sign of one, and if a DATA packet lay between the two resets the reference closed the reborn conv too -- the
 * host redoes that row's packets behind the second reset.
 * Launches: a linear chain of kernels and no memset node (timer form: clear and scatter the marks; count the
 * closing rows per tile; one block scans; one launch for the packets' pass of the receive form, closed_rows /
 * closed_at and the clear of the index; one over the rows that clears LIVE and inserts the rows that stay); the
 * last two leave at once when nothing closes.  No block waits on another, nothing spins, the probe loop is
 * bounded by the index's size.  The
 * per-tile counts live in the control path's per-stream scratch (rsk_reserve_stream before a capture).
 * RSK_EINVAL: a NULL ctx, tab, rows, in or out; a table a lookup cannot use; rows not aliasing the table; both
 * close_rows and rst_first given, or neither; unknown flags; timer form: a NULL n_close or work, n != 0, HOLD,
 * or ctl_kind given; receive form: n_close given, or with n > 0 a NULL ctl_kind or conv_row; closed_rows or
 * closed_at without n_closed; an index or a work that is not 16-B aligned, the table's id column (BY_ID) not
 * 8-B aligned; n > RSK_MAX_BATCH. */
#define RSK_CONV_CLOSE_HOLD 0x1u
uint64_t rsk_conv_close_bytes(uint32_t capacity); /* 0 for a capacity outside [1, RSK_CONN_MAX_ROWS] */

typedef struct rsk_conv_close_in {
    const uint32_t *close_rows; /* [m_max] timer form: the rows to close, e.g. rsk_conv_flush's dead_rows */
    const uint32_t *n_close;    /* [1] timer form: device word, e.g. rsk_conv_flush's n_dead */
    uint32_t m_max;             /* timer form: entries of close_rows */
    const uint32_t *rst_first;  /* [capacity] receive form: rsk_conv_resolve_batch's */
    const uint8_t  *ctl_kind;   /* [n] receive form: rsk_control_batch's kind, as the resolve read it */
    void *work;                 /* timer form: rsk_conv_close_bytes(tab->capacity) bytes */
    uint32_t flags;             /* RSK_CONV_CLOSE_HOLD */
} rsk_conv_close_in;

typedef struct rsk_conv_close_out {
    uint32_t *conv_row;    /* [n] receive form, in/out */
    int8_t   *unknown;     /* [n] receive form, in/out, optional */
    uint32_t *n_unknown;   /* [1] receive form, in/out, optional: grows by the reopened packets */
    uint32_t *closed_rows; /* [capacity] optional */
    uint32_t *closed_at;   /* [capacity] optional */
    uint32_t *n_closed;    /* [1] written; required with closed_rows or closed_at */
    uint32_t *n_reopened;  /* [1] optional, written */
    uint32_t *n_rst_again; /* [1] optional, written */
} rsk_conv_close_out;

int rsk_conv_close_batch(rsk_ctx *ctx, const rsk_conv_table *tab, const rsk_conv_rows *rows, uint32_t n,
                         const rsk_conv_close_in *in, const rsk_conv_close_out *out, void *stream);

/* Send: SubGroup::sconnSend / ClientGroup::cconSend set the head's conv, then IConn::Send -> afterSend
 * counts the packet.  ok[i] (optional) = 1 iff conv_row[i] < capacity and the row is LIVE; the given
 * columns conv[i], dst[i], id[8i..] (an rsk_encode_in's) receive the row's values, or zero; *n_bad = the
 * packets that are not ok (written).  With `sent` given (int32 [n], the encode's status) every packet
 * that is ok and has sent[i] > 0 adds 1 to cur_out[row], combined on chip as the resolve's counts; no
 * counting without it.  The caller expands before the encode (sent NULL) and counts after it (no output
 * columns).  No scratch: memset nodes and one kernel.
 * RSK_EINVAL: a NULL ctx, tab, out or tab->state; unknown flags or a bad capacity; a NULL conv_row with
 * n > 0; an output column whose table column is NULL; sent without tab->cur_out; an id column (the
 * table's or out->id) that is not 8-B aligned when out->id is given; n > RSK_MAX_BATCH. */
typedef struct rsk_conv_send_out {  /* every field optional */
    uint32_t *conv;   /* [n] */
    uint32_t *dst;    /* [n] */
    uint8_t  *id;     /* [n*8], 8-B aligned */
    uint8_t  *ok;     /* [n] */
    uint32_t *n_bad;  /* [1] */
} rsk_conv_send_out;
int rsk_conv_send_batch(rsk_ctx *ctx, const rsk_conv_table *tab, uint32_t n, const uint32_t *conv_row,
                        const int32_t *sent, const rsk_conv_send_out *out, void *stream);

/* IGroup::Flush (conn/IGroup.cpp:81-107) as one pass over the rows.  Per row r:
 *   1. not LIVE: nothing but state[r] is read or written;
 *   2. LIVE and alive[r] == 0: r is appended to dead_rows and its counters are left alone (the reference
 *      closes it before the flush loop, so it is never flushed);
 *   3. LIVE and alive: alive[r] = (prev_in[r] != cur_in[r]) && (prev_out[r] != cur_out[r]), then
 *      prev_in[r] = cur_in[r], prev_out[r] = cur_out[r] (DataStat::Flush).
 * dead_rows is in row order; *n_dead and *n_alive (the LIVE rows alive after the pass: IGroup::Alive() is
 * n_alive != 0) are written, not accumulated.  A conv that goes quiet is therefore marked at one flush
 * and listed at the next, as in the reference.  state stays read-only: rsk_conv_close_batch(close_rows =
 * dead_rows, n_close = n_dead) closes the listed rows on the device (or the host clears LIVE for them and
 * rebuilds).  No index is read.  Launches and scratch are rsk_keepalive_flush's.
 * RSK_EINVAL: a NULL ctx, tab, out, state, alive or one of the four counter columns; unknown flags or a
 * bad capacity; dead_rows without n_dead. */
typedef struct rsk_conv_flush_out {  /* every field optional */
    uint32_t *dead_rows;  /* [C] */
    uint32_t *n_dead;     /* [1] required with dead_rows */
    uint32_t *n_alive;    /* [1] */
} rsk_conv_flush_out;
int rsk_conv_flush(rsk_ctx *ctx, const rsk_conv_table *tab, const rsk_conv_flush_out *out, void *stream);

/* Host twins (host pointers, the same rules and outputs, nthreads as rsk_deliver_host; the IdBuf columns
 * are read bytewise at any alignment; the build, the flush and the counting run on the caller's thread). */
int rsk_conv_index_build_host(const rsk_conv_table *tab, uint32_t *n_dup, int nthreads);
int rsk_conv_resolve_host(const rsk_conv_table *tab, uint32_t n, const rsk_conv_resolve_in *in,
                          const rsk_conv_resolve_out *out, int nthreads);
int rsk_conv_send_host(const rsk_conv_table *tab, uint32_t n, const uint32_t *conv_row, const int32_t *sent,
                       const rsk_conv_send_out *out, int nthreads);
int rsk_conv_flush_host(const rsk_conv_table *tab, const rsk_conv_flush_out *out, int nthreads);
/* rsk_conv_create_batch's twin: sequential on the caller's thread, the same work buffer (16-B aligned). */
int rsk_conv_create_host(const rsk_conv_table *tab, const rsk_conv_rows *rows, uint32_t n,
                         const rsk_conv_create_in *in, const rsk_conv_create_out *out, int nthreads);
/* rsk_conv_close_batch's twin: sequential on the caller's thread, the same work buffer in the timer form. */
int rsk_conv_close_host(const rsk_conv_table *tab, const rsk_conv_rows *rows, uint32_t n,
                        const rsk_conv_close_in *in, const rsk_conv_close_out *out, int nthreads);

/* ---- capture filter ------------------------------------------------------- */
/* RCap::doInit (cap/RCap.cpp:64-88) compiles BuildFilterStr("tcp", srcIp, dstIp, srcPorts, dstPorts,
 * isServer) (cap/cap_util.cpp:67-144) into the kernel's BPF filter.  For a client that string is
 *   F  = tcp [and (ip src S)] [and (ip dst D)] [and ( src port p or ... src portrange a-b ... )]
 *        [and ( dst port p or ... dst portrange a-b ... )]
 * and for a server  ((tcp[tcpflags] & tcp-syn != 0) and F') or (F and (tcp[tcpflags] & (tcp-syn) == 0))
 * where F' is F with every "dst" replaced by "src".  rsk_capture_filter_batch evaluates that
 * predicate with libpcap's meaning of each primitive:
 *   tcp          IPv4 with protocol 6, or IPv6 with next header 6 (directly, or after a fragment
 *                header, 44);
 *   ip src/dst   IPv4 only, the address field equals S / D;
 *   [src|dst] port / portrange   IPv4 with protocol 6, 17 or 132 and fragment offset 0, or IPv6
 *                with next header 6, 17 or 132; the port field (at 4 * IHL on IPv4, 40 on IPv6)
 *                equals p / lies in [a, b];
 *   tcp[tcpflags]  IPv4 with protocol 6 and fragment offset 0: TCP header byte 13.
 * Link layer: DLT_EN10MB ethertype 0x0800 / 0x86dd at bytes 12-13; DLT_NULL a 4-byte family in
 * host order, 2 = IPv4, 24 / 28 / 30 = IPv6 (BSD values).  Evaluation is left to right with
 * short-circuit; a field read past cap_len rejects the packet (as a BPF load out of bounds does).
 * match[i] = 1 / 0; match_idx / n_match (optional, may be NULL) list the matches in order. */
#define RSK_FILTER_MAX_PORTS 64
typedef struct rsk_port_list {
    uint16_t n_single, n_range;            /* RPortList::GetSinglePortList / GetPortRangeList sizes */
    uint16_t single[RSK_FILTER_MAX_PORTS]; /* in list order                                        */
    uint16_t range[RSK_FILTER_MAX_PORTS][2]; /* [source, dest], source < dest (RPortList.cpp:21-27) */
} rsk_port_list;
typedef struct rsk_capture_filter {
    uint32_t src_ip, dst_ip;  /* IPv4 as stored in the header (network-order bytes read LE)        */
    uint8_t has_src_ip;       /* srcIp non-empty                                                  */
    uint8_t has_dst_ip;       /* dstIp non-empty                                                  */
    uint8_t is_server;
    uint8_t reserved;         /* 0                                                                */
    rsk_port_list src_ports, dst_ports;
} rsk_capture_filter;
int rsk_capture_filter_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *cap_arena, const uint64_t *cap_off,
                             const uint32_t *cap_len, int datalink, const rsk_capture_filter *filter,
                             uint8_t *match, uint32_t *match_idx, uint32_t *n_match, void *stream);
/* The filter and rsk_parse_decode_batch in one pass over a capture batch (the parse reuses the
 * filter's header window): match[i] as above; a packet the filter passes gets exactly
 * rsk_parse_decode_batch's outputs, one it rejects (pcap never hands it to RawTcp::RawInput) gets
 * parse_status RSK_PARSE_DROP, zero TcpInfo and dec->status RSK_RECV_DROP; dec->valid_idx lists the
 * VALID packets in order. */
int rsk_filter_parse_decode_batch(rsk_ctx *ctx, uint32_t n, const uint8_t *cap_arena, const uint64_t *cap_off,
                                  const uint32_t *wire_len, const uint32_t *cap_len, int datalink, int flags,
                                  const rsk_capture_filter *filter, uint8_t *match, const rsk_tcpinfo_out *tcp,
                                  const rsk_decode_out *dec, void *stream);
/* Host: the exact string BuildFilterStr returns for this filter (proto "tcp", addresses dotted),
 * NUL-terminated into buf.  Returns its length, or -1 if buf_len is too small. */
int rsk_filter_str(const rsk_capture_filter *filter, char *buf, size_t buf_len);

/* ---- single-packet shims with the reference signatures (host pointers) ----------------------- */
/* These run the same HIP kernels on a batch of one (device round trip, synchronous), so a caller
 * can swap them in per call.  They are a compatibility surface, not a fast path. */
/* Writes the 8-byte tag for data[0] to tag_out; returns tag_out + 8 (NULL if data_len <= 0). */
uint8_t *rsk_compute_hash(rsk_ctx *ctx, uint8_t *tag_out, const uint8_t *data, int data_len);
/* 1 if tag == MD5(key || data[0])[8..15], 0 otherwise (0 when data == NULL or data_len <= 0). */
int rsk_hash_equal(rsk_ctx *ctx, const uint8_t *tag, const uint8_t *data, int data_len);
/* Writes the 23-byte EncHead; returns p + 23, or NULL when p == NULL or buf_len < 23. */
uint8_t *rsk_enchead_enc2buf(rsk_ctx *ctx, uint8_t *p, int buf_len, uint8_t cmd, const uint8_t id[8],
                             uint32_t conv, uint64_t conn_key);
/* Decodes fields; returns p + len (len = p[0]), or NULL when p == NULL, buf_len < 23 or len > buf_len.
 * Any output pointer may be NULL. */
const uint8_t *rsk_enchead_decodebuf(rsk_ctx *ctx, const uint8_t *p, int buf_len, uint8_t *len,
                                     uint8_t *cmd, uint8_t id[8], uint32_t *conv, uint64_t *conn_key);

/* ---- connKey helpers (host, pure integer arithmetic) ---------------------------------------- */
/* KeyForTcp: 0x10000000 | (dp << 16) | sp — the type bit overlaps dp bit 12, reproduced as-is. */
uint64_t rsk_key_for_tcp(uint16_t sp, uint16_t dp);
uint64_t rsk_key_for_udp(uint16_t sp, uint16_t dp);

/* ---- synthetic workload generator (device; used by bench/tests, not by the codec) ------------ */
/* Fills n bytes at dst with the splitmix64 stream: 8-byte word w = splitmix64(seed + w) (LE). */
int rsk_fill_splitmix(void *dst, uint64_t nbytes, uint64_t seed, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RSK_CODEC_H */
