/*
 * ref_tcpstate_harness.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Runs the REFERENCE's own fake-TCP connection state and raw-TCP send, compiled from /root/reference by
 * oracle/Makefile (`make -C oracle ref` -> oracle/_ref/librsk_ref_tcpstate.so; nothing from the reference
 * is copied here):
 *   send     FakeTcp::Output (conn/FakeTcp.cpp:43-50) -> INetConn::Output (conn/INetConn.cpp:32-40, stamps
 *            the connKey into the head) -> IConn::Output -> the output callback -> RConn::Send ->
 *            RConn::Output (conn/RConn.cpp:87-131, the REAL class: oversize check, compute_hash, Enc2Buf)
 *            -> RawTcp::Send -> RawTcp::Output (conn/RawTcp.cpp:111-130, mIpId++) -> RawTcp::SendRawTcp
 *            (:280-341) -> libnet_build_tcp / libnet_build_ipv4 / libnet_write
 *   receive  IConn::Input -> FakeTcp::OnRecv (conn/FakeTcp.cpp:52-67) -> INetConn::OnRecv -> IConn::OnRecv
 *            -> the recv callback, which returns the scripted value; the `n >= 0` gate and the plain
 *            unsigned compare are the reference's
 *   init     FakeTcp::Init -> TcpUtil::SetISN / SetAckISN (src/util/TcpUtil.cpp)
 * K real FakeTcp objects over one real RConn, which owns one real RawTcp.
 *
 * THE ONE STAND-IN of this pin: libnet exists only as a prebuilt archive, which is never linked or run.
 * libnet_build_tcp, libnet_build_ipv4, libnet_write and libnet_geterror are defined HERE with the
 * prototypes of the vendored libnet.h, as recorders: they store every argument (the payload pointer's
 * bytes, payload_s and the ptag included), build no packet, and return a positive ptag / the payload
 * length.  So the VALUES SendRawTcp hands to libnet are the reference's own code; the byte layout libnet
 * would give them is not pinned here (it stays pinned to RFC 791 / 793 / 1071).
 *
 * What is not run: RConn::Init / RawTcp::Init (libnet_init, pcap, the services); the two objects are
 * marked initialised through the public base IConn::Init(), RawTcp::mTcpNet points at a dummy that only
 * the recorders receive, and RawTcp::mIpId is set from the script.  FakeTcp's constructor asserts its
 * socket's 4-tuple against GetTcpInfo; that one object (FakeTcp.cpp) is compiled with -DNDEBUG and gets an
 * unconnected uv_tcp_t from uv_tcp_init on a private loop that never runs until teardown.  The class is
 * neither edited nor copied.  Private members (FakeTcp::mInfo, RConn::mRawTcp, RawTcp::mIpId / mTcpNet)
 * are reached by compiling the class headers with `private` spelled `public` in THIS translation unit only
 * (layout unchanged), as ref_parse_harness.cpp does.  Functions none of this calls stay unresolved;
 * RTLD_LAZY.
 */
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#include <libnet.h>
#include <pcap.h>
#include <uv.h>
#include <plog/Log.h>
#include <plog/Appenders/IAppender.h>

#include "rscomm.h"
#include "rcommon.h"
#include "bean/EncHead.h"
#include "bean/TcpInfo.h"
#include "src/service/IRouteObserver.h"
#include "src/service/ITimerObserver.h"

#define private public
#include "conn/IConn.h"
#include "conn/INetConn.h"
#include "conn/FakeTcp.h"
#include "conn/RawTcp.h"
#include "conn/RConn.h"
#undef private

namespace {

const int REC_W = 32;
/* One record per event (int64):
 *  0 kind (0 send, 1 receive)   1 return of FakeTcp::Output / IConn::Input
 *  2 libnet_build_tcp calls  3 libnet_build_ipv4 calls  4 libnet_write calls   (during this event)
 *  5 mInfo.seq after   6 mInfo.ack after   7 RawTcp::mIpId after
 *  libnet_build_tcp:  8 sp  9 dp  10 seq  11 ack  12 control  13 win  14 sum  15 urg  16 len
 *                    17 payload_s  18 ptag  19 payload != NULL
 *  libnet_build_ipv4: 20 ip_len  21 tos  22 id  23 frag  24 ttl  25 prot  26 sum  27 src  28 dst
 *                    29 payload != NULL  30 payload_s  31 ptag */
struct Rec {
    int64_t *row = nullptr;
    uint8_t *frame = nullptr;
    uint32_t frame_cap = 0;
};
Rec g_rec;
libnet_t *g_ctx = nullptr;  /* the dummy context: the recorders check they are handed this one */
char g_ctx_store[64];
bool g_plog = false;

struct State {
    uv_loop_t loop;
    RConn *rconn = nullptr;
    std::vector<FakeTcp *> conns;
    int recv_ret = 0;
};

}  // namespace

/* ---- the recorders (prototypes of the vendored libnet-functions.h) --------------------------------- */
extern "C" {

libnet_ptag_t libnet_build_tcp(uint16_t sp, uint16_t dp, uint32_t seq, uint32_t ack, uint8_t control, uint16_t win,
                               uint16_t sum, uint16_t urg, uint16_t len, const uint8_t *payload, uint32_t payload_s,
                               libnet_t *l, libnet_ptag_t ptag) {
    int64_t *r = g_rec.row;
    if (!r || l != g_ctx) return -1;
    r[2]++;
    r[8] = sp; r[9] = dp; r[10] = seq; r[11] = ack; r[12] = control; r[13] = win; r[14] = sum; r[15] = urg;
    r[16] = len; r[17] = payload_s; r[18] = ptag; r[19] = payload != nullptr;
    if (g_rec.frame && payload) {
        std::memcpy(g_rec.frame, payload, payload_s < g_rec.frame_cap ? payload_s : g_rec.frame_cap);
    }
    return 1;
}

libnet_ptag_t libnet_build_ipv4(uint16_t ip_len, uint8_t tos, uint16_t id, uint16_t frag, uint8_t ttl, uint8_t prot,
                                uint16_t sum, uint32_t src, uint32_t dst, const uint8_t *payload, uint32_t payload_s,
                                libnet_t *l, libnet_ptag_t ptag) {
    int64_t *r = g_rec.row;
    if (!r || l != g_ctx) return -1;
    r[3]++;
    r[20] = ip_len; r[21] = tos; r[22] = id; r[23] = frag; r[24] = ttl; r[25] = prot; r[26] = sum; r[27] = src;
    r[28] = dst; r[29] = payload != nullptr; r[30] = payload_s; r[31] = ptag;
    return 2;
}

int libnet_write(libnet_t *l) {
    int64_t *r = g_rec.row;
    if (!r || l != g_ctx) return -1;
    r[4]++;
    return (int)r[20];  /* libnet_write returns the bytes written: the IP total length */
}

char *libnet_geterror(libnet_t *l) {
    static char none[] = "recorder";
    return none;
}

/* ---- the C ABI ------------------------------------------------------------------------------------ */

int ref_ts_head_size(void) { return RConn::HEAD_SIZE; }  /* the reference's object, not a constant here */

/* K conns from K rows: info [k][7] = src, dst, sp, dp, seq, ack, flag (the TcpInfo FakeTcp is constructed
 * with, as from TcpAckPool) and key [k].  state0 [k][2] gets mInfo.seq / mInfo.ack after FakeTcp::Init. */
void *ref_ts_open(const char *hash_key, int key_len, uint32_t k, const uint32_t *info, const uint64_t *key,
                  uint32_t ip_id0, uint32_t *state0) {
    if (!g_plog) {  /* TcpUtil and RConn::Output log; severity none logs nothing */
        plog::init(plog::none);
        g_plog = true;
    }
    g_ctx = reinterpret_cast<libnet_t *>(g_ctx_store);
    State *s = new State;
    uv_loop_init(&s->loop);
    s->rconn = new RConn(std::string(hash_key, (size_t)key_len), "lo", &s->loop, nullptr, false);
    s->rconn->IConn::Init();           /* mInited only: RConn::Init would open libnet and pcap */
    s->rconn->mRawTcp->IConn::Init();
    s->rconn->mRawTcp->mTcpNet = g_ctx;
    s->rconn->mRawTcp->mIpId = (uint16_t)ip_id0;
    RConn *rc = s->rconn;
    for (uint32_t i = 0; i < k; i++) {
        TcpInfo t;
        t.src = info[7 * i]; t.dst = info[7 * i + 1]; t.sp = (uint16_t)info[7 * i + 2];
        t.dp = (uint16_t)info[7 * i + 3]; t.seq = info[7 * i + 4]; t.ack = info[7 * i + 5];
        t.flag = (uint8_t)info[7 * i + 6];
        uv_tcp_t *tcp = (uv_tcp_t *)std::malloc(sizeof(uv_tcp_t));  /* freed by the reference's close_cb */
        uv_tcp_init(&s->loop, tcp);
        FakeTcp *c = new FakeTcp(tcp, key[i], t);
        c->Init();  /* SetISN / SetAckISN; uv_read_start fails on the unconnected handle and is ignored there */
        c->SetOutputCb([rc](ssize_t nread, const rbuf_t &rbuf) { return rc->Send(nread, rbuf); });
        c->SetOnRecvCb([s](ssize_t nread, const rbuf_t &rbuf) { return s->recv_ret; });
        state0[2 * i] = c->mInfo.seq;
        state0[2 * i + 1] = c->mInfo.ack;
        s->conns.push_back(c);
    }
    return s;
}

/* A script of events.  kind 0: send (conn, a = nread, payload at pay_arena + pay_off, conv in the head);
 * kind 1: receive (conn, a = TcpInfo.seq of the packet, b = what the upstream callback returns).
 * rec [n][REC_W]; frames (optional) [n][frame_cap] gets the bytes behind libnet_build_tcp's payload. */
int ref_ts_run(void *h, uint32_t n, const uint8_t *kind, const uint32_t *conn, const uint32_t *a, const int32_t *b,
               const uint8_t *pay_arena, const uint64_t *pay_off, const uint32_t *conv, const uint8_t *id8,
               int64_t *rec, uint8_t *frames, uint32_t frame_cap) {
    State *s = static_cast<State *>(h);
    IdBufType ib;
    std::memcpy(ib.data(), id8, ID_BUF_SIZE);
    for (uint32_t i = 0; i < n; i++) {
        if (conn[i] >= s->conns.size()) return -2;
        FakeTcp *c = s->conns[conn[i]];
        int64_t *r = rec + (size_t)REC_W * i;
        std::memset(r, 0, REC_W * sizeof(int64_t));
        g_rec.row = r;
        g_rec.frame = frames ? frames + (size_t)frame_cap * i : nullptr;
        g_rec.frame_cap = frame_cap;
        r[0] = kind[i];
        if (kind[i] == 0) {
            EncHead head;  /* as the app groups hand it down: cmd DATA, the group's IdBuf, the conv */
            head.SetIdBuf(ib);
            head.SetConv(conv[i]);
            const rbuf_t buf = {const_cast<char *>(reinterpret_cast<const char *>(pay_arena + pay_off[i])),
                                (int)a[i], &head};
            r[1] = c->Output((ssize_t)a[i], buf);
        } else {
            EncHead head;
            TcpInfo pkt = c->mInfo;  /* the packet's TcpInfo as RawInput fills it: only seq matters here */
            pkt.seq = a[i];
            pkt.head = &head;
            char dummy[4] = {0};
            const rbuf_t buf = {dummy, 1, &pkt};
            s->recv_ret = b[i];
            r[1] = c->Input(1, buf);
        }
        r[5] = c->mInfo.seq;
        r[6] = c->mInfo.ack;
        r[7] = s->rconn->mRawTcp->mIpId;
    }
    g_rec.row = nullptr;
    g_rec.frame = nullptr;
    return 0;
}

/* Each conn's mInfo.seq / mInfo.ack as they stand (state [k][2]) and RawTcp::mIpId. */
void ref_ts_state(void *h, uint32_t *state, uint32_t *ip_id) {
    State *s = static_cast<State *>(h);
    for (size_t i = 0; i < s->conns.size(); i++) {
        state[2 * i] = s->conns[i]->mInfo.seq;
        state[2 * i + 1] = s->conns[i]->mInfo.ack;
    }
    *ip_id = s->rconn->mRawTcp->mIpId;
}

void ref_ts_close(void *h) {
    State *s = static_cast<State *>(h);
    for (FakeTcp *c : s->conns) {
        c->Close();  /* uv_close on the handle; the reference's close_cb frees it when the loop runs */
        delete c;
    }
    RawTcp *raw = s->rconn->mRawTcp;
    s->rconn->mRawTcp = nullptr;  /* RawTcp::Close would unregister from services that were never started */
    raw->mTcpNet = nullptr;
    raw->IConn::Close();
    delete raw;
    s->rconn->Close();
    delete s->rconn;
    uv_run(&s->loop, UV_RUN_DEFAULT);
    uv_loop_close(&s->loop);
    delete s;
}

}  // extern "C"
