/*
 * ref_conncreate_harness.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Runs the REFERENCE's own way from a handshake to a fake-TCP conn, compiled from /root/reference by
 * oracle/Makefile (`make -C oracle ref` -> oracle/_ref/librsk_ref_conncreate.so; nothing from the reference is
 * copied here):
 *   SYN      RawTcp::RawInput (conn/RawTcp.cpp:138-237; server: TcpInfo::Reverse, bean/TcpInfo.cpp:60-63) ->
 *            TcpAckPool::AddInfoFromPeer (net/TcpAckPool.cpp:17-33)
 *   DATA     RawTcp::RawInput -> cap2uv (captured) -> INetGroup::Input (conn/INetGroup.cpp:57-83) ->
 *            SNetGroup::CreateNetConn (server/SNetGroup.cpp:20-46) -> ServerNetManager::GetTcp
 *            (server/ServerNetManager.cpp:52-75) -> TcpAckPool::Wait2TransferInfo (net/TcpAckPool.cpp:45-70) ->
 *            new FakeTcp, FakeTcp::Init (TcpUtil::SetISN / SetAckISN) -> INetGroup::AddNetConn -> the conn's Input
 *            (FakeTcp::OnRecv); without a conn the group's default conn and ERR_NO_CONN
 *   expiry   TcpAckPool::OnFlush (:85-95), ServerNetManager::OnFlush (:82-103)
 *   send     INetGroup::Send -> doSend (:111-135) over rand() -> FakeTcp::Output
 *   client   the statement sequence of ClientNetManager::createINetConn (client/ClientNetManager.cpp:65-78) around
 *            the reference's objects: Wait2TransferInfo on the real pool (filled by RawInput without the server flag),
 *            KeyGenerator::KeyForConnInfo, new FakeTcp, Init, and a real INetGroup::AddNetConn.  The class itself
 *            needs a connected socket (GetTcpInfo) and is not run.
 * One real TcpAckPool, one real ServerNetManager over it (constructed, never Init()ed: the constructor only stores
 * its arguments), G real SNetGroups sharing that manager, real FakeTcps (the -DNDEBUG object of the tcpstate pin).
 *
 * Stand-ins:
 *   - accepted sockets: ServerNetManager::mPool is filled HERE with the reference's ConnHelper around uv_tcp_t
 *     handles on a private loop that never runs until teardown (add2Pool needs GetTcpInfo of a connected socket).
 *     Each handle is opened (uv_tcp_open) over an unconnected socket() descriptor of its own, not left bare as in
 *     ref_tcpstate_harness.cpp: SNetGroup::CreateNetConn gives the conn up when FakeTcp::Init fails, and Init returns
 *     uv_read_start, which refuses a handle without a descriptor.  One descriptor per pooled or taken socket: the
 *     process's soft limit is raised to its hard limit, and a script that needs more fails (-4).  GetTcp, OnFlush
 *     and closeTcp are the reference's.  A closed socket is one uv_is_closing();
 *   - the clock: both pools stamp entries with rsk_now_ms() + PersistMs().  So that expiry can be scripted, the
 *     expiry AddInfoFromPeer has just stored is rewritten to (the event's ts + PersistMs()) and an accepted socket's
 *     ConnHelper is built with the same sum; OnFlush(ts) then is the reference's compare on scripted numbers;
 *   - each SNetGroup gets its default conn and a Handler that queues nothing without INetGroup::Init (which needs
 *     the service graph), as ref_control_harness.cpp does; the subclass overrides CreateNetConn only to call the
 *     base and note what it returned;
 *   - the groups' output / recv callbacks return nread; the output one notes the sending conn's key;
 *   - rand() is defined HERE (-Wl,-Bsymbolic-functions), so doSend's draws are inputs.
 * Private and protected members are reached by compiling the reference's class headers with both words spelled
 * `public` in THIS translation unit only (layout unchanged).  Functions none of this calls stay unresolved;
 * RTLD_LAZY.
 */
#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/resource.h>
#include <sys/socket.h>
#include <unistd.h>

#include <algorithm>
#include <array>
#include <cassert>
#include <chrono>
#include <condition_variable>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <libnet.h>
#include <pcap.h>
#include <uv.h>
#include <plog/Log.h>

#define private public
#define protected public
#include "rscomm.h"
#include "rcommon.h"
#include "bean/EncHead.h"
#include "bean/ConnInfo.h"
#include "bean/TcpInfo.h"
#include "src/service/IRouteObserver.h"
#include "src/service/ITimerObserver.h"
#include "src/util/TcpCmpFn.h"
#include "src/util/KeyGenerator.h"
#include "conn/IConn.h"
#include "conn/INetConn.h"
#include "conn/IGroup.h"
#include "conn/INetGroup.h"
#include "conn/FakeTcp.h"
#include "conn/RawTcp.h"
#include "net/TcpAckPool.h"
#include "net/INetManager.h"
#include "server/ServerNetManager.h"
#include "server/SNetGroup.h"
#include "util/Handler.h"
#include "util/RPortList.h"
#include "util/rsutil.h"
#undef protected
#undef private

namespace {

struct Created {  /* one conn, in creation order */
    INetConn *conn;
    int group;
    uint32_t packet;  /* the index, within its batch, of the packet that made it */
    uint32_t info[7]; /* mInfo after Init: src, dst, sp, dp, seq, ack, flag */
};

struct State;
State *g_st = nullptr;
const uint64_t SCRIPT_TS_END = 1ull << 40;  /* scripted times and expiries lie below, the wall clock above */
bool g_plog = false;

class ProbeTcp : public RawTcp {  /* as ref_parse_harness.cpp: cap2uv captures what RawInput hands over */
public:
    ProbeTcp(TcpAckPool *pool, bool server) : RawTcp("lo", nullptr, pool, server) {}
    int called = 0;
    TcpInfo info;
    const char *payload = nullptr;
    int payload_len = 0;

protected:
    int cap2uv(const TcpInfo *i, const char *p, int n) override {
        called = 1;
        info = *i;
        payload = p;
        payload_len = n;
        return 0;
    }
};

class DefaultConn : public IConn {  /* INetGroup::mDefaultFakeConn */
public:
    DefaultConn() : IConn("default") {}
    int OnRecv(ssize_t nread, const rbuf_t &rbuf) override { return 0; }
};

class NullHandler : public Handler {  /* never run: a message sent to it is dropped */
public:
    explicit NullHandler(uv_loop_t *loop) : Handler(loop) {}
    bool SendMessage(const Message &message) override { return true; }
    bool SendMessageAtTime(const Message &msg, uint64_t ts) override { return true; }
};

struct State {
    uv_loop_t loop;
    TcpAckPool *pool = nullptr;
    ServerNetManager *mgr = nullptr;
    ProbeTcp *raw_server = nullptr, *raw_client = nullptr;
    std::vector<INetGroup *> groups;
    INetGroup *client = nullptr;
    std::vector<Created> conns;
    std::map<INetConn *, int> ordinal;
    std::vector<uv_tcp_t *> sockets;  /* every accepted socket, pooled or taken or closed */
    /* the packet in flight */
    int cur_group = 0;
    uint32_t cur_packet = 0;
    int create_ran = 0, create_ret = 0;
    /* the send in flight */
    const uint32_t *draws = nullptr;
    uint32_t n_draws = 0, used = 0;
    bool exhausted = false;
    uint64_t sender_key = 0;
};

class RecGroup : public SNetGroup {
public:
    RecGroup(const std::string &id, uv_loop_t *loop, ServerNetManager *mgr, int g) : SNetGroup(id, loop, mgr), mG(g) {}
    INetConn *CreateNetConn(IntKeyType key, const ConnInfo *info) override {
        INetConn *c = SNetGroup::CreateNetConn(key, info);
        State *s = g_st;
        s->create_ran = 1;
        s->create_ret = c != nullptr;
        if (c) {
            Created r;
            r.conn = c;
            r.group = mG;
            r.packet = s->cur_packet;
            const TcpInfo &m = static_cast<FakeTcp *>(c)->mInfo;
            const uint32_t f[7] = {m.src, m.dst, m.sp, m.dp, m.seq, m.ack, m.flag};
            std::memcpy(r.info, f, sizeof f);
            s->ordinal[c] = (int)s->conns.size();
            s->conns.push_back(r);
        }
        return c;
    }
    int mG;
};

class ClientGroupStandIn : public INetGroup {  /* client/CNetGroup.cpp:11-13 */
public:
    explicit ClientGroupStandIn(uv_loop_t *loop) : INetGroup("client", loop) {}
    INetConn *CreateNetConn(IntKeyType key, const ConnInfo *info) override { return nullptr; }
};

void wire_group(State *s, INetGroup *g) {
    g->IGroup::Init();
    g->mDefaultFakeConn = new DefaultConn();
    g->mDefaultFakeConn->Init();
    g->mHandler = std::make_shared<NullHandler>(&s->loop);
    g->SetOnRecvCb([](ssize_t nread, const rbuf_t &) { return (int)nread; });
    g->SetOutputCb([](ssize_t nread, const rbuf_t &rbuf) {
        ConnInfo *info = static_cast<ConnInfo *>(rbuf.data);
        g_st->sender_key = info && info->head ? info->head->ConnKey() : 0;
        return (int)nread;
    });
}

void unwire_group(INetGroup *g, State *s) {
    for (auto &r : s->conns) {
        if (r.conn && g->ConnOfIntKey(r.conn->IntKey()) == r.conn) {
            g->INetGroup::RemoveConn(r.conn);
            r.conn->Close();  /* uv_close on the socket; the reference's close_cb frees it when the loop runs */
            delete r.conn;
            r.conn = nullptr;
        }
    }
    g->mDefaultFakeConn->Close();
    delete g->mDefaultFakeConn;
    g->mDefaultFakeConn = nullptr;
    g->mHandler = nullptr;
    g->IConn::Close();
    delete g;
}

uv_tcp_t *new_socket(State *s) {  /* nullptr: no file descriptor left */
    const int fd = socket(AF_INET, SOCK_STREAM, 0);
    if (fd < 0) return nullptr;
    uv_tcp_t *tcp = (uv_tcp_t *)std::malloc(sizeof(uv_tcp_t));  /* freed by the reference's close_cb */
    uv_tcp_init(&s->loop, tcp);
    if (uv_tcp_open(tcp, fd)) {
        close(fd);
        std::free(tcp);
        return nullptr;
    }
    s->sockets.push_back(tcp);
    return tcp;
}

void raw_input(ProbeTcp *t, const uint8_t *pkt, uint32_t len) {
    pcap_pkthdr hdr;
    std::memset(&hdr, 0, sizeof hdr);
    hdr.len = len;
    hdr.caplen = len;
    t->called = 0;
    t->RawInput(nullptr, &hdr, pkt);
}

}  // namespace

/* doSend's rand(): the next input draw.  Bound to the reference's objects by -Bsymbolic-functions. */
extern "C" int rand(void) {
    State *s = g_st;
    if (!s || !s->draws) return 0;
    if (s->used >= s->n_draws) {
        s->exhausted = true;
        return (int)(s->used++ & 0x7fffffffu);
    }
    return (int)(s->draws[s->used++] & 0x7fffffffu);
}

extern "C" {

/* Every packet is an Ethernet capture (DLT_EN10MB) with cap_len = wire length.  Every entry returns 0 or a
 * negative number: -1 a capacity is too small, -2 a bad index, -3 the draws ran out, -4 no file descriptor left,
 * -5 FakeTcp::Init failed. */

void *ref_cc_open(uint32_t n_groups, uint64_t persist_ms) {
    if (!g_plog) {
        plog::init(plog::none);
        g_plog = true;
    }
    struct rlimit rl;
    if (getrlimit(RLIMIT_NOFILE, &rl) == 0 && rl.rlim_cur < rl.rlim_max) {
        rl.rlim_cur = rl.rlim_max;
        setrlimit(RLIMIT_NOFILE, &rl);
    }
    State *s = new State;
    uv_loop_init(&s->loop);
    s->pool = new TcpAckPool(persist_ms);
    RPortList ports;
    s->mgr = new ServerNetManager(&s->loop, ports, "127.0.0.1", s->pool);
    s->raw_server = new ProbeTcp(s->pool, true);
    s->raw_client = new ProbeTcp(s->pool, false);
    s->raw_server->mDatalink = DLT_EN10MB;
    s->raw_client->mDatalink = DLT_EN10MB;
    g_st = s;
    for (uint32_t g = 0; g < n_groups; g++) {
        INetGroup *grp = new RecGroup("g" + std::to_string(g), &s->loop, s->mgr, (int)g);
        wire_group(s, grp);
        s->groups.push_back(grp);
    }
    s->client = new ClientGroupStandIn(&s->loop);
    wire_group(s, s->client);
    return s;
}

/* k SYN captures through RawInput (server != 0: the server flag set); each entry the pool took gets the expiry
 * ts + PersistMs().  took[i] = AddInfoFromPeer stamped an entry (a new one or the tuple's old one). */
int ref_cc_syn(void *h, uint32_t k, const uint8_t *arena, const uint64_t *off, const uint32_t *len, int server, uint64_t ts,
               uint8_t *took) {
    State *s = static_cast<State *>(h);
    g_st = s;
    ProbeTcp *t = server ? s->raw_server : s->raw_client;
    for (uint32_t i = 0; i < k; i++) {
        /* the entry AddInfoFromPeer has just stamped is the one that carries the wall clock (rsk_now_ms is
         * gettimeofday, above 2^40 ms; every scripted ts is below 2^39) */
        raw_input(t, arena + off[i], len[i]);
        took[i] = 0;
        for (auto &e : s->pool->mInfoPool) {
            if (e.second >= SCRIPT_TS_END) {
                e.second = ts + s->pool->PersistMs();
                took[i] = 1;
            }
        }
    }
    return 0;
}

/* k accepted sockets: (src, dst, sp, dp) in the orientation GetTcpInfo gives on the server (src = the local end)
 * into ServerNetManager::mPool with the expiry ts + POOL_PERSIST_MS. */
int ref_cc_accept(void *h, uint32_t k, const uint32_t *tuple, uint64_t ts) {
    State *s = static_cast<State *>(h);
    g_st = s;
    for (uint32_t i = 0; i < k; i++) {
        TcpInfo info;
        info.src = tuple[4 * i];
        info.dst = tuple[4 * i + 1];
        info.sp = (uint16_t)tuple[4 * i + 2];
        info.dp = (uint16_t)tuple[4 * i + 3];
        uv_tcp_t *tcp = new_socket(s);
        if (!tcp) return -4;
        s->mgr->mPool.emplace(info, ServerNetManager::ConnHelper(tcp, ts + s->mgr->POOL_PERSIST_MS));
    }
    return 0;
}

/* n DATA captures: RawInput -> the captured TcpInfo -> groups[group[i]]->Input with a head carrying key[i].
 * ret[i] = Input's return (INT32_MIN: RawInput did not hand the packet over); created[i] = 0 CreateNetConn did not
 * run, 1 it returned nullptr, 2 it returned a conn; conn[i] = the creation ordinal of the conn the key names after
 * the packet (-1 none); ack[i] = that conn's mInfo.ack then; info[7 i ..] = the TcpInfo RawInput handed over. */
int ref_cc_data(void *h, uint32_t n, const uint8_t *arena, const uint64_t *off, const uint32_t *len, const uint32_t *group,
                const uint64_t *key, int32_t *ret, uint8_t *created, int32_t *conn, uint32_t *ack, uint32_t *info) {
    State *s = static_cast<State *>(h);
    g_st = s;
    s->draws = nullptr;
    for (uint32_t i = 0; i < n; i++) {
        if (group[i] >= s->groups.size()) return -2;
        INetGroup *g = s->groups[group[i]];
        ProbeTcp *t = s->raw_server;
        raw_input(t, arena + off[i], len[i]);
        created[i] = 0;
        conn[i] = -1;
        ack[i] = 0;
        std::memset(info + 7 * (size_t)i, 0, 7 * sizeof(uint32_t));
        if (!t->called) {
            ret[i] = INT32_MIN;
            continue;
        }
        const uint32_t f[7] = {t->info.src, t->info.dst, t->info.sp, t->info.dp, t->info.seq, t->info.ack, t->info.flag};
        std::memcpy(info + 7 * (size_t)i, f, sizeof f);
        EncHead head;
        head.SetConnKey(key[i]);
        TcpInfo pi = t->info;
        pi.head = &head;
        const rbuf_t rb = new_buf(t->payload_len, const_cast<char *>(t->payload), &pi);
        s->cur_group = (int)group[i];
        s->cur_packet = i;
        s->create_ran = s->create_ret = 0;
        ret[i] = g->Input(t->payload_len, rb);
        created[i] = (uint8_t)(s->create_ran ? 1 + s->create_ret : 0);
        INetConn *c = g->ConnOfIntKey(key[i]);
        if (c) {
            conn[i] = s->ordinal[c];
            ack[i] = static_cast<FakeTcp *>(c)->mInfo.ack;
        }
    }
    return 0;
}

int ref_cc_flush(void *h, int which, uint64_t ts) {  /* 0 TcpAckPool::OnFlush, 1 ServerNetManager::OnFlush */
    State *s = static_cast<State *>(h);
    g_st = s;
    if (which == 0) s->pool->OnFlush(ts);
    else s->mgr->OnFlush(ts);
    return 0;
}

/* n sends of 8 bytes through groups[group]->Send: sender[i] = the conn's IntKey (0: ERR_NO_CONN), consumed[i] = the
 * draws that send took. */
int ref_cc_send(void *h, uint32_t group, uint32_t n, const uint32_t *draws, uint32_t n_draws, uint64_t *sender,
                uint32_t *consumed) {
    State *s = static_cast<State *>(h);
    g_st = s;
    if (group >= s->groups.size()) return -2;
    s->draws = draws;
    s->n_draws = n_draws;
    s->used = 0;
    s->exhausted = false;
    char body[8] = {1, 2, 3, 4, 5, 6, 7, 8};
    for (uint32_t i = 0; i < n && !s->exhausted; i++) {
        EncHead head;
        const rbuf_t rb = new_buf(8, body, &head);
        const uint32_t before = s->used;
        s->sender_key = 0;
        const int r = s->groups[group]->Send(8, rb);
        sender[i] = r > 0 ? s->sender_key : 0;
        consumed[i] = s->used - before;
    }
    s->draws = nullptr;
    return s->exhausted ? -3 : 0;
}

/* Both pools as they stand, in the maps' own order.  ack_rows [n][6] = src, dst, sp, dp, seq, ack and ack_exp [n];
 * net_rows [n][4] and net_exp [n]; *closed = the accepted sockets that are closing. */
int ref_cc_pools(void *h, uint32_t cap, uint32_t *ack_rows, uint64_t *ack_exp, uint32_t *n_ack, uint32_t *net_rows,
                 uint64_t *net_exp, uint32_t *n_net, uint32_t *closed) {
    State *s = static_cast<State *>(h);
    if (s->pool->mInfoPool.size() > cap || s->mgr->mPool.size() > cap) return -1;
    uint32_t k = 0;
    for (auto &e : s->pool->mInfoPool) {
        const TcpInfo &t = e.first;
        const uint32_t f[6] = {t.src, t.dst, t.sp, t.dp, t.seq, t.ack};
        std::memcpy(ack_rows + 6 * (size_t)k, f, sizeof f);
        ack_exp[k++] = e.second;
    }
    *n_ack = k;
    k = 0;
    for (auto &e : s->mgr->mPool) {
        const TcpInfo &t = e.first;
        const uint32_t f[4] = {t.src, t.dst, t.sp, t.dp};
        std::memcpy(net_rows + 4 * (size_t)k, f, sizeof f);
        net_exp[k++] = e.second.expireMs;
    }
    *n_net = k;
    uint32_t c = 0;
    for (uv_tcp_t *t : s->sockets) c += uv_is_closing((uv_handle_t *)t) ? 1 : 0;  /* no conn is closed before teardown */
    *closed = c;
    return 0;
}

/* The conns made so far, in creation order: group [n], key [n], packet [n], info [n][7]. */
int ref_cc_conns(void *h, uint32_t cap, uint32_t *n, int32_t *group, uint64_t *key, uint32_t *packet, uint32_t *info) {
    State *s = static_cast<State *>(h);
    if (s->conns.size() > cap) return -1;
    for (size_t i = 0; i < s->conns.size(); i++) {
        const Created &r = s->conns[i];
        group[i] = r.group;
        key[i] = r.conn->IntKey();
        packet[i] = r.packet;
        std::memcpy(info + 7 * i, r.info, sizeof r.info);
    }
    *n = (uint32_t)s->conns.size();
    return 0;
}

/* k dials on the client group: tuple [k][4] is what GetTcpInfo gives of the dialled socket (src = the local end).
 * ok[i] = Wait2TransferInfo's return (a miss blocks for wait_ms); key[i] = KeyForConnInfo; info [k][7] = mInfo after
 * Init; found[i] = ConnOfIntKey(key) names the new conn after AddNetConn.  A key the group holds already ends in
 * the reference's assert: -2 before it is tried. */
int ref_cc_dial(void *h, uint32_t k, const uint32_t *tuple, uint32_t wait_ms, uint8_t *ok, uint64_t *key, uint32_t *info,
                uint8_t *found) {
    State *s = static_cast<State *>(h);
    g_st = s;
    for (uint32_t i = 0; i < k; i++) {
        TcpInfo tcpInfo;
        tcpInfo.src = tuple[4 * i];
        tcpInfo.dst = tuple[4 * i + 1];
        tcpInfo.sp = (uint16_t)tuple[4 * i + 2];
        tcpInfo.dp = (uint16_t)tuple[4 * i + 3];
        key[i] = 0;
        found[i] = 0;
        std::memset(info + 7 * (size_t)i, 0, 7 * sizeof(uint32_t));
        ok[i] = s->pool->Wait2TransferInfo(tcpInfo, std::chrono::milliseconds(wait_ms)) ? 1 : 0;
        if (!ok[i]) {
            s->pool->RemoveInfo(tcpInfo);
            continue;
        }
        const IntKeyType kk = KeyGenerator::KeyForConnInfo(tcpInfo);
        if (s->client->ConnOfIntKey(kk)) return -2;
        uv_tcp_t *tcp = new_socket(s);
        if (!tcp) return -4;
        FakeTcp *c = new FakeTcp(tcp, kk, tcpInfo);
        if (c->Init()) return -5;
        s->client->AddNetConn(c);
        Created r;
        r.conn = c;
        r.group = -1;
        r.packet = i;
        const TcpInfo &m = c->mInfo;
        const uint32_t f[7] = {m.src, m.dst, m.sp, m.dp, m.seq, m.ack, m.flag};
        std::memcpy(r.info, f, sizeof f);
        std::memcpy(info + 7 * (size_t)i, f, sizeof f);
        key[i] = kk;
        found[i] = s->client->ConnOfIntKey(kk) == c;
        s->ordinal[c] = -1;
        s->conns.push_back(r);
    }
    return 0;
}

void ref_cc_close(void *h) {
    State *s = static_cast<State *>(h);
    g_st = s;
    s->draws = nullptr;
    for (INetGroup *g : s->groups) unwire_group(g, s);
    unwire_group(s->client, s);
    for (auto &e : s->mgr->mPool)
        if (e.second.conn) s->mgr->closeTcp(e.second.conn);
    s->mgr->mPool.clear();
    delete s->mgr;
    for (ProbeTcp *t : {s->raw_server, s->raw_client}) {  /* never Init()ed, so not Close()d: the base's alone */
        t->IConn::Close();
        delete t;
    }
    delete s->pool;
    uv_run(&s->loop, UV_RUN_DEFAULT);
    uv_loop_close(&s->loop);
    g_st = nullptr;
    delete s;
}

}  // extern "C"
