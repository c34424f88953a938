/*
 * ref_control_harness.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Runs the REFERENCE's own control path, keepalive timer, send pick and conv flush, compiled from
 * /root/reference by oracle/Makefile (`make -C oracle ref` -> oracle/_ref/librsk_ref_control.so; nothing
 * from the reference is copied here):
 *   control  IAppGroup::Input by cmd (conn/IAppGroup.cpp:76-96) -> ConnReset::Input
 *            (callbacks/ConnReset.cpp:43-90) / NetConnKeepAlive::Input (callbacks/NetConnKeepAlive.cpp:37-98)
 *            -> IAppGroup::doSendCmd / SendNetConnReset -> INetGroup::doSend (conn/INetGroup.cpp:111-135)
 *   timer    NetConnKeepAlive::OnFlush (:110-145), KeepAliveRouteObserver::OnNetConnected / OnNetDisconnected
 *   pick     INetGroup::doSend over rand()
 *   flush    IAppGroup::Flush -> IGroup::Flush (conn/IGroup.cpp:81-107) -> IConn::DataStat::Flush
 *            (conn/IConn.cpp:63-79), counters through IConn::Input / IConn::Send
 * One IAppGroup (ClientGroup, or one SubGroup for the server shape) over one INetGroup, wired as
 * ref_demux_harness.cpp's wire_app does, but with the reference's real ConnReset and NetConnKeepAlive.
 *
 * Stand-ins sit only at the ends, behind the reference's own virtual interfaces:
 *   - the net conns are INetConn subclasses that record Send and NotifyErr and then run the base method;
 *   - INetGroup::CreateNetConn returns nullptr (CNetGroup; an SNetGroup without a pooled tcp): a DATA packet
 *     of an unknown connKey takes IAppGroup.cpp:84-86; RemoveConn records and runs the base method;
 *   - IAppGroup::doSendCmd / SendNetConnReset (virtual) record the message and run the base method;
 *   - INetGroup::mHandler is a Handler on a loop that never runs, whose SendMessage queues nothing, so
 *     handleMessage never deletes a conn: the harness owns the conns;
 *   - NetConnKeepAlive::Init() registers with the services and is not called: mRouteObserver is constructed
 *     directly;
 *   - rand() is defined HERE and the library is linked with -Wl,-Bsymbolic-functions, so doSend's draws are
 *     an input array and their number an output; a run that would exhaust the array fails (-3);
 *   - the leaves of the conv flush are the reference's CConn (client) / plain IConns (the SConn position),
 *     with recording Close(); their output callback returns the scripted value, their recv callback nread.
 * Private and protected members are reached by compiling the reference's class headers with both words
 * spelled `public` in THIS translation unit only (layout unchanged), as ref_demux_harness.cpp does.
 * Functions none of this calls (uv timers, libnet, services) stay unresolved; RTLD_LAZY.
 */
#include <arpa/inet.h>
#include <netinet/in.h>
#include <sys/socket.h>
#include <sys/un.h>

#include <algorithm>
#include <array>
#include <cassert>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <random>
#include <set>
#include <sstream>
#include <string>
#include <vector>

#include <uv.h>
#include <plog/Log.h>

#define private public
#define protected public
#include "rscomm.h"
#include "rcommon.h"
#include "bean/EncHead.h"
#include "bean/ConnInfo.h"
#include "bean/TcpInfo.h"
#include "callbacks/IReset.h"
#include "callbacks/INetConnKeepAlive.h"
#include "callbacks/ConnReset.h"
#include "callbacks/NetConnKeepAlive.h"
#include "callbacks/KeepAliveRouteObserver.h"
#include "conn/IConn.h"
#include "conn/INetConn.h"
#include "conn/CConn.h"
#include "conn/IGroup.h"
#include "conn/INetGroup.h"
#include "conn/IAppGroup.h"
#include "server/SubGroup.h"
#include "client/ClientGroup.h"
#include "util/Handler.h"
#include "util/rsutil.h"
#include "src/util/KeyGenerator.h"
#undef protected
#undef private

using namespace std::placeholders;

namespace {

/* ---- the run's state: event log and draws ---------------------------------------------------- */
enum EvKind : int64_t {
    EV_MSG = 1,    /* a doSendCmd / SendNetConnReset: conn = the conn that sent or -1; cmd, body (the first
                      min(len, 8) bytes, little-endian), body length, keyOfConnToReset, draws consumed, the
                      head's IdBuf (little-endian word), the return value */
    EV_NOTIFY = 2, /* INetConn::NotifyErr(code)              (conn, code)                                */
    EV_REMOVE = 3, /* INetGroup::RemoveConn                  (conn)                                      */
    EV_CLOSE = 4,  /* a leaf's Close() from IGroup::CloseConn (leaf)                                     */
};
const int EV_W = 10; /* kind, step, conn, then seven values */

struct Run {
    std::vector<int64_t> ev;
    int64_t step = -1;
    const uint32_t *draws = nullptr;
    uint32_t n_draws = 0, used = 0;
    bool exhausted = false;
    bool leaf_routing = false;
    int out_ret = 0;          /* what the leaves' output callback returns */
    bool scripted_out = false;
    int sender = -1, sender_cmd = 0;
    uint64_t sender_id = 0;
    void add(int64_t kind, int64_t conn, int64_t a = 0, int64_t b = 0, int64_t c = 0, int64_t d = 0, int64_t e = 0,
             int64_t f = 0, int64_t g = 0) {
        const int64_t row[EV_W] = {kind, step, conn, a, b, c, d, e, f, g};
        ev.insert(ev.end(), row, row + EV_W);
    }
};
Run *g_run = nullptr;
bool g_plog = false;

uint64_t word_of(const char *p, size_t n) {
    uint64_t w = 0;
    std::memcpy(&w, p, n < 8 ? n : 8);  /* the build machine is little-endian, as the reference assumes */
    return w;
}

}  // namespace

/* doSend's rand(): the next input draw.  Bound to the reference's objects by -Bsymbolic-functions. */
extern "C" int rand(void) {
    Run *r = g_run;
    if (!r) return 0;
    if (r->used >= r->n_draws) {  /* never wraps: the run fails; walking the indices ends doSend's loop */
        r->exhausted = true;
        return (int)(r->used++ & 0x7fffffffu);
    }
    return (int)(r->draws[r->used++] & 0x7fffffffu);
}

namespace {

/* ---- the recording ends ------------------------------------------------------------------------ */
class CtlNetConn : public INetConn {  /* FakeTcp position */
public:
    CtlNetConn(IntKeyType key, int id) : INetConn(key), mId(id) { mInfo.head = nullptr; }
    bool IsUdp() override { return false; }
    ConnInfo *GetInfo() override { return &mInfo; }
    int Send(ssize_t nread, const rbuf_t &rbuf) override {
        EncHead *hd = static_cast<EncHead *>(rbuf.data);
        g_run->sender = mId;
        g_run->sender_cmd = hd->Cmd();
        IdBufType idb = hd->IdBuf();
        g_run->sender_id = word_of(idb.data(), 8);
        return INetConn::Send(nread, rbuf);
    }
    void NotifyErr(int err) override {
        g_run->add(EV_NOTIFY, mId, err);
        INetConn::NotifyErr(err);
    }
    TcpInfo mInfo;
    int mId;
};

class CtlDefault : public IConn {  /* INetGroup::mDefaultFakeConn */
public:
    CtlDefault() : IConn("default") {}
    int OnRecv(ssize_t nread, const rbuf_t &rbuf) override { return 0; }
};

class CtlNetGroup : public INetGroup {
public:
    explicit CtlNetGroup(const std::string &groupId) : INetGroup(groupId, nullptr) {}
    INetConn *CreateNetConn(IntKeyType key, const ConnInfo *info) override { return nullptr; }
    bool RemoveConn(IConn *conn) override {
        auto *c = dynamic_cast<CtlNetConn *>(conn);
        if (g_run && c) g_run->add(EV_REMOVE, c->mId);
        return INetGroup::RemoveConn(conn);
    }
};

class NullHandler : public Handler {  /* never run: a message sent to it is dropped */
public:
    explicit NullHandler(uv_loop_t *loop) : Handler(loop) {}
    bool SendMessage(const Message &message) override { return true; }
    bool SendMessageAtTime(const Message &msg, uint64_t ts) override { return true; }
};

template <class Base>
class Rec : public Base {  /* the app group: messages recorded on their way down */
public:
    using Base::Base;
    template <class F>
    int record(uint8_t cmd, ssize_t nread, const rbuf_t &rbuf, IntKeyType avoid, F call) {
        Run *r = g_run;
        const uint32_t before = r->used;
        r->sender = -1;
        IdBufType idb = this->mHead.IdBuf();
        const uint64_t own_id = word_of(idb.data(), 8);
        const int n = call();
        const bool sent = r->sender >= 0;
        r->add(EV_MSG, r->sender, sent ? r->sender_cmd : cmd, (int64_t)word_of(rbuf.base, nread > 0 ? (size_t)nread : 0),
               nread, (int64_t)avoid, r->used - before, (int64_t)(sent ? r->sender_id : own_id), n);
        return n;
    }
    int doSendCmd(uint8_t cmd, ssize_t nread, const rbuf_t &rbuf) override {
        return record(cmd, nread, rbuf, 0, [&] { return IAppGroup::doSendCmd(cmd, nread, rbuf); });
    }
    int SendNetConnReset(ssize_t nread, const rbuf_t &rbuf, IntKeyType key) override {
        return record(EncHead::TYPE_NETCONN_RST, nread, rbuf, key,
                      [&] { return IAppGroup::SendNetConnReset(nread, rbuf, key); });
    }
    int OnRecv(ssize_t nread, const rbuf_t &rbuf) override {  /* DATA: routed to the leaves only in the flush run */
        if (g_run->leaf_routing) return Base::OnRecv(nread, rbuf);
        return (int)nread;
    }
};
typedef Rec<ClientGroup> CtlClient;
typedef Rec<SubGroup> CtlSub;

class FlushCConn : public CConn {
public:
    FlushCConn(const std::string &key, const SA *addr, uint32_t conv, int id, std::vector<IConn *> *all)
        : CConn(key, addr, conv), mId(id), mAll(all) {}
    int Close() override {
        if (g_run && (*mAll)[mId]) g_run->add(EV_CLOSE, mId);
        (*mAll)[mId] = nullptr;
        return CConn::Close();
    }
    int mId;
    std::vector<IConn *> *mAll;
};

class FlushLeaf : public IConn {
public:
    FlushLeaf(const std::string &key, int id, std::vector<IConn *> *all) : IConn(key), mId(id), mAll(all) {}
    int Close() override {
        if (g_run && (*mAll)[mId]) g_run->add(EV_CLOSE, mId);
        (*mAll)[mId] = nullptr;
        return IConn::Close();
    }
    int mId;
    std::vector<IConn *> *mAll;
};

/* ---- one group ---------------------------------------------------------------------------------- */
enum : uint8_t { F_ALIVE = 1, F_NEW = 2 };

struct Stack {
    uv_loop_t loop;
    CtlNetGroup *net = nullptr;
    IAppGroup *app = nullptr;
    CtlClient *cli = nullptr;
    CtlSub *sub = nullptr;
    ConnReset *reset = nullptr;
    NetConnKeepAlive *ka = nullptr;
    std::vector<CtlNetConn *> conns;  /* every net conn ever added, removed from the group or not */
    std::vector<IConn *> leaves;      /* the flush run's leaves; nullptr once closed */
    IdBufType idb;
    struct sockaddr_in target;

    Stack(int shape, uint32_t n_conn, const uint64_t *keys, const uint8_t *flags, const uint64_t *est, const uint8_t *id) {
        uv_loop_init(&loop);
        std::memset(&target, 0, sizeof target);
        target.sin_family = AF_INET;
        target.sin_port = htons(10001);
        target.sin_addr.s_addr = htonl(0x7f000001);
        std::memcpy(idb.data(), id, 8);
        net = new CtlNetGroup("net");
        if (shape == 0) {
            sub = new CtlSub("server01", nullptr, (const struct sockaddr *)&target, net, nullptr);
            app = sub;
        } else {
            cli = new CtlClient("client01", "", "", 0, nullptr, net, nullptr);
            app = cli;
        }
        app->mHead.SetIdBuf(idb);  /* IAppGroup's constructor: Str2IdBuf(groupId) */
        app->IGroup::Init();
        net->IGroup::Init();
        net->mDefaultFakeConn = new CtlDefault();
        net->mDefaultFakeConn->Init();
        net->mHandler = std::make_shared<NullHandler>(&loop);
        net->SetOutputCb(std::bind(&IConn::Output, app, _1, _2));
        net->SetOnRecvCb(std::bind(&IConn::OnRecv, app, _1, _2));
        app->SetOutputCb([](ssize_t nread, const rbuf_t &) { return (int)nread; });  /* the RConn below */
        reset = new ConnReset(app);
        ka = new NetConnKeepAlive(app, reset, 1000);
        ka->mRouteObserver = new KeepAliveRouteObserver(ka);
        app->mResetHelper = reset;
        app->mKeepAlive = ka;
        for (uint32_t k = 0; k < n_conn; k++) {
            auto *c = new CtlNetConn(keys[k], (int)k);
            c->Init();
            c->mAlive = (flags[k] & F_ALIVE) != 0;
            c->mNew = (flags[k] & F_NEW) != 0;
            const_cast<uint64_t &>(c->mEstablishedTimeStampMs) = est ? est[k] : 0;
            conns.push_back(c);
            net->AddNetConn(c);
        }
    }

    void add_leaf(int shape, uint32_t conv, uint32_t dst) {
        const int id = (int)leaves.size();
        auto out = [](ssize_t nread, const rbuf_t &) { return g_run->scripted_out ? g_run->out_ret : (int)nread; };
        auto rcv = [](ssize_t nread, const rbuf_t &) { return (int)nread; };
        if (shape == 0) {
            auto *leaf = new FlushLeaf(KeyGenerator::BuildConvKey(dst, conv), id, &leaves);
            leaf->Init();
            leaves.push_back(leaf);
            sub->AddConn(leaf, out, rcv);
        } else {  /* ClientGroup::newConn (client/ClientGroup.cpp:206-217) */
            struct sockaddr_in a = target;
            a.sin_port = htons((uint16_t)(20000 + id % 40000));
            a.sin_addr.s_addr = htonl(0x7f000001 + (uint32_t)(id / 40000));
            auto *leaf = new FlushCConn(CConn::BuildKey((const SA *)&a), (const SA *)&a, conv, id, &leaves);
            leaf->Init();
            leaves.push_back(leaf);
            cli->AddConn(leaf, out, rcv);
            cli->mConvMap.insert({conv, leaf});
        }
    }

    int index_of(IConn *c) {
        auto *n = dynamic_cast<CtlNetConn *>(c);
        return n ? n->mId : -1;
    }

    ~Stack() {
        Run *keep = g_run;
        g_run = nullptr;  /* teardown is not part of the record */
        for (size_t i = 0; i < leaves.size(); i++) {
            IConn *c = leaves[i];
            if (!c) continue;
            app->RemoveConn(c);
            c->Close();
            delete c;
        }
        for (CtlNetConn *c : conns) {
            if (net->ConnOfIntKey(c->IntKey()) == c) net->INetGroup::RemoveConn(c);
            c->Close();
            delete c;
        }
        net->mDefaultFakeConn->Close();
        delete net->mDefaultFakeConn;
        net->mDefaultFakeConn = nullptr;
        net->mHandler = nullptr;
        net->IConn::Close();
        delete ka->mRouteObserver;
        ka->mRouteObserver = nullptr;
        delete ka;
        delete reset;
        app->mKeepAlive = nullptr;
        app->mResetHelper = nullptr;
        app->IConn::Close();
        app->mFakeNetGroup = nullptr;
        if (sub && sub->mTarget) {
            free(sub->mTarget);
            sub->mTarget = nullptr;
        }
        delete net;
        delete app;
        uv_loop_close(&loop);
        g_run = keep;
    }

    /* one packet through IConn::Input of the app group, as RConn's recv callback does */
    int input(uint8_t cmd, const uint8_t *id, uint32_t conv, uint64_t conn_key, uint32_t dst, const char *body, int nread) {
        EncHead head;
        head.SetCmd(cmd);
        IdBufType b;
        std::memcpy(b.data(), id, 8);
        head.SetIdBuf(b);
        head.SetConv(conv);
        head.SetConnKey(conn_key);
        TcpInfo info;
        info.src = 0x0100000a;
        info.dst = dst;
        info.sp = 10001;
        info.dp = 43932;
        info.head = &head;
        const rbuf_t rb = new_buf(nread, body, &info);
        return app->Input(nread, rb);
    }
};

void start(Run &run, const uint32_t *draws, uint32_t n_draws) {
    if (!g_plog) {
        plog::init(plog::none);
        g_plog = true;
    }
    run.draws = draws;
    run.n_draws = n_draws;
    g_run = &run;
}

int finish(Run &run, int64_t *ev, uint32_t ev_cap, uint32_t *n_ev, uint32_t *draws_used) {
    g_run = nullptr;
    if (run.exhausted) return -3;
    if (run.ev.size() / EV_W > ev_cap) return -1;
    if (!run.ev.empty()) std::memcpy(ev, run.ev.data(), run.ev.size() * sizeof(int64_t));
    *n_ev = (uint32_t)(run.ev.size() / EV_W);
    *draws_used = run.used;
    return 0;
}

int copy_reqs(NetConnKeepAlive *ka, uint64_t *keys, int32_t *tries, uint32_t cap, uint32_t *n) {
    if (ka->mReqMap.size() > cap) return -1;
    uint32_t k = 0;
    for (auto &e : ka->mReqMap) {
        keys[k] = e.first;
        tries[k++] = e.second;
    }
    *n = k;
    return 0;
}

}  // namespace

extern "C" {

/* Every entry: shape 0 = one SubGroup (server), 1 = ClientGroup.  The group's net conns are keys[c] with
 * flags[c] (1 alive, 2 new) and est[c] (mEstablishedTimeStampMs; may be NULL), c < n_conn; id[8] is the
 * group's IdBuf.  ev receives EV_W int64 per event (see EvKind).  Returns 0; -1 a capacity is too small;
 * -2 the run would enter doSend's endless loop; -3 the draws ran out; -4 a script names a closed leaf. */

/* A batch of decoded packets through top->Input, with mReqMap = req_keys / req_tries before it.
 * Packet i: cmd[i], pid[8i..], conv[i], conn_key[i] (the head's), body bytes body[body_off[i] ..
 * + body_len[i]) with nread = body_len[i].
 * ret[i] = Input's return; look[i] = the conn INetGroup::ConnOfIntKey names for the body's key just before
 * the packet (cmd 2, 3, 4 with a full body; -1 when none, -2 when not looked at). */
int ref_control_run(int shape, uint32_t n_conn, const uint64_t *keys, const uint8_t *flags, const uint64_t *est,
                    const uint8_t *id, uint32_t n_req, const uint64_t *req_keys, const int32_t *req_tries, uint32_t n,
                    const uint8_t *cmd, const uint8_t *pid, const uint32_t *conv, const uint64_t *conn_key,
                    const uint8_t *body, const uint64_t *body_off, const int32_t *body_len, const uint32_t *draws,
                    uint32_t n_draws, int32_t *ret, int32_t *look, int64_t *ev, uint32_t ev_cap, uint32_t *n_ev,
                    uint64_t *req_keys_out, int32_t *req_tries_out, uint32_t req_cap, uint32_t *n_req_out,
                    uint32_t *draws_used) {
    Run run;
    start(run, draws, n_draws);
    int rc = 0;
    {
        Stack s(shape, n_conn, keys, flags, est, id);
        for (uint32_t k = 0; k < n_req; k++) s.ka->mReqMap.emplace(req_keys[k], req_tries[k]);
        for (uint32_t i = 0; i < n && !run.exhausted; i++) {
            run.step = i;
            const char *b = (const char *)body + body_off[i];
            look[i] = -2;
            IntKeyType k = 0;
            if (cmd[i] >= 2 && cmd[i] <= 4 && KeyGenerator::DecodeKeySafe(body_len[i], b, &k) > 0)
                look[i] = s.index_of(s.net->ConnOfIntKey(k));
            ret[i] = s.input(cmd[i], pid + 8ull * i, conv[i], conn_key[i], 0x0200000a, b, body_len[i]);
        }
        rc = copy_reqs(s.ka, req_keys_out, req_tries_out, req_cap, n_req_out);
    }
    const int rf = finish(run, ev, ev_cap, n_ev, draws_used);
    return rf ? rf : rc;
}

/* A script of steps on the group: op 0 OnFlush(arg); 1 a KEEP_ALIVE_RESP packet for key arg; 2 the conn of
 * key arg removed from the group (INetGroup::RemoveConn); 3 its mNew cleared; 4 OnNetConnected (arg != 0) /
 * OnNetDisconnected; 5 INetGroup::Flush(arg), which removes the dead conns (IAppGroup::Flush's second half).
 * After every OnFlush mReqMap is appended to snap_*: (step, key, tries) per entry. */
int ref_keepalive_run(int shape, uint32_t n_conn, const uint64_t *keys, const uint8_t *flags, const uint64_t *est,
                      const uint8_t *id, uint32_t n_req, const uint64_t *req_keys, const int32_t *req_tries, int online,
                      uint32_t n_steps, const uint8_t *op, const uint64_t *arg, const uint32_t *draws, uint32_t n_draws,
                      int64_t *ev, uint32_t ev_cap, uint32_t *n_ev, int64_t *snap_step, uint64_t *snap_key,
                      int32_t *snap_tries, uint32_t snap_cap, uint32_t *n_snap, uint32_t *draws_used) {
    Run run;
    start(run, draws, n_draws);
    int rc = 0;
    uint32_t ns = 0;
    {
        Stack s(shape, n_conn, keys, flags, est, id);
        for (uint32_t k = 0; k < n_req; k++) s.ka->mReqMap.emplace(req_keys[k], req_tries[k]);
        s.ka->mRouteObserver->mAlive = online != 0;
        for (uint32_t i = 0; i < n_steps && !run.exhausted && rc == 0; i++) {
            run.step = i;
            INetConn *c = s.net->ConnOfIntKey(arg[i]);
            switch (op[i]) {
                case 0: {
                    s.ka->OnFlush(arg[i]);
                    for (auto &e : s.ka->mReqMap) {
                        if (ns >= snap_cap) { rc = -1; break; }
                        snap_step[ns] = i;
                        snap_key[ns] = e.first;
                        snap_tries[ns++] = e.second;
                    }
                    break;
                }
                case 1: {
                    char b[8];
                    KeyGenerator::EncodeKey(b, arg[i]);
                    uint8_t idb[8];
                    std::memcpy(idb, id, 8);
                    s.input(EncHead::TYPE_KEEP_ALIVE_RESP, idb, 0, 0, 0x0200000a, b, 8);
                    break;
                }
                case 2:
                    if (c) s.net->RemoveConn(c);
                    break;
                case 3:
                    if (c) c->mNew = false;
                    break;
                case 4:
                    if (arg[i]) s.ka->mRouteObserver->OnNetConnected("eth0", "10.0.0.1");
                    else s.ka->mRouteObserver->OnNetDisconnected();
                    break;
                case 5:
                    s.net->Flush(arg[i]);
                    break;
                default:
                    rc = -1;
            }
        }
    }
    *n_snap = ns;
    const int rf = finish(run, ev, ev_cap, n_ev, draws_used);
    return rf ? rf : rc;
}

/* n sends on the group: avoid[i] != 0 goes down IAppGroup::SendNetConnReset(.., avoid[i]), 0 down
 * IAppGroup::doSendCmd(KEEP_ALIVE_REQ).  One EV_MSG per send.  order[0..n_conn) = the conns in mConns
 * iteration order before the first send. */
int ref_dosend_run(int shape, uint32_t n_conn, const uint64_t *keys, const uint8_t *flags, const uint8_t *id, uint32_t n,
                   const uint64_t *avoid, const uint32_t *draws, uint32_t n_draws, int64_t *ev, uint32_t ev_cap,
                   uint32_t *n_ev, int32_t *order, uint32_t *draws_used) {
    Run run;
    start(run, draws, n_draws);
    int rc = 0;
    {
        Stack s(shape, n_conn, keys, flags, nullptr, id);
        uint32_t k = 0;
        for (auto &e : s.net->mConns) order[k++] = s.index_of(e.second);
        char b[8] = {1, 2, 3, 4, 5, 6, 7, 8};
        for (uint32_t i = 0; i < n && !run.exhausted; i++) {
            run.step = i;
            if (avoid[i] != 0) {  /* the loop that never ends: only the avoided conn is alive */
                bool other = false, self = false;
                for (auto &e : s.net->mConns) {
                    auto *c = dynamic_cast<INetConn *>(e.second);
                    if (!c->Alive()) continue;
                    if (c->IntKey() == avoid[i]) self = true; else other = true;
                }
                if (self && !other) { rc = -2; break; }
            }
            const rbuf_t rb = new_buf(8, b, nullptr);
            if (avoid[i] != 0) s.app->SendNetConnReset(8, rb, avoid[i]);
            else s.app->doSendCmd(EncHead::TYPE_KEEP_ALIVE_REQ, 8, rb);
        }
    }
    const int rf = finish(run, ev, ev_cap, n_ev, draws_used);
    return rf ? rf : rc;
}

/* Rounds on the leaves convs[0..n_conv) of the group (dst: the server leaves' BuildConvKey address).
 * Round r: the packets in_conv[in_off[r] .. in_off[r+1]) as DATA of the first net conn's key through
 * top->Input (in_ret receives each return); the sends out_leaf[out_off[r] .. out_off[r+1]) through the
 * leaf's Send with the output callback returning out_ret[k]; then IAppGroup::Flush(now[r]).
 * After the flush of round r: alive[r*n_conv + c] = the leaf's Alive(), -1 once it is closed;
 * counters[(r*n_conv + c)*4 ..] = curr_in, curr_out, prev_in, prev_out of a leaf still there. */
int ref_convflush_run(int shape, uint32_t n_conn, const uint64_t *keys, const uint8_t *flags, const uint8_t *id,
                      uint32_t n_conv, const uint32_t *convs, uint32_t dst, uint32_t n_rounds, const uint32_t *in_off,
                      const uint32_t *in_conv, const uint32_t *out_off, const uint32_t *out_leaf, const int32_t *out_ret,
                      const uint64_t *now, const uint32_t *draws, uint32_t n_draws, int32_t *in_ret, int8_t *alive,
                      uint32_t *counters, int64_t *ev, uint32_t ev_cap, uint32_t *n_ev, uint32_t *draws_used) {
    if (n_conn == 0) return -1;
    Run run;
    start(run, draws, n_draws);
    run.leaf_routing = true;
    run.scripted_out = true;
    int rc = 0;
    {
        Stack s(shape, n_conn, keys, flags, nullptr, id);
        for (uint32_t c = 0; c < n_conv; c++) s.add_leaf(shape, convs[c], dst);
        char payload[32];
        std::memset(payload, 0x5a, sizeof payload);
        for (uint32_t r = 0; r < n_rounds && rc == 0 && !run.exhausted; r++) {
            run.step = r;
            for (uint32_t k = in_off[r]; k < in_off[r + 1]; k++)
                in_ret[k] = s.input(EncHead::TYPE_DATA, id, in_conv[k], keys[0], dst, payload, 32);
            for (uint32_t k = out_off[r]; k < out_off[r + 1]; k++) {
                IConn *leaf = out_leaf[k] < n_conv ? s.leaves[out_leaf[k]] : nullptr;
                if (!leaf) { rc = -4; break; }
                run.out_ret = out_ret[k];
                const rbuf_t rb = new_buf(32, payload, nullptr);
                leaf->Send(32, rb);
            }
            if (rc) break;
            s.app->Flush(now[r]);
            for (uint32_t c = 0; c < n_conv; c++) {
                IConn *leaf = s.leaves[c];
                const size_t at = (size_t)r * n_conv + c;
                alive[at] = leaf ? (int8_t)leaf->Alive() : (int8_t)-1;
                uint32_t *q = counters + 4 * at;
                q[0] = leaf ? leaf->mStat.curr_in : 0;
                q[1] = leaf ? leaf->mStat.curr_out : 0;
                q[2] = leaf ? leaf->mStat.prev_in : 0;
                q[3] = leaf ? leaf->mStat.prev_out : 0;
            }
        }
    }
    const int rf = finish(run, ev, ev_cap, n_ev, draws_used);
    return rf ? rf : rc;
}

}  // extern "C"
