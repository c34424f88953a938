"""TEST INFRASTRUCTURE: the walk.  A plain-Python rsock server that handles ONE packet, ONE send or ONE timer tick at
a time, in the containers the reference holds, written from INTEGRATION.md and the reference lines it cites:

  ack pool      dict keyed by the 4-tuple (src, sp, dst, dp)      TcpAckPool::mInfoPool      (net/TcpAckPool.cpp)
  socket pool   dict keyed by the same tuple                      ServerNetManager::mPool    (server/ServerNetManager.cpp)
  conns         one dict per IdBuf, keyed by connKey              INetGroup::mConnMap        (conn/INetGroup.cpp:57-83)
  convs         one dict per IdBuf, keyed by (dst, conv)          SubGroup::mConns           (server/SubGroup.cpp:31-68)
  closed        the sockets closed so far, by tuple

It imports none of the per-call batch rules (pool_ref, conn_create_ref, control_ref, conn_close_ref, conv_ref,
conv_create_ref, conv_close_ref, pick_ref, demux_ref, deliver_ref) and knows nothing of tiles, indexes or scratch.

What it takes from the batch interface, because the reference has no such thing, is stated here once:
  * Row numbers.  The reference keeps maps; the tables have rows.  A new pool entry, conn or conv takes the lowest
    vacant row in first-arrival order.  A row vacated inside an event (a consumed or purged pool entry, a conv closed
    by a CONV_RST, anything a tick removes) is vacant from the NEXT event on -- the settle runs behind the adds, and a
    reset conv's row is held until the host clears it after the batch.  Convs get their rows at the end of a capture:
    first the convs born of keys the table did not know, then the convs reborn behind a reset, each in arrival order
    (the two rsk_conv_create_batch calls of the chain).
  * Sends happen behind the event.  The answers a capture causes and the requests a keepalive tick causes are queued
    and picked after the event (side effects run at batch completion, in input order), from the
    conns alive THEN.  The pick is a function of a draw column: candidate draw % m of the group's alive conns in row
    order, the avoid rule of rsk_conn_pick_batch (k = d % (m - 1), k += k >= p).  The reference's rejection sampling
    and its removal of a dead conn it drew are not modelled: a dead conn leaves at the next keepalive tick.
  * A FIN / RST packet on a server is the host's (ServerGroup::OnTcpFinOrRst walks every SubGroup): RECV_CLOSE, no
    table effect here or there.
  * The keepalive tick visits the conns in row order (the reference: mConns order); IGroup::Flush's removal of the
    conns that are not alive runs behind NetConnKeepAlive::OnFlush in the same tick.

DOCUMENTED DEVIATIONS.  The batch calls deviate from a walk in the ways listed below.  The walk DETECTS each and
raises SessionDeviation naming the packet; it neither skips the packet nor emulates the batch rule.

  deviation                                                                  covered on its own by
  a refused key whose later packet carries another tuple that has an offer   conncreate.npz `deviation_other_tuple`
                                                                             (test_conncreate_golden.py)
  a tuple's DATA packet ahead of its own handshake in one capture            conncreate.npz `half_offers`, `refused_syn`
                                                                             (test_pool_host.py: the settle's purge)
  a packet that names (by key or in a control body) a conn that an earlier
    packet of the same batch reset or created (DATA packets of the key a
    packet of the batch created are the create's step 8 and agree)           test_control_golden_host.py::
                                                                             test_snapshot_question, test_host_walk
  a CONV_RST naming a conv born in the same batch                            test_conv_close_host.py::test_deviations
  a conv reset twice in one batch with DATA between the resets               `n_rst_again`: test_conv_close_host.py::
                                                                             test_deviations
  a keepalive request carried by a conn that is still new in the same flush  test_control_golden_host.py::
                                                                             test_flush_model_on_the_fixture
  a pick group whose only alive conn is the one to avoid                     test_pick_host.py::test_host_avoid_keys
  a table or pool that runs full                                             test_conv_create_host.py::test_table_full,
                                                                             pool_ref.CASES `pool_full`, the creates' n_full
  u_max below the batch's unknowns                                           test_conv_create_host.py::
                                                                             test_u_max_repeated_calls, test_conn_create_host.py::
                                                                             test_repeat_loop_reaches_the_one_call_result
(the last one cannot arise in the walk: the session's driver always passes u_max = n.)"""
from __future__ import annotations

import heapq

LIVE, ALIVE, NEW = 0x1, 0x2, 0x4
TH_FIN, TH_SYN, TH_RST, TH_ACK = 0x01, 0x02, 0x04, 0x10
PARSE_DROP, PARSE_DELIVER, PARSE_SYN = 0, 1, 2
VALID, CLOSE, DROP = 1, 0, -1
DATA, CONV_RST, NETCONN_RST, KA_REQ, KA_RESP = 0, 1, 2, 3, 4
K_NONE, K_CONV_RST, K_NETCONN_RST, K_KA_REQ, K_KA_RESP, K_TCP_CLOSE, K_SHORT, K_UNKNOWN = range(8)
NONE = 0xFFFFFFFF
KA_NONE = 0xFF
HEAD = 31                 # 8-byte tag + 23-byte EncHead in front of every payload
KA_DELAY_MS, KA_MAX_RETRY = 15000, 3
M32 = 0xFFFFFFFF


class SessionDeviation(Exception):
    """The traffic entered one of the documented deviations (module docstring); .what names it, .packet the packet."""

    def __init__(self, what, packet=None):
        super().__init__(f"{what} (packet {packet})")
        self.what, self.packet = what, packet


class Packet:
    """What a sender put on the wire: the IPv4 / TCP fields and, for a frame, the EncHead and the payload."""

    __slots__ = ("ip_src", "ip_dst", "sport", "dport", "th_seq", "th_ack", "flags", "cmd", "id8", "conv", "key", "payload",
                 "corrupt")

    def __init__(self, ip_src, ip_dst, sport, dport, th_seq, th_ack, flags, cmd=0, id8=b"", conv=0, key=0, payload=b"",
                 corrupt=False):
        self.ip_src, self.ip_dst, self.sport, self.dport = ip_src, ip_dst, sport, dport
        self.th_seq, self.th_ack, self.flags = th_seq & M32, th_ack & M32, flags
        self.cmd, self.id8, self.conv, self.key, self.payload, self.corrupt = cmd, bytes(id8), conv, key, bytes(payload), corrupt


class Rows:
    """The rows of one table: the lowest vacant one first; a row given back is vacant from the next event on."""

    def __init__(self, capacity, what):
        self.free, self.pending, self.what = list(range(capacity)), [], what
        heapq.heapify(self.free)

    def take(self, packet=None):
        if not self.free:
            raise SessionDeviation(f"{self.what} runs full", packet)
        return heapq.heappop(self.free)

    def give(self, row):
        self.pending.append(row)

    def end_event(self):
        for r in self.pending:
            heapq.heappush(self.free, r)
        self.pending = []


class Conn:
    __slots__ = ("row", "id8", "key", "tup", "seq", "ack", "flag", "alive", "new", "ka", "est")


class Conv:
    __slots__ = ("row", "id8", "dst", "conv", "cur_in", "cur_out", "prev_in", "prev_out", "alive", "stream", "born_in")


class Walk:
    def __init__(self, cap_conn, cap_conv, cap_ack, cap_sock, persist_ms=1000):
        self.persist = persist_ms
        self.r_conn, self.r_conv = Rows(cap_conn, "the conn table"), Rows(cap_conv, "the conv table")
        self.r_ack, self.r_sock = Rows(cap_ack, "the ack pool"), Rows(cap_sock, "the socket pool")
        self.ack_pool, self.sock_pool = {}, {}      # tuple -> [row, seq, ack, expiry] / [row, expiry]
        self.conns, self.convs = {}, {}             # id8 -> {key: Conn} / {(dst, conv): Conv}
        self.conn_at, self.conv_at = {}, {}         # row -> object
        self.bound = {}                             # conn row -> the tuple of its socket
        self.closed = []                            # tuples of the sockets closed, in order
        self.conv_closed = []                       # (row, id8, dst, conv) of the convs closed, in order
        self.ip_id = 0
        self.queue = []                             # the messages waiting for their pick
        self.event = 0
        self.seen = dict.fromkeys(("conns_born", "conns_reset", "conns_timed_out", "rows_reused", "convs_born", "convs_reset",
                                   "convs_reborn", "offers_refused", "pool_expired", "ka_answers", "csum_drops"), 0)
        self.used_rows = {"conn": set(), "conv": set(), "ack": set(), "sock": set()}

    # ---- helpers --------------------------------------------------------------------------------------------------
    def _end_event(self):
        for r in (self.r_conn, self.r_conv, self.r_ack, self.r_sock):
            r.end_event()
        self.event += 1

    def _take(self, which, rows, packet=None):
        r = rows.take(packet)
        if r in self.used_rows[which]:
            self.seen["rows_reused"] += 1
        self.used_rows[which].add(r)
        return r

    @staticmethod
    def parse(p):
        """RawTcp::RawInput on a server with the ack pool: -> (parse_status, src, dst, sp, dp, seq, ack).  A received
        packet's TcpInfo is stored the way the answer travels (src = the packet's destination); a SYN row is
        Reverse()d again, addresses, ports and seq <-> ack (conn/RawTcp.cpp:221-227)."""
        src, dst, sp, dp = p.ip_dst, p.ip_src, p.dport, p.sport
        if p.flags & TH_SYN:
            return PARSE_SYN, dst, src, dp, sp, p.th_ack, p.th_seq
        n = HEAD + len(p.payload) if p.id8 else 0
        close = p.flags & (TH_FIN | TH_RST)
        if n < 9 and not close:
            return PARSE_DROP, 0, 0, 0, 0, 0, 0
        return PARSE_DELIVER, src, dst, sp, dp, (p.th_seq + n) & M32, p.th_ack

    # ---- ServerNetManager::add2Pool -------------------------------------------------------------------------------
    def accept(self, tuples, now):
        """The sockets accepted since the last batch; a second accept of a pooled tuple changes nothing."""
        out = []
        for t in tuples:
            t = tuple(int(x) for x in t)  # (src, sp, dst, dp)
            if t[1] == 0 or t[3] == 0:
                out.append(NONE)
                continue
            e = self.sock_pool.get(t)
            if e is None:
                e = self.sock_pool[t] = [self._take("sock", self.r_sock), now + self.persist]
            out.append(e[0])
        self._end_event()
        return out

    # ---- one capture, packet by packet ----------------------------------------------------------------------------
    def capture(self, packets, now):
        n = len(packets)
        o = {k: [v] * n for k, v in (("parse_status", PARSE_DROP), ("status", DROP), ("conn", None), ("hit", 0), ("miss", DROP),
                                    ("kind", K_NONE), ("arg", 0), ("cconn", None), ("conv", None))}
        cnt = dict.fromkeys(("a_new", "a_again", "a_zero_port", "n_bad", "n_new", "n_refused", "n_ctl", "purged_ack",
                             "closed_socks", "v_new", "v_reborn", "v_closed", "n_reopened", "n_rst_again"), 0)
        touched, named, refused, data_tuples = {}, set(), set(), set()
        closed_convs, born, reborn = {}, [], []
        taken, closed_now, conv_closed_now, conn_first = [], [], [], []
        first_msg = len(self.queue)
        for i, p in enumerate(packets):
            st, src, dst, sp, dp, seq, ack = self.parse(p)
            o["parse_status"][i] = st
            tup = (src, sp, dst, dp)
            if st == PARSE_SYN:  # TcpAckPool::AddInfoFromPeer: the first handshake wins, a later one moves the expiry
                if sp == 0 or dp == 0:
                    cnt["a_zero_port"] += 1
                    continue
                if tup in data_tuples:
                    raise SessionDeviation("a tuple's DATA packet ahead of its own handshake in one capture", i)
                e = self.ack_pool.get(tup)
                if e is None:
                    self.ack_pool[tup] = [self._take("ack", self.r_ack, i), seq, ack, now + self.persist]
                    cnt["a_new"] += 1
                else:
                    e[3] = now + self.persist
                    cnt["a_again"] += 1
                continue
            if st != PARSE_DELIVER:
                continue
            if p.flags & (TH_FIN | TH_RST):
                o["status"][i] = CLOSE
                continue
            if p.corrupt:  # the kernel's TCP input would have dropped it
                cnt["n_bad"] += 1
                self.seen["csum_drops"] += 1
                continue
            o["status"][i] = VALID
            gk = p.id8
            if p.cmd == DATA:
                group = self.conns.setdefault(gk, {})
                c = group.get(p.key)
                if c is not None and touched.get((gk, p.key)) == "reset":
                    raise SessionDeviation("a packet names a conn that an earlier packet of the batch reset", i)
                if c is None:  # INetGroup::Input's miss path -> SNetGroup::CreateNetConn -> ServerNetManager::GetTcp
                    if (gk, p.key) in named:
                        raise SessionDeviation("a control body named the conn a later packet of the batch creates", i)
                    rec, sock = self.ack_pool.get(tup), self.sock_pool.get(tup)
                    data_tuples.add(tup)
                    if rec is not None and sock is not None:
                        if (gk, p.key) in refused:
                            raise SessionDeviation("a refused key whose later packet carries a tuple that has an offer", i)
                        c = Conn()
                        c.row, c.id8, c.key, c.tup = self._take("conn", self.r_conn, i), gk, p.key, tup
                        c.seq, c.ack, c.flag = (rec[2] + 1) & M32, (rec[2] + 2) & M32, TH_ACK
                        c.alive, c.new, c.ka, c.est = True, True, None, now
                        group[p.key] = self.conn_at[c.row] = c
                        del self.ack_pool[tup], self.sock_pool[tup]
                        self.r_ack.give(rec[0])
                        self.r_sock.give(sock[0])
                        self.bound[c.row] = tup
                        taken.append((sock[0], c.row))
                        conn_first.append(i)
                        touched[(gk, p.key)] = "created"
                        cnt["n_new"] += 1
                        self.seen["conns_born"] += 1
                    else:  # CreateNetConn returns nullptr: GetTcp empties what one pool holds of the tuple
                        if (gk, p.key) not in refused:
                            refused.add((gk, p.key))
                            cnt["n_refused"] += 1
                            self.seen["offers_refused"] += 1
                        if rec is not None:
                            del self.ack_pool[tup]
                            self.r_ack.give(rec[0])
                            cnt["purged_ack"] += 1
                        if sock is not None:
                            del self.sock_pool[tup]
                            self.r_sock.give(sock[0])
                            self.closed.append(tup)
                            closed_now.append(sock[0])
                            cnt["closed_socks"] += 1
                        o["miss"][i] = VALID
                        self.queue.append((NETCONN_RST, p.key, gk, p.key, i))  # IAppGroup.cpp:84-86
                        continue
                o["conn"][i], o["hit"][i] = c, 1
                if c.ack < seq:  # FakeTcp::OnRecv
                    c.ack = seq
                cg = self.convs.setdefault(gk, {})  # SubGroup::OnRecv by BuildConvKey(dst, conv)
                ck = (dst, p.conv)
                v = cg.get(ck)
                if v is None:
                    v = Conv()
                    v.row, v.id8, v.dst, v.conv = None, gk, dst, p.conv
                    v.cur_in = v.cur_out = v.prev_in = v.prev_out = 0
                    v.alive, v.stream, v.born_in = 1, [], self.event
                    cg[ck] = v
                    if (gk, ck) in closed_convs:
                        reborn.append((v, i))
                        closed_convs[(gk, ck)] = "reborn"
                    else:
                        born.append((v, i))
                if (gk, ck) in closed_convs:  # a packet behind its conv's reset: it goes to the reborn conv
                    cnt["n_reopened"] += 1
                v.cur_in = (v.cur_in + 1) & M32
                v.stream.append(p.payload)
                o["conv"][i] = v
                continue
            # control packets: IAppGroup::Input's other branches
            cnt["n_ctl"] += 1
            body = p.payload
            if p.cmd > KA_RESP:
                o["kind"][i] = K_UNKNOWN
                continue
            if len(body) < (4 if p.cmd == CONV_RST else 8):
                o["kind"][i] = K_SHORT
                continue
            if p.cmd == CONV_RST:  # ConnReset::OnRecvConvRst -> IGroup::CloseConn
                conv = int.from_bytes(body[:4], "little")
                o["kind"][i], o["arg"][i] = K_CONV_RST, conv
                ck = (dst, conv)
                v = self.convs.get(gk, {}).get(ck)
                if v is None:
                    if (gk, ck) in closed_convs:
                        cnt["n_rst_again"] += 1
                    continue
                if v.row is None:
                    what = ("a conv reset twice in one batch with DATA between the resets" if (gk, ck) in closed_convs
                            else "a CONV_RST naming a conv born in the same batch")
                    raise SessionDeviation(what, i)
                del self.convs[gk][ck]
                del self.conv_at[v.row]
                self.r_conv.give(v.row)
                self.conv_closed.append((v.row, gk, dst, conv))
                conv_closed_now.append(v.row)
                closed_convs[(gk, ck)] = "closed"
                o["conv"][i] = v
                cnt["v_closed"] += 1
                self.seen["convs_reset"] += 1
                continue
            key = int.from_bytes(body[:8], "little")
            o["kind"][i], o["arg"][i] = p.cmd, key  # the CTL_* codes of cmd 2..4 are the cmd values
            if (gk, key) in touched:
                raise SessionDeviation("a control body names a conn that an earlier packet of the batch reset or created", i)
            named.add((gk, key))
            c = self.conns.get(gk, {}).get(key)
            o["cconn"][i] = c
            if p.cmd == NETCONN_RST:  # ConnReset::OnRecvNetConnRst -> INetConn::NotifyErr: dead, still in mConnMap
                if c is not None:
                    if c.alive:
                        self.seen["conns_reset"] += 1
                    c.alive = False
                    touched[(gk, key)] = "reset"
            elif p.cmd == KA_REQ:  # NetConnKeepAlive::Input
                self.queue.append((KA_RESP, key, gk, 0, i) if c is not None else (NETCONN_RST, key, gk, key, i))
                self.seen["ka_answers"] += 1
            elif c is not None:  # KA_RESP: RemoveRequest
                c.ka = None
        for v, _i in born + reborn:
            v.row = self._take("conv", self.r_conv, _i)
            self.conv_at[v.row] = v
        cnt["v_new"], cnt["v_reborn"] = len(born), len(reborn)
        self.seen["convs_born"] += len(born)
        self.seen["convs_reborn"] += len(reborn)
        row = lambda x: NONE if x is None else x.row  # noqa: E731
        res = dict(o, conn=[row(c) for c in o["conn"]], cconn=[row(c) for c in o["cconn"]], conv_row=[row(v) for v in o["conv"]],
                   counts=cnt, taken=taken, closed_sock_rows=sorted(closed_now), conv_closed_rows=sorted(conv_closed_now),
                   conn_new_rows=[r for _s, r in taken], conn_new_first=conn_first,
                   conv_new_rows=[v.row for v, _ in born], conv_new_first=[i for _, i in born],
                   conv_reborn_rows=[v.row for v, _ in reborn], conv_reborn_first=[i for _, i in reborn],
                   messages=list(self.queue[first_msg:]))
        streams = {}
        for i, v in enumerate(o["conv"]):
            if v is not None and o["kind"][i] == K_NONE:
                streams.setdefault(v.row, []).append(packets[i].payload)
        res["delivered"] = {r: b"".join(s) for r, s in streams.items()}
        self._end_event()
        return res

    # ---- INetGroup::doSend ----------------------------------------------------------------------------------------
    def pick(self, id8, draw, avoid=0, packet=None):
        cand = sorted((c for c in self.conns.get(id8, {}).values() if c.alive), key=lambda c: c.row)
        m = len(cand)
        if m == 0:
            return None
        a = self.conns.get(id8, {}).get(avoid) if avoid else None
        if a is not None and a.alive:
            if m == 1:
                raise SessionDeviation("a pick group whose only alive conn is the one to avoid", packet)
            p = cand.index(a)
            k = draw % (m - 1)
            return cand[k + (k >= p)]
        return cand[draw % m]

    def _send(self, c, cmd, id8, conv, payload):
        """INetConn::Output -> FakeTcp::Output -> RawTcp::SendRawTcp: the fields of the packet that leaves."""
        src, sp, dst, dp = c.tup
        s = dict(conn=c.row, src=src, dst=dst, sp=sp, dp=dp, seq=c.seq, ack=c.ack, flag=c.flag, ip_id=self.ip_id, cmd=cmd,
                 id8=id8, conv=conv, key=c.key, payload=payload)
        c.seq = (c.seq + HEAD + len(payload)) & M32
        self.ip_id = (self.ip_id + 1) & 0xFFFF
        c.new = False
        return s

    def send_queued(self, draws, tick=False):
        """The messages of the event before, in their order, each on the conn its draw picks."""
        out = []
        for k, (cmd, body, id8, avoid, src) in enumerate(self.queue):
            c = self.pick(id8, int(draws[k]), avoid, src)
            if c is None:
                out.append(None)
                continue
            if tick and c.new:
                raise SessionDeviation("a keepalive request carried by a conn that is still new in the same flush", src)
            out.append(self._send(c, cmd, id8, 0, int(body).to_bytes(8, "little")))
        self.queue = []
        self._end_event()
        return out

    def send(self, conv_rows, draws, payloads):
        """SubGroup::sconnSend -> IAppGroup::Send: one payload per conv row, on the conn the draw picks."""
        out = []
        for r, d, pay in zip(conv_rows, draws, payloads):
            v = self.conv_at[int(r)]
            c = self.pick(v.id8, int(d))
            if c is None:
                out.append(None)
                continue
            out.append(self._send(c, DATA, v.id8, v.conv, bytes(pay)))
            v.cur_out = (v.cur_out + 1) & M32
        self._end_event()
        return out

    # ---- the three timers -----------------------------------------------------------------------------------------
    def tick(self, now, which):
        res = {"ka_dead": [], "conn_closed": [], "conv_dead": [], "ack_dead": [], "sock_dead": [], "requests": []}
        if "ka" in which:  # NetConnKeepAlive::OnFlush, then IGroup::Flush's removal of the conns that are not alive
            for r in sorted(self.conn_at):
                c = self.conn_at[r]
                df = (now - c.est) & M32
                df = df - (1 << 32) if df >= 1 << 31 else df  # canSendRequest's `int df`
                if not c.new and now > c.est and df >= KA_DELAY_MS:
                    had = c.ka is not None
                    c.ka = c.ka + 1 if had else 0
                    if not had or c.ka < KA_MAX_RETRY:
                        self.queue.append((KA_REQ, c.key, c.id8, 0, r))
                if c.ka is not None and c.ka >= KA_MAX_RETRY:
                    c.ka = None
                    res["ka_dead"].append(r)
                    if c.alive:
                        self.seen["conns_timed_out"] += 1
                    c.alive = False  # onNetConnDead -> NotifyErr(ERR_TIMEOUT)
            for r in sorted(self.conn_at):
                c = self.conn_at[r]
                if not c.alive:  # INetGroup::RemoveConn
                    del self.conn_at[r], self.conns[c.id8][c.key]
                    self.r_conn.give(r)
                    self.closed.append(self.bound.pop(r))
                    res["conn_closed"].append(r)
            res["requests"] = list(self.queue)
        if "conv" in which:  # IGroup::Flush over the convs
            for r in sorted(self.conv_at):
                v = self.conv_at[r]
                if not v.alive:
                    del self.conv_at[r], self.convs[v.id8][(v.dst, v.conv)]
                    self.r_conv.give(r)
                    self.conv_closed.append((r, v.id8, v.dst, v.conv))
                    res["conv_dead"].append(r)
                else:
                    v.alive = int(v.prev_in != v.cur_in and v.prev_out != v.cur_out)
                    v.prev_in, v.prev_out = v.cur_in, v.cur_out
        if "pool" in which:  # TcpAckPool::OnFlush, ServerNetManager::OnFlush
            for t, e in sorted(self.ack_pool.items(), key=lambda x: x[1][0]):
                if e[3] <= now:
                    del self.ack_pool[t]
                    self.r_ack.give(e[0])
                    res["ack_dead"].append(e[0])
            for t, e in sorted(self.sock_pool.items(), key=lambda x: x[1][0]):
                if now >= e[1]:
                    del self.sock_pool[t]
                    self.r_sock.give(e[0])
                    self.closed.append(t)
                    res["sock_dead"].append(e[0])
            self.seen["pool_expired"] += len(res["ack_dead"]) + len(res["sock_dead"])
        self._end_event()
        return res

    # ---- what the tables must hold --------------------------------------------------------------------------------
    def snapshot(self):
        conn = {r: dict(state=LIVE | (ALIVE if c.alive else 0) | (NEW if c.new else 0), conn_key=c.key, id=c.id8, src=c.tup[0],
                        dst=c.tup[2], sp=c.tup[1], dp=c.tup[3], seq=c.seq, ack=c.ack, flag=c.flag,
                        ka_tries=KA_NONE if c.ka is None else c.ka, established_ms=c.est) for r, c in self.conn_at.items()}
        conv = {r: dict(state=LIVE, conv=v.conv, dst=v.dst, id=v.id8, cur_in=v.cur_in, cur_out=v.cur_out, prev_in=v.prev_in,
                        prev_out=v.prev_out, alive=v.alive) for r, v in self.conv_at.items()}
        ack = {e[0]: dict(state=LIVE, src=t[0], sp=t[1], dst=t[2], dp=t[3], seq=e[1], ack=e[2], expiry=e[3])
               for t, e in self.ack_pool.items()}
        sock = {e[0]: dict(state=LIVE, src=t[0], sp=t[1], dst=t[2], dp=t[3], expiry=e[1]) for t, e in self.sock_pool.items()}
        return {"conn": conn, "conv": conv, "ack": ack, "sock": sock, "bound": dict(self.bound), "closed": sorted(self.closed),
                "ip_id": self.ip_id}
