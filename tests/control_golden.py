"""TEST INFRASTRUCTURE: tests/golden/control.npz -- the control walk, the keepalive timer, doSend's pick and
the conv flush as the REFERENCE's own classes ran them (oracle/ref_control_harness.cpp through
tests/oracle_lib.RefControl; written by tests/golden/make_control_golden.py) -- and the scenarios that hold
rsk_control_batch, rsk_keepalive_flush, rsk_conn_pick_batch and rsk_conv_resolve / send / flush (or their
host twins: codec None, device "cpu") against it.  Every comparison is integer-exact.

The fixture stores inputs and recorded results only.  What both the generator and the live re-run
(tests/test_control_golden_host.py) need -- turning a case's inputs into a harness call and the event log
into the stored columns -- is the reference_* functions here; frames() lays a walk case's bodies out as the
frames rsk_control_batch reads."""
from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

from rsock_amd import _abi as A
from rsock_amd import workload
from tests import conn_ref as CR
from tests import control_ref as C
from tests import conv_ref as V
from tests import pick_ref as P

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "control.npz")
NONE = A.CONN_NONE
NO_RST = 0xFFFFFFFF
EV_MSG, EV_NOTIFY, EV_REMOVE, EV_CLOSE = 1, 2, 3, 4
F_ALIVE, F_NEW = 1, 2
ERR_TIMEOUT, ERR_FIN_RST = 1, 2
OP_FLUSH, OP_RESP, OP_REMOVE, OP_CLEAR_NEW, OP_ONLINE, OP_GROUP_FLUSH = range(6)
SERVER, CLIENT = 0, 1
ERR_NO_CONN = CR.ERR_NO_CONN
FAMILIES = ("walk", "timer", "send", "flush")
DST = 0x0A000002  # the server leaves' address (BuildConvKey(dst, conv))


@functools.lru_cache(maxsize=None)
def _npz():
    return dict(np.load(GOLDEN))


def names(family):
    return _npz()[family + "_names"].tolist()


SCALARS = ("shape", "seed", "n_draws", "online", "draws_used")  # stored together as one `meta` member per case


ABSENT = 2**64 - 1


def pack(c):
    """A case as it is stored: its scalars in one uint64 array, in the order of SCALARS (ABSENT: not a field)."""
    out = {k: np.asarray(v) for k, v in c.items() if k not in SCALARS}
    out["meta"] = np.array([int(c[k]) if k in c else ABSENT for k in SCALARS], np.uint64)
    return out


def unpack(c):
    c = dict(c)
    for k, v in zip(SCALARS, c.pop("meta").tolist()):
        if v != ABSENT:
            c[k] = np.uint64(v)
    return c


def case(family, name, z=None):
    z = z or _npz()
    p = f"{family[0]}{z[family + '_names'].tolist().index(name)}_"
    return unpack({k[len(p):]: v for k, v in z.items() if k.startswith(p)})


def draws_of(seed, n):
    """The rand() values of a case: 31 bits of each word of the splitmix64 stream of `seed`."""
    return (workload.splitmix64_np(int(seed), 0, int(n)) >> np.uint64(33)).astype(np.uint32)


def case_draws(c):
    return np.asarray(c["draws"], np.uint32) if "draws" in c else draws_of(c["seed"], c["n_draws"])


def id_word(c):
    return int(np.ascontiguousarray(c["id"], np.uint8).view(np.uint64)[0])


def events(ev, kind):
    ev = np.asarray(ev, np.int64).reshape(-1, 10)
    return ev[ev[:, 0] == kind]


# ---- the control walk -------------------------------------------------------------------------------------------
def walk_pay_len(c):
    """Body length per packet: the j-th control packet of each cmd takes C.LENS[j % 12], a packet marked force8
    eight; DATA 1 + i % 1399."""
    status, cmd = c["status"], c["cmd"]
    n = len(cmd)
    pay_len = (1 + np.arange(n) % 1399).astype(np.uint16)
    for cm in (1, 2, 3, 4):
        at = np.nonzero((status == A.RECV_VALID) & (cmd == cm))[0]
        pay_len[at] = np.array(C.LENS, np.uint16)[np.arange(len(at)) % len(C.LENS)]
    pay_len[c["force8"] == 1] = 8
    return pay_len


def walk_body_key(c):
    k = c["pool"][c["bk"]].astype(np.uint64)
    return np.where(c["cmd"] == A.CMD_CONV_RST, k & np.uint64(0xFFFFFFFF), k)


def frames(c, wild=False):
    """The frame columns of a walk case: the k-th body that is read lies at byte alignment k % 16, the arena
    holds exactly the bytes a body read may touch, and every other packet points nowhere near it with wild
    (the host side: reading one crashes).  No random numbers: the fixture fixes every byte."""
    status, cmd = c["status"], c["cmd"]
    n = len(cmd)
    i = np.arange(n)
    pay_len, key = walk_pay_len(c), walk_body_key(c)
    pay_off, inner_off = (31 + i % 9).astype(np.uint16), (i * 7 % 80).astype(np.uint16)
    base_off = np.full(n, 1 << 45 if wild else 0, np.uint64)
    parts, pos, k = [np.arange(256, dtype=np.uint8)], 256, 0
    for j in np.nonzero((status == A.RECV_VALID) & (cmd >= 1) & (cmd <= 4))[0].tolist():
        need = C.need_of(int(cmd[j]))
        if pay_len[j] < need:
            continue
        pad = (k % 16 - pos) % 16
        k += 1
        parts.append(np.full(pad, 0xC3, np.uint8))
        parts.append(np.frombuffer(int(key[j]).to_bytes(8, "little")[:need], np.uint8))
        base_off[j] = pos + pad - int(inner_off[j]) - int(pay_off[j])
        pos += pad + need
    return dict(arena=np.concatenate(parts), base_off=base_off, inner_off=inner_off, pay_off=pay_off, pay_len=pay_len)


def reference_walk(ref, c):
    """The case's VALID packets through the reference: -> the result columns the fixture stores."""
    vi = np.nonzero(c["status"] == A.RECV_VALID)[0]
    n = len(vi)
    pay_len, key = walk_pay_len(c)[vi], walk_body_key(c)[vi]
    body = np.full((n, 16), 0xA5, np.uint8)
    body[:, :8] = np.ascontiguousarray(key).view(np.uint8).reshape(n, 8)
    pool = c["pool"]
    req = {int(c["keys"][k]): int(t) for k, t in zip(c["req_conn"], c["req_tries"])}
    o = ref.control(int(c["shape"]), c["keys"], np.full(len(c["keys"]), F_ALIVE, np.uint8), c["id"], req, c["cmd"][vi],
                    np.tile(c["id"], n), np.zeros(n, np.uint32), pool[c["ck"]][vi], body.ravel(), 16 * np.arange(n),
                    np.minimum(pay_len, 16), case_draws(c))
    index = {int(k): j for j, k in enumerate(pool)}

    def pool_idx(v):  # 0 -> -1; every other value the reference sent is a key of the pool
        return np.array([-1 if int(x) == 0 else index[int(x) & (2**64 - 1)] for x in v], np.int32)

    m, nt, rm = events(o["ev"], EV_MSG), events(o["ev"], EV_NOTIFY), events(o["ev"], EV_REMOVE)
    assert bool((m[:, 5] == 8).all()) and bool((m[:, 8].astype(np.uint64) == np.uint64(id_word(c))).all())
    conn_of = {int(k): j for j, k in enumerate(c["keys"])}
    ret, look = np.zeros(len(c["cmd"]), np.int8), np.full(len(c["cmd"]), -2, np.int16)
    ret[vi], look[vi] = o["ret"], o["look"]
    return {"ret": ret, "look": look, "msg_src": vi[m[:, 1]].astype(np.uint32), "msg_conn": m[:, 2].astype(np.int16),
            "msg_cmd": m[:, 3].astype(np.uint8), "msg_body": pool_idx(m[:, 4]), "msg_avoid": pool_idx(m[:, 6]),
            "msg_draws": m[:, 7].astype(np.uint16), "nt_pkt": vi[nt[:, 1]].astype(np.uint32),
            "nt_conn": nt[:, 2].astype(np.int16), "nt_code": nt[:, 3].astype(np.uint8),
            "rm_pkt": vi[rm[:, 1]].astype(np.uint32), "rm_conn": rm[:, 2].astype(np.int16),
            "req_out_conn": np.array([conn_of[int(k)] for k in o["req_keys"]], np.int16),
            "req_out_tries": o["req_tries"].astype(np.uint8), "draws_used": np.uint32(o["draws_used"])}


WALK_RESULTS = ("ret", "look", "msg_src", "msg_conn", "msg_cmd", "msg_body", "msg_avoid", "msg_draws", "nt_pkt", "nt_conn",
                "nt_code", "rm_pkt", "rm_conn", "req_out_conn", "req_out_tries", "draws_used")


def walk_table(c, seed=7):
    """The case's conns at shuffled rows of a table twice their number: the unknown keys of the pool stand in
    rows that are not LIVE, and on a server also LIVE under another IdBuf.  -> (cols, capacity, row of conn)."""
    by_id = int(c["shape"]) == SERVER
    rng = np.random.default_rng(seed)
    nk, pool = len(c["keys"]), c["pool"]
    cap = 2 * len(pool) + 3
    cols = CR.random_columns(rng, cap, by_id=by_id)
    rows = rng.permutation(cap)
    row = rows[:nk]
    idb = np.ascontiguousarray(c["id"], np.uint8)
    CR.place(cols, row, c["keys"], id=np.tile(idb, nk) if by_id else None)
    unk = pool[nk:]
    spare = rows[nk:nk + len(unk)]
    cols["conn_key"][spare] = unk
    cols["state"][spare] = A.CONN_ALIVE
    if by_id:
        other = idb.copy()
        other[2] ^= 0x10
        cols["id"].reshape(-1, 8)[spare] = idb
        more = rows[nk + len(unk):nk + 2 * len(unk)]
        CR.place(cols, more, unk, id=np.tile(other, len(unk)))
    return cols, cap, row.astype(np.int64)


def scenario_walk(rc, name, device, codec=None):
    c = case("walk", name)
    by_id = int(c["shape"]) == SERVER
    n, nk, pool = len(c["cmd"]), len(c["keys"]), c["pool"]
    cols, cap, row = walk_table(c)
    tab = C.table_on(rc, cols, cap, by_id, device, codec)
    b = dict(status=c["status"], cmd=c["cmd"], id=np.tile(np.ascontiguousarray(c["id"], np.uint8), n), conn_key=pool[c["ck"]],
             tcp_sp=None, tcp_dp=None, miss=None)
    b.update(frames(c, wild=codec is None))
    # miss: the resolve's own column (rsk_conn_resolve_batch / its host twin)
    if codec is None:
        _conn, _hit, miss, _nm = rc.conn_resolve_host(tab, b["status"], b["conn_key"], cmd=b["cmd"], id=b["id"] if by_id else None)
    else:
        import torch

        t = lambda a, dt=None: C.tensor(a, device, dt)  # noqa: E731
        conn_t = torch.zeros(n, dtype=torch.int32, device=device)
        miss_t = torch.zeros(n, dtype=torch.int8, device=device)
        codec.conn_resolve_batch(tab, t(b["status"]), t(b["conn_key"], np.int64), conn_t, cmd=t(b["cmd"]),
                                 id=t(b["id"]) if by_id else None, miss=miss_t)
        torch.cuda.synchronize()
        miss = miss_t.cpu().numpy()
    b["miss"] = np.ascontiguousarray(miss, np.int8)
    tries0 = np.full(cap, A.KA_NONE, np.uint8)
    tries0[row[c["req_conn"]]] = c["req_tries"]
    got = C.run_control(rc, tab, b, device, codec, ka_tries=tries0)
    # the model agrees with the kernel (so a failure below is the restatement's, not only the kernel's)
    tmap, _ = CR.table_map(cols["state"], cols["conn_key"], cols["id"])
    C.compare(got, C.snapshot_ref(b, tmap, cap, by_id, tries0))

    valid, cmd, pay_len = c["status"] == A.RECV_VALID, c["cmd"], b["pay_len"]
    kind, arg, conn, ret, look = got["kind"], got["arg"], got["conn"], c["ret"].astype(np.int64), c["look"].astype(np.int64)
    # 1. kind and arg: the branch the reference took and the body it decoded
    full = valid & (cmd >= 1) & (cmd <= 4) & (pay_len >= np.where(cmd == 1, 4, 8))
    want_kind = np.where(~valid | (cmd == 0), A.CTL_NONE, np.where(cmd > 4, A.CTL_UNKNOWN, np.where(full, cmd, A.CTL_SHORT)))
    assert np.array_equal(kind, want_kind.astype(np.uint8))
    assert bool((ret[(kind == A.CTL_SHORT) | (kind == A.CTL_UNKNOWN)] == -1).all())
    ka = (kind == A.CTL_KA_REQ) | (kind == A.CTL_KA_RESP)
    assert np.array_equal(ret[ka], np.minimum(pay_len[ka], 16).astype(np.int64))  # nread: the body was accepted
    rst = kind == A.CTL_NETCONN_RST
    assert np.array_equal(ret[rst], np.where(look[rst] >= 0, 0, -1))
    assert bool((look[kind < 2] == -2).all()) and bool((look[kind > 4] == -2).all())
    data = valid & (cmd == 0)
    assert np.array_equal(ret[data] == ERR_NO_CONN, miss[data] == A.RECV_VALID) and bool((ret[data & (miss != 1)] > 0).all())
    assert np.array_equal(arg, np.where(full, walk_body_key(c), 0).astype(np.uint64))
    keyed = full & (cmd >= 2)
    named = look >= 0  # the reference's own lookup names the conn whose key the kernel decoded
    assert np.array_equal(c["keys"][look[named]], arg[named])
    # 2. conn: the reference's lookup, until a doSend has drawn the dead conn and removed it
    removed_at = np.full(nk, n, np.int64)
    removed_at[c["rm_conn"]] = c["rm_pkt"]
    first_rst = np.full(nk, n, np.int64)
    fin = c["nt_code"] == ERR_FIN_RST
    assert bool(fin.all())
    np.minimum.at(first_rst, c["nt_conn"][fin].astype(np.int64), c["nt_pkt"][fin].astype(np.int64))
    assert bool((removed_at >= first_rst).all())  # only a dead conn is removed, and only a reset kills one here
    conn_of_row = np.full(cap, -1, np.int64)
    conn_of_row[row] = np.arange(nk)
    i = np.nonzero(keyed)[0]
    snap = np.where(conn[i] != NONE, conn_of_row[np.minimum(conn[i], cap - 1)], -1)
    assert bool((conn[~keyed] == NONE).all())
    gone = (snap >= 0) & (i > removed_at[np.maximum(snap, 0)])
    assert np.array_equal(look[i][~gone], snap[~gone])        # the snapshot is the reference's lookup ...
    assert bool((look[i][gone] == -1).all())                  # ... until the conn has left mConnMap
    # the header's guarantee: every packet at or before its row's rst_first
    rf = got["rst_first"]
    early = (snap < 0) | (i <= np.where(snap >= 0, rf[row[np.maximum(snap, 0)]], NO_RST))
    assert np.array_equal(look[i][early], snap[early])
    # and past rst_first: the conn is still found as long as nothing was sent through doSend's removal
    late = ~early
    assert np.array_equal(look[i][late] >= 0, ~gone[late])
    # 3. rst_first: the first NotifyErr(ERR_FIN_RST) per conn
    want_rf = np.full(cap, NO_RST, np.uint32)
    hit = first_rst < n
    want_rf[row[hit]] = first_rst[hit]
    assert np.array_equal(rf, want_rf)
    # 4. the messages, in order
    m = got["msgs"]
    k = got["n_msg"]
    assert k == len(c["msg_src"]) and np.array_equal(m["src"], c["msg_src"])
    pk = lambda idx: np.where(idx >= 0, pool[np.maximum(idx, 0)], 0).astype(np.uint64)  # noqa: E731
    ref_body, ref_avoid, ref_cmd = pk(c["msg_body"]), pk(c["msg_avoid"]), c["msg_cmd"]
    src = c["msg_src"].astype(np.int64)
    gone_msg = np.zeros(k, bool)  # answers to a KA_REQ whose conn a doSend had removed: RESP here, RST there
    where = {int(p): j for j, p in enumerate(i)}
    for j in np.nonzero(kind[src] == A.CTL_KA_REQ)[0].tolist():
        gone_msg[j] = gone[where[int(src[j])]]
    ok = ~gone_msg
    assert np.array_equal(m["cmd"][ok], ref_cmd[ok]) and np.array_equal(m["body"], ref_body)
    assert np.array_equal(m["avoid_key"][ok], ref_avoid[ok])
    assert bool((ref_cmd[gone_msg] == A.CMD_NETCONN_RST).all()) and np.array_equal(ref_avoid[gone_msg], ref_body[gone_msg])
    assert bool((m["cmd"][gone_msg] == A.CMD_KEEP_ALIVE_RESP).all()) and bool((m["avoid_key"][gone_msg] == 0).all())
    assert np.array_equal(m["id"], np.tile(np.ascontiguousarray(c["id"], np.uint8), (k, 1)))
    # 5. ka_tries: mReqMap after the walk, row by row
    want_tries = np.full(cap, A.KA_NONE, np.uint8)
    want_tries[row[c["req_out_conn"]]] = c["req_out_tries"]
    assert np.array_equal(got["ka_tries"], want_tries)
    return {"n_gone": int(gone.sum()), "n_late": int(late.sum()), "n_late_found": int((look[i][late] >= 0).sum()),
            "n_msg": k, "n_removed": len(c["rm_conn"])}


# ---- the keepalive timer ------------------------------------------------------------------------------------------
def reference_timer(ref, c):
    allk = np.concatenate([c["keys"], c["extra"]]).astype(np.uint64)
    req = {int(allk[k]): int(t) for k, t in zip(c["req_key"], c["req_tries"])}
    op = c["op"]
    arg = np.where(np.isin(op, (OP_RESP, OP_REMOVE, OP_CLEAR_NEW)), allk[np.minimum(c["arg"], len(allk) - 1).astype(np.int64)],
                   c["arg"]).astype(np.uint64)
    o = ref.keepalive(int(c["shape"]), c["keys"], c["flags"], c["est"], c["id"], req, int(c["online"]), op, arg, case_draws(c))
    index = {int(k): j for j, k in enumerate(allk)}
    m, nt, rm = events(o["ev"], EV_MSG), events(o["ev"], EV_NOTIFY), events(o["ev"], EV_REMOVE)
    assert bool((m[:, 3] == A.CMD_KEEP_ALIVE_REQ).all()) and bool((m[:, 6] == 0).all())
    return {"snd_step": m[:, 1].astype(np.uint16), "snd_key": np.array([index[int(x)] for x in m[:, 4]], np.int16),
            "snd_conn": m[:, 2].astype(np.int16), "nt_step": nt[:, 1].astype(np.uint16), "nt_conn": nt[:, 2].astype(np.int16),
            "nt_code": nt[:, 3].astype(np.uint8), "rm_step": rm[:, 1].astype(np.uint16), "rm_conn": rm[:, 2].astype(np.int16),
            "snap_step": o["snap_step"].astype(np.uint16), "snap_key": np.array([index[int(x)] for x in o["snap_key"]], np.int16),
            "snap_tries": o["snap_tries"].astype(np.uint8), "draws_used": np.uint32(o["draws_used"])}


TIMER_RESULTS = ("snd_step", "snd_key", "snd_conn", "nt_step", "nt_conn", "nt_code", "rm_step", "rm_conn", "snap_step",
                 "snap_key", "snap_tries", "draws_used")


def scenario_timer(rc, name, device, codec=None):
    """The script step by step: the flushes through rsk_keepalive_flush, every other step applied to the
    columns by the host.  The extra keys (requests of keys that have no conn) stand in rows
    that are not LIVE."""
    c = case("timer", name)
    by_id = int(c["shape"]) == SERVER
    nk, ne = len(c["keys"]), len(c["extra"])
    cap = nk + ne + 2
    rng = np.random.default_rng(nk)
    cols = CR.random_columns(rng, cap, by_id=by_id)
    row = rng.permutation(cap)[:nk + ne].astype(np.int64)  # of conn / extra key k
    cols["conn_key"][row] = np.concatenate([c["keys"], c["extra"]])
    fl = c["flags"].astype(np.uint8)
    cols["state"][row[:nk]] = A.CONN_LIVE | np.where(fl & F_ALIVE, A.CONN_ALIVE, 0) | np.where(fl & F_NEW, A.CONN_NEW, 0)
    if by_id:
        cols["id"].reshape(-1, 8)[:] = np.ascontiguousarray(c["id"], np.uint8)
    est = rng.integers(0, 2**62, cap, dtype=np.uint64)
    est[row[:nk]] = c["est"]
    tries = np.full(cap, A.KA_NONE, np.uint8)
    tries[row[c["req_key"]]] = c["req_tries"]
    tab = CR.make_table(rc, cols, cap, device, by_id=by_id)
    online = bool(c["online"])
    state = cols["state"]
    conn_of_row = np.full(cap, -1, np.int64)
    conn_of_row[row] = np.arange(nk + ne)
    flushes = sent_total = dead_total = 0
    for s, (op, arg) in enumerate(zip(c["op"].tolist(), c["arg"].tolist())):
        if op == OP_FLUSH:
            tries, msgs, dead = C.run_flush(rc, tab, tries, est, int(arg), device, codec, online=online)
            want = c["snd_key"][c["snd_step"] == s]
            got_rows = msgs["src"].astype(np.int64)
            assert bool((np.diff(got_rows) > 0).all())  # ours go out in row order, the reference's in mConns order
            assert sorted(conn_of_row[got_rows].tolist()) == sorted(want.tolist()), s
            C.check_flush_msgs(msgs, got_rows, cols)  # bodies = the rows' keys
            to = c["nt_conn"][(c["nt_step"] == s) & (c["nt_code"] == ERR_TIMEOUT)]
            assert bool((np.diff(dead.astype(np.int64)) > 0).all())
            assert sorted(conn_of_row[dead.astype(np.int64)].tolist()) == sorted(to.tolist()), s
            want_tries = np.full(cap, A.KA_NONE, np.uint8)
            at = c["snap_step"] == s
            want_tries[row[c["snap_key"][at]]] = c["snap_tries"][at]
            assert np.array_equal(tries, want_tries), s
            # the host's part: a timed-out conn is dead (NotifyErr), a conn that carried a request is not new
            state[dead.astype(np.int64)] &= np.uint8(~A.CONN_ALIVE & 0xFF)
            carriers = c["snd_conn"][(c["snd_step"] == s) & (c["snd_conn"] >= 0)]
            state[row[carriers]] &= np.uint8(~A.CONN_NEW & 0xFF)
            flushes += 1
            sent_total += len(want)
            dead_total += len(to)
        elif op == OP_RESP:
            tries[row[arg]] = A.KA_NONE  # rsk_control_batch: a KA_RESP whose conn is r (RemoveRequest by key)
        elif op == OP_REMOVE:
            state[row[arg]] = 0
        elif op == OP_CLEAR_NEW:
            state[row[arg]] &= np.uint8(~A.CONN_NEW & 0xFF)
        elif op == OP_ONLINE:
            online = bool(arg)
            tries[:] = A.KA_NONE  # RemoveAllRequest
        state[row[c["rm_conn"][c["rm_step"] == s]]] = 0  # the conns the reference's group dropped at this step
        tab.load(state=state)
    return {"flushes": flushes, "sent": sent_total, "dead": dead_total}


# ---- doSend -----------------------------------------------------------------------------------------------------
def reference_send(ref, c):
    allk = np.concatenate([c["keys"], c["extra"]]).astype(np.uint64)
    avoid = np.where(c["avoid"] >= 0, allk[np.maximum(c["avoid"], 0)], 0).astype(np.uint64)
    o = ref.dosend(int(c["shape"]), c["keys"], c["flags"], c["id"], avoid, case_draws(c))
    m, rm = events(o["ev"], EV_MSG), events(o["ev"], EV_REMOVE)
    assert len(m) == len(avoid) and np.array_equal(m[:, 1], np.arange(len(avoid)))
    assert np.array_equal(m[:, 9] == ERR_NO_CONN, m[:, 2] < 0)
    return {"order": o["order"].astype(np.int32), "sender": m[:, 2].astype(np.int16), "consumed": m[:, 7].astype(np.uint16),
            "rm_step": rm[:, 1].astype(np.uint32), "rm_conn": rm[:, 2].astype(np.int16), "draws_used": np.uint32(o["draws_used"])}


SEND_RESULTS = ("order", "sender", "consumed", "rm_step", "rm_conn", "draws_used")


def send_inputs(c):
    """-> (avoid keys [n], the draw each send ended on [n]: the reference's consumed draw)."""
    allk = np.concatenate([c["keys"], c["extra"]]).astype(np.uint64)
    avoid = np.where(c["avoid"] >= 0, allk[np.maximum(c["avoid"], 0)], 0).astype(np.uint64)
    end = np.cumsum(c["consumed"].astype(np.int64))
    assert int(end[-1]) == int(c["draws_used"])
    d = case_draws(c)
    return avoid, np.where(c["consumed"] > 0, d[np.maximum(end - 1, 0)], 0).astype(np.uint32)


def send_table(c, order):
    """A table whose rows stand in `order` (conn indices): -> (cols, row of conn)."""
    by_id = int(c["shape"]) == SERVER
    nk = len(c["keys"])
    cols = CR.random_columns(np.random.default_rng(nk), nk, by_id=by_id)
    order = np.asarray(order, np.int64)
    cols["conn_key"][:] = c["keys"][order]
    alive = (c["flags"][order] & F_ALIVE) != 0
    cols["state"][:] = np.where(alive, P.UP, A.CONN_LIVE).astype(np.uint8)
    if by_id:
        cols["id"].reshape(-1, 8)[:] = np.ascontiguousarray(c["id"], np.uint8)
    row = np.empty(nk, np.int64)
    row[order] = np.arange(nk)
    return cols, row


def is_exact_send(c):
    """All alive and no avoid key inside the group: the reference consumes one draw per send."""
    return bool((c["flags"] & F_ALIVE).all()) and not bool(((c["avoid"] >= 0) & (c["avoid"] < len(c["keys"]))).any())


SIGMA5 = 403  # 5 * sqrt(65536 * (1/9) * (8/9)) = 5 * 80.45


def check_uniform(picks, allowed):
    """The 65,536-send case: each of the 9 allowed conns within 5 sigma of N / 9."""
    cnt = np.bincount(np.asarray(picks, np.int64), minlength=int(max(allowed)) + 1)[np.asarray(allowed, np.int64)]
    assert int(cnt.sum()) == len(picks) and len(allowed) == 9
    assert bool((np.abs(cnt - len(picks) / 9.0) <= SIGMA5).all()), cnt


def set_pick_path(rc, codec, path):
    """The library's internal switch (tools/bench_paths.py): 0 by the table, 1 plain, 2 staged."""
    f = rc.lib().rsk__set_pick_path
    f.argtypes, f.restype = [ctypes.c_void_p, ctypes.c_int], ctypes.c_int
    assert f(codec._ctx, path) == A.OK


def scenario_send(rc, name, device, codec=None, path=None):
    """path (device only): None = the entry point's own choice, 1 = candidates from global memory, 2 = staged."""
    c = case("send", name)
    by_id = int(c["shape"]) == SERVER
    n, nk = len(c["avoid"]), len(c["keys"])
    avoid, draw = send_inputs(c)
    idcol = np.tile(np.ascontiguousarray(c["id"], np.uint8), n) if by_id else None
    sender = c["sender"].astype(np.int64)
    # the group's order is the string order of StrForIntKey
    assert c["order"].tolist() == sorted(range(nk), key=lambda k: str(int(c["keys"][k])))
    if path is not None:
        set_pick_path(rc, codec, path)
    try:
        cols, row = send_table(c, c["order"])
        tab = P.make_table(rc, cols, by_id, device, codec)
        conn, n_none, used = P.run_pick(rc, tab, n, device, codec, id=idcol, avoid_key=avoid, draw=draw)
        P.compare((conn, n_none, used), P.rule_ref(cols, by_id, n, id=idcol, avoid_key=avoid, draw=draw))
        want = np.where(sender >= 0, row[np.maximum(sender, 0)], NONE).astype(np.uint32)
        exact = is_exact_send(c)
        if exact:
            assert bool((c["consumed"] == 1).all()) and np.array_equal(conn, want)
        # in every case: never a dead or the avoided conn, NONE where the reference had no conn, used = the picks
        dead_rows = np.nonzero((cols["state"] & P.UP) != P.UP)[0]
        assert not np.isin(conn, dead_rows).any()
        inside = (c["avoid"] >= 0) & (c["avoid"] < nk)
        assert not bool((conn[inside] == row[c["avoid"][inside]]).any())
        assert np.array_equal(conn == NONE, sender < 0) and n_none == int((sender < 0).sum())
        mark = np.zeros(nk, np.uint8)
        mark[conn[conn != NONE]] = 1
        assert np.array_equal(used, mark)
        differ = None
        if exact and nk >= 2:  # the layout requirement is real: rows in numeric key order miss the reference's picks
            ncols, nrow = send_table(c, np.argsort(c["keys"], kind="stable"))
            ntab = P.make_table(rc, ncols, by_id, device, codec)
            nconn, _nn, _u = P.run_pick(rc, ntab, n, device, codec, id=idcol, avoid_key=avoid, draw=draw)
            nwant = np.where(sender >= 0, nrow[np.maximum(sender, 0)], NONE).astype(np.uint32)
            differ = int((nconn != nwant).sum())
            assert differ > 0, "numeric row order reproduced the reference: the keys are badly chosen"
    finally:
        if path is not None:
            set_pick_path(rc, codec, 0)
    return {"conn": conn, "row": row, "exact": exact, "differ": differ}


# ---- the conv flush -----------------------------------------------------------------------------------------------
def reference_flush(ref, c):
    o = ref.convflush(int(c["shape"]), c["net_key"], c["id"], c["convs"], DST, c["in_off"], c["convs"][c["in_leaf"]], c["out_off"],
                      c["out_leaf"], c["out_ret"], c["now"])
    cl = events(o["ev"], EV_CLOSE)
    assert bool((o["in_ret"] == 32).all()) and o["draws_used"] == 0
    return {"alive": o["alive"], "counters": o["counters"], "cl_round": cl[:, 1].astype(np.uint8), "cl_leaf": cl[:, 2].astype(np.int16)}


FLUSH_RESULTS = ("alive", "counters", "cl_round", "cl_leaf")


def scenario_flush(rc, name, device, codec=None):
    c = case("flush", name)
    server = int(c["shape"]) == SERVER
    nc = len(c["convs"])
    cap = nc + 3
    rng = np.random.default_rng(nc)
    cols = V.random_columns(rng, cap, by_dst=server, by_id=server)
    row = np.sort(rng.permutation(cap)[:nc]).astype(np.int64) if nc % 2 else rng.permutation(cap)[:nc].astype(np.int64)
    cols["conv"][row] = c["convs"]
    if server:
        cols["dst"][row] = DST
        cols["id"].reshape(-1, 8)[row] = np.ascontiguousarray(c["id"], np.uint8)
    cols["state"][row] = A.CONN_LIVE
    for k in V.COUNTERS:
        cols[k][:] = 0  # a new conn's DataStat
    tab = V.make_table(rc, cols, device, server, server, codec)
    state = cols["state"].copy()
    leaf_of_row = np.full(cap, -1, np.int64)
    leaf_of_row[row] = np.arange(nc)
    closed_total = 0
    for r in range(len(c["now"])):
        lo, hi = int(c["in_off"][r]), int(c["in_off"][r + 1])
        k = hi - lo
        if k:
            leaf = c["in_leaf"][lo:hi].astype(np.int64)
            b = {"status": np.ones(k, np.int8), "cmd": np.zeros(k, np.uint8), "conv": c["convs"][leaf],
                 "id": np.tile(np.ascontiguousarray(c["id"], np.uint8), k) if server else None,
                 "dst": np.full(k, DST, np.uint32) if server else None, "hit": None, "ctl_kind": None, "ctl_arg": None}
            got = V.run_resolve(rc, tab, b, device, codec, msg_mode="count")
            assert got["tail_ok"] and np.array_equal(got["conv_row"], row[leaf].astype(np.uint32)) and got["n_unknown"] == 0
        lo, hi = int(c["out_off"][r]), int(c["out_off"][r + 1])
        if hi > lo:
            V.run_send(rc, tab, row[c["out_leaf"][lo:hi].astype(np.int64)].astype(np.uint32), device, codec,
                       sent=c["out_ret"][lo:hi].astype(np.int32), cols=())
        got = V.run_flush(rc, tab, device, codec)
        closed = c["cl_leaf"][c["cl_round"] == r].astype(np.int64)
        assert bool((np.diff(got["dead_rows"].astype(np.int64)) > 0).all())
        assert sorted(leaf_of_row[got["dead_rows"].astype(np.int64)].tolist()) == sorted(closed.tolist()), r
        alive = c["alive"][r]
        there = alive >= 0
        assert not there[closed].any()
        assert np.array_equal(tab.column("alive")[row[there]], alive[there].astype(np.uint8)), r
        for j, name_ in enumerate(("cur_in", "cur_out", "prev_in", "prev_out")):
            assert np.array_equal(tab.column(name_)[row[there]], c["counters"][r][there, j]), (r, name_)
        assert got["n_alive"] == int((alive == 1).sum()), r
        closed_total += len(closed)
        if len(closed):  # IGroup::CloseConn: the host frees the rows the flush listed
            state[got["dead_rows"].astype(np.int64)] = 0
            tab.load(state=state)
            tab.rebuild(codec)
    return {"closed": closed_total}
